"""pointwise_loglik at the headline size, device against host: S = 900 saved
field rows (three chains of 300) over N locations (default 1e6), one
observation per location, and a regression term of q = 2 (the pollution pair)
and q = 156 (the full Heavy_metals design) columns.  Per q the device path
(nngp_pointwise_loglik) is timed as the median of three calls after a warming
one, with pointwise_loglik_stats beside the wall time.  The figure to set it
against is effects_summary with the same three blocks as its addend (q = 2),
timed the same way in the same process: it stages the same bytes.  The host
backend (numpy) runs once at HOST_N observations (default 1e5) of the same
problem; the line carries its time and the figure scaled to N, marked as not
run.  Prints one JSON line per case.
argv: [N [HOST_N]] [nohost] [noeffects]"""
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _pkgload  # noqa: E402

P = _pkgload.load()
argv = [a for a in sys.argv[1:] if a not in ("nohost", "noeffects")]
with_host, with_effects = "nohost" not in sys.argv, "noeffects" not in sys.argv
n = int(float(argv[0])) if len(argv) > 0 else 1_000_000
host_n = min(n, int(float(argv[1])) if len(argv) > 1 else 100_000)
ROWS, CHAINS = 300, 3
S = ROWS * CHAINS
rng = np.random.default_rng(8)
blocks = [0.3 * k + rng.standard_normal((ROWS, n)) for k in range(CHAINS)]
lnv = rng.standard_normal(S) * 0.2 - 0.5
y = 0.3 + rng.standard_normal(n) * 1.3
loc = np.arange(1, n + 1, dtype=np.int32)


def median3(call, stats):
    call()  # warm
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        res = call()
        runs.append(dict(stats(), wall_s=time.perf_counter() - t))
    wall_s = statistics.median(r["wall_s"] for r in runs)
    mid = min(runs, key=lambda r: abs(r["wall_s"] - wall_s))
    line = {"n": n, "S": S, "device_s_median3": round(wall_s, 4), "device_s_runs": [round(r["wall_s"], 4) for r in runs]}
    line.update({k + "_events": round(v, 2) for k, v in mid.items() if k.endswith("_ms")})
    line.update({"staged_bytes": mid["staged_bytes"], "chunk_cols": mid["chunk_cols"]})
    return res, line


for q in (2, 156):
    coef = rng.standard_normal((S, q)) / np.sqrt(q)
    X = rng.standard_normal((q, n)).T  # n x q, column-major storage
    dev, line = median3(lambda: P.pointwise_loglik(y, loc, blocks, lnv, coef=coef, X=X, backend="hip", device=0),
                        P.estimate.pointwise_loglik_stats)
    line = dict({"case": "pointwise_loglik", "q": q}, **line)
    if with_host:
        t = time.perf_counter()
        host = P.pointwise_loglik(y[:host_n], loc[:host_n], [b[:, :host_n] for b in blocks], lnv, coef=coef,
                                  X=X[:host_n])
        host_s = time.perf_counter() - t
        line.update({"host_n": host_n, "host_s": round(host_s, 4),
                     "host_s_scaled_to_n_not_run": None if host_n == n else round(host_s * n / host_n, 2),
                     "speedup_device_vs_host_scaled": round(host_s * n / host_n / line["device_s_median3"], 2),
                     "max_abs_diff_vs_host": float(np.nanmax(np.abs(dev[:host_n] - host)))})
    print(json.dumps(line), flush=True)
    if q == 2 and with_effects:
        _, eline = median3(lambda: P.effects_summary(coef, X, addend=blocks, backend="hip", device=0),
                           P.estimate.effects_stats)
        print(json.dumps(dict({"case": "effects_summary with the blocks as addend", "q": q}, **eline)), flush=True)
