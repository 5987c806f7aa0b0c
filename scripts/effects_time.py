"""effects_summary at the reference's two sizes, host against device: S = 900
coefficient rows (three chains of 300), N new locations (default 1e6) and a
design of q = 2 (the pollution pair) and q = 156 (the full Heavy_metals
design) columns.  Per q the device path (nngp_effects_summary, no sample on the
host) is timed as the median of five calls after a warming one, with
effects_stats beside the wall time; then once more (q = 2) with an addend of
three 300 x N blocks.  The baseline is the host path of
mcmc_nngp_predict_fixed_effects (the product per chain, a vstack, the numpy
get_summary) in the same process at HOST_N locations (default 1e5: at 1e6 its
matrix and the stacked copy are 14.4 GB); the line carries its time and the
figure scaled to N, marked as not run.  Prints one JSON line per case.
argv: [N [HOST_N]] [nohost] [noaddend]"""
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
argv = [a for a in sys.argv[1:] if a not in ("nohost", "noaddend")]
with_host, with_addend = "nohost" not in sys.argv, "noaddend" not in sys.argv
n = int(float(argv[0])) if len(argv) > 0 else 1_000_000
host_n = min(n, int(float(argv[1])) if len(argv) > 1 else 100_000)
ROWS, CHAINS = 300, 3
S = ROWS * CHAINS
rng = np.random.default_rng(8)


def timed(coef, X, **kw):
    t = time.perf_counter()
    res = P.effects_summary(coef, X, backend="hip", device=0, **kw)
    wall = time.perf_counter() - t
    return res, dict(P.estimate.effects_stats(), wall_s=wall)


def device_case(label, coef, X, **kw):
    dev, _ = timed(coef, X, **kw)  # warm
    runs = [timed(coef, X, **kw)[1] for _ in range(5)]
    wall_s = statistics.median(r["wall_s"] for r in runs)
    mid = min(runs, key=lambda r: abs(r["wall_s"] - wall_s))
    return dev, {"case": label, "n": n, "S": S, "q": coef.shape[1], "device_s_median5": round(wall_s, 4),
                 "device_s_runs": [round(r["wall_s"], 4) for r in runs],
                 "copy_ms_events": round(mid["copy_ms"], 2), "generate_ms_events": round(mid["generate_ms"], 2),
                 "kernel_ms_events": round(mid["kernel_ms"], 2), "staged_bytes": mid["staged_bytes"],
                 "chunk_cols": mid["chunk_cols"]}


for q in (2, 156):
    coef = rng.standard_normal((S, q)) / np.sqrt(q)
    X = rng.standard_normal((q, n)).T  # n x q, column-major storage: passed where it lies
    dev, line = device_case("fixed effects", coef, X)
    if with_host:
        Xh = X[:host_n]
        t = time.perf_counter()
        out = [coef[k * ROWS:(k + 1) * ROWS] @ Xh.T for k in range(CHAINS)]
        host = P.get_summary(np.vstack(out))
        host_s = time.perf_counter() - t
        del out
        line.update({"host_n": host_n, "host_s": round(host_s, 4),
                     "host_s_scaled_to_n_not_run": None if host_n == n else round(host_s * n / host_n, 2),
                     "speedup_device_vs_host_scaled": round(host_s * n / host_n / line["device_s_median5"], 2),
                     "max_abs_diff_vs_host": float(np.nanmax(np.abs(dev[:host_n] - host)))})
    print(json.dumps(line), flush=True)
    if q == 2 and with_addend:
        blocks = [0.3 * k + rng.standard_normal((ROWS, n)) for k in range(CHAINS)]
        _, line = device_case("response (addend of three blocks)", coef, X, addend=blocks)
        del blocks
        print(json.dumps(line), flush=True)
