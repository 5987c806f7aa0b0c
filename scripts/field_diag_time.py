"""field_diagnostics at the headline shape, device against host: three chains'
blocks of ROWS x N seeded AR(1) samples (default 300 x 1e6: 7.2 GB) with one
offset per row.  The device path (nngp_field_diag: blocks passed where they
lie) is timed as the median of three runs after one warm run, with the
HIP-event times of its staging copies and kernels; the host backend (numpy)
runs once on the first HOST_COLS columns (default 20000; the subset is
stated in the output).  Prints one JSON line.
argv: [N [ROWS [CHUNK_COLS [HOST_COLS]]]]"""
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
argv = sys.argv[1:]
n = int(float(argv[0])) if len(argv) > 0 else 1_000_000
rows = int(argv[1]) if len(argv) > 1 else 300
chunk_cols = int(argv[2]) if len(argv) > 2 else 0
host_cols = min(n, int(argv[3]) if len(argv) > 3 else 20_000)
rng = np.random.default_rng(8)
blocks = []
for k in range(3):
    x = rng.standard_normal((rows, n))
    for t in range(1, rows):  # AR(1), rho = .9
        x[t] += 0.9 * x[t - 1]
    blocks.append(x + 0.3 * k)
off = 0.1 * rng.standard_normal(3 * rows)

diag = P.diagnose
dev = diag.field_diagnostics(blocks, row_offset=off, backend="hip", device=0, chunk_cols=chunk_cols)  # warm
runs = []
for _ in range(3):
    t = time.perf_counter()
    dev = diag.field_diagnostics(blocks, row_offset=off, backend="hip", device=0, chunk_cols=chunk_cols)
    wall = time.perf_counter() - t
    runs.append(dict(diag.field_diagnostics_stats(), wall_s=wall))
wall_s = statistics.median(r["wall_s"] for r in runs)
mid = min(runs, key=lambda r: abs(r["wall_s"] - wall_s))

t = time.perf_counter()
host = diag.field_diagnostics([b[:, :host_cols] for b in blocks], row_offset=off)
host_s = time.perf_counter() - t
with np.errstate(all="ignore"):
    rel = np.abs(dev[:host_cols] - host) / np.abs(host)
print(json.dumps({
    "n": n, "rows_per_chain": rows, "chains": 3, "matrix_bytes": 8 * 3 * rows * n,
    "device_s_median3": round(wall_s, 4), "device_s_runs": [round(r["wall_s"], 4) for r in runs],
    "copy_ms_events": round(mid["copy_ms"], 2), "kernel_ms_events": round(mid["kernel_ms"], 2),
    "kernel_below_copy": bool(mid["kernel_ms"] < mid["copy_ms"]),
    "staged_bytes": mid["staged_bytes"], "chunk_cols": mid["chunk_cols"],
    "host_cols": host_cols, "host_s_on_subset": round(host_s, 4),
    "host_s_scaled_to_n": round(host_s * n / host_cols, 2),
    "max_rel_diff_vs_host_on_subset": [float(np.nanmax(rel[:, j])) for j in range(5)],
}), flush=True)
