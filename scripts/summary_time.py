"""get_summary at the headline shape, host against device: three chains'
blocks of ROWS x N seeded normals (default 100 x 1e6: 2.4 GB) with one offset
per row.  The host path (stack, centre, numpy) is timed once; the device path
(nngp_summary: blocks passed where they lie) as the median of five runs after
one warm run, with the HIP-event times of its staging copies and kernels.
Prints one JSON line.  argv: [N [ROWS [CHUNK_COLS]]] [nohost] (nohost skips
the host path); NNGP_SUMMARY_BITS picks the digit width of the radix select
(2 or 4)."""
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _pkgload  # noqa: E402

P = _pkgload.load()
argv = [a for a in sys.argv[1:] if a != "nohost"]
with_host = "nohost" not in sys.argv[1:]
n = int(float(argv[0])) if len(argv) > 0 else 1_000_000
rows = int(argv[1]) if len(argv) > 1 else 100
chunk_cols = int(argv[2]) if len(argv) > 2 else 0
rng = np.random.default_rng(8)
blocks = [0.3 * k + rng.standard_normal((rows, n)) for k in range(3)]
off = 0.1 * rng.standard_normal(3 * rows)

host, host_s = None, None
if with_host:
    t = time.perf_counter()
    host = P.get_summary(blocks, row_offset=off)
    host_s = time.perf_counter() - t

dev = P.get_summary(blocks, backend="hip", device=0, row_offset=off, chunk_cols=chunk_cols)  # warm
runs = []
for _ in range(5):
    t = time.perf_counter()
    dev = P.get_summary(blocks, backend="hip", device=0, row_offset=off, chunk_cols=chunk_cols)
    wall = time.perf_counter() - t
    runs.append(dict(P.estimate.summary_stats(), wall_s=wall))
wall_s = statistics.median(r["wall_s"] for r in runs)
mid = min(runs, key=lambda r: abs(r["wall_s"] - wall_s))
print(json.dumps({
    "n": n, "rows_per_block": rows, "blocks": 3, "matrix_bytes": 8 * 3 * rows * n,
    "summary_bits": int(os.environ.get("NNGP_SUMMARY_BITS", "4")),
    "host_s": host_s and round(host_s, 4), "device_s_median5": round(wall_s, 4),
    "device_s_runs": [round(r["wall_s"], 4) for r in runs],
    "speedup_device_vs_host": host_s and round(host_s / wall_s, 2),
    "copy_ms_events": round(mid["copy_ms"], 2), "kernel_ms_events": round(mid["kernel_ms"], 2),
    "copy_share_of_wall": round(mid["copy_ms"] / (1e3 * mid["wall_s"]), 3),
    "kernel_share_of_wall": round(mid["kernel_ms"] / (1e3 * mid["wall_s"]), 3),
    "staged_bytes": mid["staged_bytes"], "chunk_cols": mid["chunk_cols"],
    "max_abs_diff_vs_host": None if host is None else float(np.nanmax(np.abs(dev - host))),
}), flush=True)
