"""get_summary at the headline shape, host against device: three chains'
blocks of ROWS x N seeded normals (default 100 x 1e6: 2.4 GB) with one offset
per row.  The host path (stack, centre, numpy) is timed once; the device path
(nngp_summary: blocks passed where they lie) as the median of five runs after
one warm run, with the HIP-event times of its staging copies and kernels.
Prints one JSON line.  argv: [N [ROWS [CHUNK_COLS]]] [nohost] (nohost skips
the host path); NNGP_SUMMARY_BITS picks the digit width of the radix select
(2 or 4).

--probs P1,P2,... and / or --thresholds T1,T2,... (either may be "default" /
"none": the three default probabilities / no threshold) time nngp_summary_probs
beside it: after one warm call of each, --runs (default 5) rounds alternate
the plain call and the widened one in this one process, and the line carries,
for both, every run's wall time, copy_ms and kernel_ms with their medians and
ranges, and whether the widened result's shared columns are bitwise the plain
call's."""
import argparse
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


def _floats(s, default):
    if s is None:
        return None
    if s in ("default", "none", ""):
        return default
    return tuple(float(v) for v in s.split(","))


ap = argparse.ArgumentParser()
ap.add_argument("pos", nargs="*")
ap.add_argument("--probs")
ap.add_argument("--thresholds")
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()
P = _pkgload.load()
argv = [a for a in args.pos if a != "nohost"]
with_host = "nohost" not in args.pos
n = int(float(argv[0])) if len(argv) > 0 else 1_000_000
rows = int(argv[1]) if len(argv) > 1 else 100
chunk_cols = int(argv[2]) if len(argv) > 2 else 0
probs, thresholds = _floats(args.probs, (0.025, 0.5, 0.975)), _floats(args.thresholds, ())
widened = probs is not None or thresholds is not None
rng = np.random.default_rng(8)
blocks = [0.3 * k + rng.standard_normal((rows, n)) for k in range(3)]
off = 0.1 * rng.standard_normal(3 * rows)

host, host_s = None, None
if with_host:
    t = time.perf_counter()
    host = P.get_summary(blocks, row_offset=off)
    host_s = time.perf_counter() - t


def timed(**kw):
    t = time.perf_counter()
    res = P.get_summary(blocks, backend="hip", device=0, row_offset=off, chunk_cols=chunk_cols, **kw)
    wall = time.perf_counter() - t
    return res, dict(P.estimate.summary_stats(), wall_s=wall)


def spread(runs, key, scale=1.0, digits=2):
    v = [scale * r[key] for r in runs]
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "runs": [round(u, digits) for u in v]}


wide_kw = {"probs": probs, "thresholds": thresholds}
dev, _ = timed()  # warm
if widened:
    wide, _ = timed(**wide_kw)
runs, wide_runs = [], []
for _ in range(args.runs):
    dev, st = timed()
    runs.append(st)
    if widened:
        wide, st = timed(**wide_kw)
        wide_runs.append(st)
wall_s = statistics.median(r["wall_s"] for r in runs)
mid = min(runs, key=lambda r: abs(r["wall_s"] - wall_s))
line = {
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
}
if widened:
    q = 3 if probs is None else len(probs)
    line["alternating"] = {
        "runs_each": args.runs,
        "nngp_summary": {"wall_ms": spread(runs, "wall_s", 1e3), "copy_ms": spread(runs, "copy_ms"),
                         "kernel_ms": spread(runs, "kernel_ms")},
        "nngp_summary_probs": {"probs": list(probs if probs is not None else (0.025, 0.5, 0.975)),
                               "thresholds": list(thresholds or ()),
                               "wall_ms": spread(wide_runs, "wall_s", 1e3), "copy_ms": spread(wide_runs, "copy_ms"),
                               "kernel_ms": spread(wide_runs, "kernel_ms")},
        "mean_and_sd_bitwise_equal": bool(np.array_equal(wide[:, [0, 1 + q]], dev[:, [0, 4]], equal_nan=True)),
    }
    if tuple(line["alternating"]["nngp_summary_probs"]["probs"]) == (0.025, 0.5, 0.975):
        line["alternating"]["default_columns_bitwise_equal"] = bool(np.array_equal(wide[:, :5], dev, equal_nan=True))
print(json.dumps(line), flush=True)
