"""mcmc_nngp_predict_field at the headline size, context engine against
batched engine, in one process: N observed locations (default 1e6, m = 10,
exponential), SAMPLES saved samples (default 300) of one chain with about a
third as many distinct shapes, and each N_PRED (default 1e4 and 1e5) uniform
new locations.  Both engines get the same injected normals; each is timed as
the whole call (nearest-neighbour search of the stacked locations included:
it is timed alone as well, `nn_s`), the batched engine also through
nngp_predict_stats (plan on the host, factor and solve by HIP events, staged
bytes, batch size).  Prints one JSON line per N_PRED.
argv: [N [SAMPLES [N_PRED ...]]] [nocontext] (nocontext skips the context
engine)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _pkgload  # noqa: E402

P = _pkgload.load()
argv = [a for a in sys.argv[1:] if a != "nocontext"]
with_context = "nocontext" not in sys.argv[1:]
n = int(float(argv[0])) if len(argv) > 0 else 1_000_000
n_samples = int(argv[1]) if len(argv) > 1 else 300
sizes = [int(float(a)) for a in argv[2:]] or [10_000, 100_000]
m = 10


def note(msg):
    print(f"# {msg}", file=sys.stderr, flush=True)


rng = np.random.default_rng(17)
locs = rng.uniform(size=(n, 2))
t = time.perf_counter()
locs = locs[P.order_maxmin(locs) - 1]
note(f"ordering {time.perf_counter() - t:.1f} s")
n_shapes = max(1, n_samples // 3)
log_range = np.log(0.02 + 0.03 * rng.uniform(size=n_shapes))
shape = log_range[np.arange(n_samples) * n_shapes // n_samples].reshape(-1, 1)
chain = {"saved_field": np.arange(1, n_samples + 1, dtype=np.float64),
         "params": {"shape": shape, "log_scale": 0.1 * rng.standard_normal((n_samples, 1)),
                    "beta_0": 1.0 + 0.1 * rng.standard_normal((n_samples, 1)),
                    "field": 1.0 + rng.standard_normal((n_samples, n))}}
L = {"locs": locs, "records": {"chain_1": chain},
     "space_time_model": {"covfun": {"stationary_covfun": "exponential_isotropic", "shape_params": ["log_range"]}}}
note("problem built")

for n_pred in sizes:
    pred = rng.uniform(size=(n_pred, 2))
    z = [rng.standard_normal((n_samples, n_pred))]
    t = time.perf_counter()
    P.find_ordered_nn(np.vstack([locs, pred]), m)
    nn_s = time.perf_counter() - t
    note(f"n_pred {n_pred}: nn search {nn_s:.1f} s")
    runs = []
    for rep in range(2):  # the first call warms the device (code objects, allocator)
        t = time.perf_counter()
        got = P.mcmc_nngp_predict_field(L, pred, burn_in=0.0, m=m, z_new=z, device=0, engine="batched")
        runs.append(dict(P.predict.predict_stats(), wall_s=time.perf_counter() - t))
        note(f"n_pred {n_pred}: batched call {rep}: {runs[-1]['wall_s']:.2f} s")
    ctx_s = diff = None
    if with_context:
        t = time.perf_counter()
        ref = P.mcmc_nngp_predict_field(L, pred, burn_in=0.0, m=m, z_new=z, device=0, engine="context")
        ctx_s = time.perf_counter() - t
        a, b = got["predicted_field_samples"][0], ref["predicted_field_samples"][0]
        diff = float(np.abs(a - b).max() / np.abs(b).max())
        note(f"n_pred {n_pred}: context call {ctx_s:.2f} s")
    r = runs[-1]
    print(json.dumps({
        "n": n, "m": m, "n_pred": n_pred, "n_samples": n_samples, "distinct_shapes": int(len(np.unique(shape))),
        "nn_search_s": round(nn_s, 3), "batched_wall_s": round(r["wall_s"], 3),
        "batched_wall_s_first_call": round(runs[0]["wall_s"], 3),
        "batched_wall_minus_nn_s": round(r["wall_s"] - nn_s, 3),
        "plan_ms": round(r["plan_ms"], 2), "factor_ms_events": round(r["factor_ms"], 2),
        "solve_ms_events": round(r["solve_ms"], 2), "staged_bytes": r["staged_bytes"],
        "sample_batch": r["sample_batch"],
        "context_wall_s": ctx_s and round(ctx_s, 3), "context_wall_minus_nn_s": ctx_s and round(ctx_s - nn_s, 3),
        "speedup_batched_vs_context": ctx_s and round(ctx_s / r["wall_s"], 2),
        "max_rel_diff_between_engines": diff,
    }), flush=True)
