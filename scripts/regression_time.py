"""Full MCMC iterations/s with covariates, regression="host" against
regression="device", in one process: N locations (default 1e6, m = 15,
exponential), 3 chains in one context, a synthetic centred design of p = 10
columns of which 2 are X_locs (interweaved), n_chromatic = 10,
field_thinning = 1 -- the shape of bench.py's secondary metric plus the
regression block (update_Gaussian.R:77-83,145-151,226-250).

Each mode: a warm-up call, then REPEATS timed update calls (median reported,
all listed).  Host syncs and bytes copied per iteration are counted from the
calls the driver makes, each call charged what capi.hip does for it (e.g.
get_field: one sync and n doubles to the host; spmv: per column one sync and n
doubles each way; design_commit_chains: no sync, the coefficients to the
device).  Prints one JSON line.
argv: [N [ITERS_HOST [ITERS_DEVICE [REPEATS]]]]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _pkgload  # noqa: E402

P = _pkgload.load()
from nngp_amd.context import ChainContext  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
iters = {"host": int(sys.argv[2]) if len(sys.argv) > 2 else 10, "device": int(sys.argv[3]) if len(sys.argv) > 3 else 30}
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
m, C, p, p_locs, covfun, cp = 15, 3, 10, 2, "exponential_isotropic", [1.0, 0.05, 0.0]


def note(msg):
    print(f"# {msg}", file=sys.stderr, flush=True)


rng = np.random.default_rng(5)
t = time.perf_counter()
locs = rng.uniform(size=(n, 2))
locs = locs[P.order_maxmin(locs) - 1]
NN = P.find_ordered_nn(locs, m)
col = P.naive_greedy_coloring(NN)
note(f"graph {time.perf_counter() - t:.1f} s")
lm = np.arange(1, n + 1, dtype=np.int32)
Xm = rng.normal(size=(n, p))
Xm -= Xm.mean(0)
beta_true = rng.normal(size=p) * 0.3
with P.ChainContext(locs, NN, col, lm, np.zeros(n), device=0) as c0:
    c0.factor(0, covfun, cp)
    w = c0.tri_solve(0, rng.normal(size=n))
y = 1.0 + Xm @ beta_true + w + 0.5 * rng.normal(size=n)
X1 = np.column_stack([np.ones(n), Xm])
X = {"X": Xm, "locs": np.arange(p_locs), "solve_1XT1X": np.linalg.inv(X1.T @ X1)}
X["chol_solve_1XT1X"] = np.linalg.cholesky(X["solve_1XT1X"]).T
del X1
va = {"NNarray": NN, "coloring": col, "locs_match": lm, "n_obs": n, "n_locs": n, "hctam_scol_1": lm}
stm = {"response_model": "Gaussian", "covfun": {"stationary_covfun": covfun, "shape_params": ["log_range"]}}

# (host syncs, bytes to the device, bytes to the host) of one call
res_stride = max(p + 1, (p_locs + 1) + (p_locs + 1) * (p_locs + 2) // 2)
coef = 8 * C * (2 * p_locs + p)
COST = {
    "get_field": lambda a: (1, 0, 8 * n),
    "set_field": lambda a: (1, 8 * n, 0),
    "set_mu": lambda a: (0, 8 * n if a[0] is not None else 0, 0),
    "spmv": lambda a: (np.atleast_2d(np.asarray(a[1]).T).shape[0],) + (8 * n * np.atleast_2d(np.asarray(a[1]).T).shape[0],) * 2,
    "beta0_stats": lambda a: (1, 0, 32),
    "ancillary_step_chains": lambda a: (1, 0, 8 * 4 * 8 + 16),
    "sufficient_step_chains": lambda a: (1, 0, 8 * 4 * 8 + 16),
    "sum_squared_residuals_chains": lambda a: (1, 0, 32 * C),
    "sweep_chains": lambda a: (0, 48 * C, 0),
    "record_field": lambda a: (0, 0, 8 * n),
    "design_mean_stats_chains": lambda a: (1, 0, 8 * C * res_stride),
    "design_interweave_stats_chains": lambda a: (1, coef, 8 * C * res_stride),
    "design_commit_chains": lambda a: (0, coef, 0),
}
tally = {"syncs": 0, "h2d": 0, "d2h": 0}
originals = {}
for name, cost in COST.items():
    originals[name] = getattr(ChainContext, name)

    def wrapped(self, *a, _f=originals[name], _c=cost, **kw):
        s, up, down = _c(a)
        tally["syncs"] += s
        tally["h2d"] += up
        tally["d2h"] += down
        return _f(self, *a, **kw)

    setattr(ChainContext, name, wrapped)


def measure(mode):
    srng = np.random.default_rng(11)
    states = {f"chain_{k + 1}": {
        "params": {"shape": np.array([np.log(cp[1]) + 0.05 * srng.normal()]), "beta_0": 1.0, "beta": np.zeros(p),
                   "log_scale": 0.0, "log_noise_variance": np.log(0.25), "field": 1.0 + w + 0.1 * srng.normal(size=n)},
        "transition_kernels": {"covariance_params_sufficient": {"logvar": -4.0},
                               "covariance_params_ancillary": {"logvar": -4.0},
                               "log_noise_variance": {"logvar": -1.0}}} for k in range(C)}
    ctx = P.ChainContext(locs, NN, col, lm, y, device=0, n_chains=C)
    views = [ctx.view(k) for k in range(C)]
    start = 0

    def run(it):
        nonlocal start
        out = P.mcmc_nngp_update_Gaussian(locs, X, y, stm, va, states, it, contexts=views,
                                          iterations=np.array([[start, 0.0]]), regression=mode)
        start += it
        for name, r in out.items():
            states[name] = r["state"]
        return out

    run(max(2, iters[mode] // 5))  # warm-up: code objects, graphs, allocator, the resident design
    times, acc = [], []
    for _ in range(repeats):
        for k in tally:
            tally[k] = 0
        t0 = time.perf_counter()
        out = run(iters[mode])  # ends with get_field: a host sync
        times.append(time.perf_counter() - t0)
        counts = {k: v / iters[mode] for k, v in tally.items()}
        acc.append(float(np.mean([np.mean(r["acceptance"]["covariance_acceptance_ancillary"]) +
                                  np.mean(r["acceptance"]["covariance_acceptance_sufficient"]) for r in out.values()])))
        del out
        note(f"{mode}: {iters[mode] / times[-1]:.2f} iterations/s")
    ctx.close()
    med = float(np.median(times))
    return {"iterations_per_s": round(iters[mode] / med, 2), "ms_per_iteration": round(med * 1e3 / iters[mode], 2),
            "iterations_per_s_all": [round(iters[mode] / x, 2) for x in times], "iterations": iters[mode],
            "host_syncs_per_iteration": round(counts["syncs"], 1),
            "mib_to_device_per_iteration": round(counts["h2d"] / 2 ** 20, 2),
            "mib_to_host_per_iteration": round(counts["d2h"] / 2 ** 20, 2),
            "accepted_proposals_per_chain_iteration": round(float(np.mean(acc)), 2)}


res = {mode: measure(mode) for mode in ("host", "device")}
print(json.dumps({"n": n, "m": m, "chains": C, "p": p, "p_locs": p_locs, "n_chromatic": 10, "field_thinning": 1.0,
                  "host": res["host"], "device": res["device"],
                  "speedup_device_vs_host": round(res["device"]["iterations_per_s"] / res["host"]["iterations_per_s"], 2)}),
      flush=True)
