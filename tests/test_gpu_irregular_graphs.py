"""The device kernels on irregular graphs (needs an MI355X): a hub column of B
of H entries in an otherwise uniform graph, a chain (sorted 1-D ordering: a
DAG of n levels of one row each) and a regular grid (exact distance ties).
Every other GPU module builds its problems with conftest.make_problem
(uniform points, max-min ordered: longest column a small multiple of m + 1,
shallow DAG, a few neighbour tiles per tile); the code branches on exactly
these quantities -- the colour engine's lanes per chain and its chunk cap
(lanes x 16 entries), the tile batches' cap (NT x RMAX cells: 512 wave-local,
3584 exchange-wave, 4096 classic), the segmented scans over a slot's cells
across lanes, DPP rows and waves, the hand-off of a slot every other tile
reads, the remote-reader mask of a tile shard.  tests/test_capi_and_graph.py
(test_*_hub_column, test_*_refuses_*) runs the same graphs through the CPU
emulations of the layouts: the first place to look when a case here fails.

Bars, all from tests/test_gpu_parity.py (its module docstring and the tests
named), none widened for these graphs:
  sweep field after two calls (3 + 2 sweeps) ... rtol 1e-8, atol 1e-9
      (test_sweep_matches_masked_reference_form), on the device's own factor
  Vecchia factor vs O.vecchia_linv ............. rtol 1e-9, atol 1e-10
      (test_factor_matches_oracle)
  log-likelihood ............................... rel 1e-10
      (test_loglik_matches_oracle), on the device's own factor
  triangular solve, ancillary proposal ......... rtol 1e-9, atol 1e-10
      (test_mh_building_blocks)
  beta_0 statistics (1'B'B1, 1'B'Bf) ........... rtol 1e-10
      (test_beta0_stats_reuses_loglik_pass_and_invalidates)
  batched vs single chain, r global vs LDS, the ranks of
  a shard vs one rank, the solve plans among each other ... bitwise.
The hub location itself is held to the sweep bar like every other location:
it stays at 5e-7 of it or less, so the summation bound H 2^-53 sum|terms| of
its conditional mean was not needed.

Each case prints one line "[irregular] <case>: engine, lanes, max_collen,
note" and its measured maxima as fractions of the bars (pytest -s).
Measured maxima on the MI355X over every case of this file, as fractions of
the bars: sweep 3.9e-6 (hub location 5.1e-7), factor 0.56 (Matern 3/2, range
0.05, on the n = 4000, m = 10 hub graph: |Linv| up to 1.6e3; 0.17 at n = 3000,
m = 5; exponential 7e-4), log-likelihood 6.3e-3, triangular solve 1.2e-4,
ancillary proposal 1.3e-4, beta_0 statistics 1.5e-3; every bitwise comparison
exact; no rescue of the sync-free solve on the 3000-level chain.  The bars
stay as test_gpu_parity.py states them.
"""
import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

HUB = 7
# covariance per chain (the builders give finite factors for the first two;
# the third is the first with another variance)
COVS = [("exponential_isotropic", [1.0, 0.1, 0.0]), ("matern15_isotropic", [1.0, 0.05, 0.0]),
        ("exponential_isotropic", [1.3, 0.1, 0.0])]
# per-chain scalars of the two sweep calls (3 + 2 sweeps, Philox normals)
B0 = [0.3, -0.2, 0.5]
CALLS = [(3, [0.1, -0.2, 0.3], [-0.4, -0.1, -0.8], [31, 32, 33], [0, 5, 9]),
         (2, [0.0, 0.2, -0.1], [-0.5, -0.3, -0.6], [41, 42, 43], [3, 3, 3])]
SWEEP_ENV = ["NNGP_ENGINE", "NNGP_TILES", "NNGP_TILE_XW", "NNGP_TILE_WL", "NNGP_TILE_R", "NNGP_TILE_NT",
             "NNGP_TILE_CHAINS", "NNGP_TILE_BATCH_CELLS", "NNGP_TILE_SPLIT", "NNGP_COLOUR_LANES", "NNGP_TRI"]

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _collen(NN, n):
    return np.bincount(NN[NN > 0] - 1, minlength=n)


# ---------------------------------------------------------------- graph builders
def hub_problem(P, n, m, H, seed, hub=HUB):
    """make_problem(P, n, m, seed) with the last neighbour of random rows
    k > max(hub, m) rewired to location `hub`, so that its column of B has
    exactly H entries (its own row counted, as capi.hip max_column_length
    counts it); recoloured."""
    def make():
        locs, NN, col, lm, y = make_problem(P, n, m, seed=seed)
        NN = NN.copy()
        rng = np.random.default_rng(seed + 1000)
        has = (NN == hub + 1).any(axis=1)
        cand = np.nonzero(~has & (np.arange(n) > max(hub, m)))[0]
        rows = rng.choice(cand, H - int(has.sum()), replace=False)
        NN[rows, m] = hub + 1
        col = P.naive_greedy_coloring(NN)
        cl = _collen(NN, n)
        assert cl[hub] == H == cl.max() and np.sort(cl)[-2] < 100, (cl[hub], np.sort(cl)[-2])
        assert len(np.unique(col)) == col.max()  # every colour class non-empty
        return locs, NN, col, lm, y
    return _cached(("hub", n, m, H, seed, hub), make)


def chain_problem(P, n, m, h):
    """Locations (k h, 0) in index order (no reordering): row k of the NNarray
    is k, k-1, ..., k-m -- a DAG of n levels, m + 1 colours, every column of
    length m + 1.  h = range / 5 of the covariance used."""
    def make():
        locs = np.column_stack([np.arange(n) * h, np.zeros(n)])
        NN = P.find_ordered_nn(locs, m)
        k = np.arange(n)[:, None] + 1 - np.arange(m + 1)[None, :]
        assert np.array_equal(NN[m:], k[m:]) and np.array_equal(NN[:m][k[:m] > 0], k[:m][k[:m] > 0])
        col = P.naive_greedy_coloring(NN)
        assert col.max() == m + 1 and _collen(NN, n).max() == m + 1
        lm = np.arange(1, n + 1, dtype=np.int32)
        y = np.random.default_rng(n + m).normal(size=n)
        return locs, NN, col, lm, y
    return _cached(("chain", n, m, h), make)


def grid_problem(P, g, m):
    """A g x g regular grid on the unit square, max-min ordered: exact
    distance ties in the neighbour search and in the Morton / Hilbert keys."""
    def make():
        x = np.arange(g) / (g - 1)
        locs = np.array([(a, b) for a in x for b in x])
        locs = locs[P.order_maxmin(locs) - 1]
        NN = P.find_ordered_nn(locs, m)
        col = P.naive_greedy_coloring(NN)
        n = g * g
        return locs, NN, col, np.arange(1, n + 1, dtype=np.int32), np.random.default_rng(g).normal(size=n)
    return _cached(("grid", g, m), make)


# ---------------------------------------------------------------- checks
def _set_env(monkeypatch, **env):
    for k in SWEEP_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _frac(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): <= 1 is numpy's assert_allclose"""
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def _fields0(prob, C):
    n = prob[0].shape[0]
    rng = np.random.default_rng(17)
    return [rng.normal(size=n) + B0[k] for k in range(C)]


def _setup(ctx, prob, C, fields, covs=COVS):
    for k in range(C):
        ctx.select(k)
        ctx.factor(0, *covs[k])
        ctx.set_field(fields[k])
        ctx.set_mu(None, B0[k])
    ctx.select(0)


def _two_calls(ctx, C):
    for ns, ls, lnv, seeds, bases in CALLS:
        ctx.sweep_chains(ns, B0[:C], ls[:C], lnv[:C], seeds[:C], bases[:C])


def _get_fields(ctx, C):
    out = [ctx.select(k).get_field() for k in range(C)]
    ctx.select(0)
    return out


def _oracle_two_calls(O, key, prob, k, L, field):
    """The oracle's local-form sweeps of chain k's two calls on the factor L
    (the device's own), shared by every test that needs them."""
    locs, NN, col, lm, y = prob
    n = len(locs)

    def make():
        D = O.precision_diag(L, NN)
        f = field
        for ns, ls, lnv, seeds, bases in CALLS:
            z = O.sweep_normals(seeds[k], bases[k], ns, n)
            f = O.sweep("local", f, L, NN, col, D, np.ones(n, np.int32), y, np.full(n, B0[k]), lm, B0[k], ls[k],
                        lnv[k], z)
        return f
    return _cached(("sweep", key, k, L.tobytes()), make)


def _report(label, info, figs):
    print(f"\n[irregular] {label}: sweep_engine={info['sweep_engine']} lanes_per_chain={info['lanes_per_chain']} "
          f"max_collen={info['max_collen']} n_colors={info['n_colors']} n_tiles={info['n_tiles']} "
          f"tile_exchange_wave={info['tile_exchange_wave']} note='{info['engine_note']}'")
    if figs:
        print(f"[irregular] {label}: fractions of the bars: " + " ".join(f"{k}={v:.3g}" for k, v in figs.items()))


def _check_context(P, O, label, key, prob, C, expect=None, batched_vs_single=False, ctx_type=None, covs=COVS):
    """Two sweep calls on a C-chain context against the oracle on the device's
    own factors, every chain; the factors, log-likelihood, triangular solve
    and beta_0 statistics against the oracle on the same context.  expect(info)
    asserts the path the context took.  -> the chains' fields."""
    locs, NN, col, lm, y = prob
    n = len(locs)
    fields = _fields0(prob, C)
    figs = {"sweep": 0.0, "sweep_hub": 0.0, "factor": 0.0, "loglik": 0.0, "solve": 0.0, "beta0": 0.0}
    open_ctx = ctx_type or (lambda: P.ChainContext(locs, NN, col, lm, y, device=0, n_chains=C))
    u = np.random.default_rng(5).normal(size=n)
    with open_ctx() as ctx:
        info = ctx.info
        if expect:
            expect(info)
        _setup(ctx, prob, C, fields, covs)
        Ls = [ctx.select(k).get_linv(0) for k in range(C)]
        ctx.select(0)
        _two_calls(ctx, C)
        got = _get_fields(ctx, C)
        for k in range(C):
            ctx.select(k)
            ll = ctx.loglik(0, B0[k], 0.2)
            llo = O.loglik(Ls[k], got[k] - B0[k], NN, 0.2)
            figs["loglik"] = max(figs["loglik"], abs(ll - llo) / (1e-10 * abs(llo)))
            st = ctx.beta0_stats()
            B1, Bf = O.linv_mult(Ls[k], np.ones(n), NN), O.linv_mult(Ls[k], got[k], NN)
            figs["beta0"] = max(figs["beta0"], _frac(np.array(st), np.array([B1 @ B1, B1 @ Bf]), 1e-10, 0.0))
            x = ctx.tri_solve(0, u)
            assert np.all(np.isfinite(x))
            figs["solve"] = max(figs["solve"], _frac(x, O.tri_solve(Ls[k], NN, u), 1e-9, 1e-10))
        ctx.select(0)
    for k in range(C):
        Lo = _cached(("linv", key, k), lambda: O.vecchia_linv(*covs[k], locs, NN))
        assert np.all(np.isfinite(Lo))
        figs["factor"] = max(figs["factor"], _frac(Ls[k], Lo, 1e-9, 1e-10))
        assert np.all(Ls[k][NN == O.NA] == 0.0)
        ref = _oracle_two_calls(O, key, prob, k, Ls[k], fields[k])
        figs["sweep"] = max(figs["sweep"], _frac(got[k], ref, 1e-8, 1e-9))
        figs["sweep_hub"] = max(figs["sweep_hub"], _frac(got[k][HUB:HUB + 1], ref[HUB:HUB + 1], 1e-8, 1e-9))
    _report(label, info, figs)
    for k in range(C):
        np.testing.assert_allclose(Ls[k], _cache[("linv", key, k)], rtol=1e-9, atol=1e-10, err_msg=f"factor, chain {k}")
        np.testing.assert_allclose(got[k], _oracle_two_calls(O, key, prob, k, Ls[k], fields[k]), rtol=1e-8, atol=1e-9,
                                   err_msg=f"sweep, chain {k}")
    assert figs["loglik"] <= 1.0 and figs["solve"] <= 1.0 and figs["beta0"] <= 1.0, figs
    if batched_vs_single:
        # the same context layout, chains swept one at a time: bitwise identical
        with open_ctx() as seq:
            _setup(seq, prob, C, fields, covs)
            for k in range(C):
                for ns, ls, lnv, seeds, bases in CALLS:
                    seq.select(k).sweep(ns, B0[k], ls[k], lnv[k], seeds[k], bases[k])
            for k, f in enumerate(_get_fields(seq, C)):
                np.testing.assert_array_equal(got[k], f, err_msg=f"batched vs alone, chain {k}")
    return got


# ---------------------------------------------------------------- hub column
def test_hub_column_under_every_engine(P, O, engine):
    """H = 300 at 3 chains under the four engines of the suite (colours on 21
    lanes; 24 wave-local tiles; the default tile count, with and without the
    exchange wave): two calls, every chain against the oracle."""
    prob = hub_problem(P, 3000, 5, 300, seed=1)

    def expect(info):
        assert info["max_collen"] == 300, info
        if info["sweep_engine"] == 0:
            assert info["lanes_per_chain"] == 21, info
    _check_context(P, O, f"hub H=300 C=3 [{engine}]", "hub300", prob, 3, expect)


def _colours(lanes, H):
    def expect(info):
        assert info["sweep_engine"] == 0 and info["lanes_per_chain"] == lanes and info["max_collen"] == H, info
    return expect


def _tiles(H, xw, wave_local, T=24):
    def expect(info):
        assert info["sweep_engine"] == 1 and info["n_tiles"] == T and info["max_collen"] == H, info
        assert info["tile_exchange_wave"] == xw and info["tile_r_global"] == 0, info
        assert ("wave-local" in info["engine_note"]) == wave_local, info["engine_note"]
    return expect


# The tile cases fix NNGP_TILES=24: the default tile count (n / 2048: 2 to 4
# tiles at these sizes) would run them on tiles too, but with a hub that only
# 1 to 3 other tiles read; with 24 tiles it is a foreign slot of 23.
HUB_CASES = {
    # (a) colours, 3 chains, no override: 21 lanes chosen for the column of 300 (> 256)
    "a-colours-3chains-H300": ((3000, 5, 300, 1), "hub300", 3, {"NNGP_ENGINE": "colors"}, _colours(21, 300), True),
    # (b) one slot fills nearly a whole chunk: 500 of 512 at 2 chains, 1000 of 1024 at 1 chain
    "b-colours-2chains-H500": ((4000, 10, 500, 2), "hub500", 2, {"NNGP_ENGINE": "colors"}, _colours(32, 500), False),
    "b-colours-1chain-H1000": ((6000, 5, 1000, 3), "hub1000", 1, {"NNGP_ENGINE": "colors"}, _colours(64, 1000), False),
    # (c) tiles, 3 chains, wave-local batches (default): one slot fills a 64-lane batch (500 of 512 cells)
    "c-tiles-3chains-wave-local-H500": ((4000, 10, 500, 2), "hub500", 3, {"NNGP_TILES": "24"},
                                        _tiles(500, 1, True), True),
    # (d) tiles, 1 chain: the slot covers several whole waves (3000 of 3584 / 4096 cells)
    "d-tiles-1chain-exchange-wave-H3000": ((8000, 5, 3000, 4), "hub3000", 1, {"NNGP_TILES": "24"},
                                           _tiles(3000, 1, False), False),
    "d-tiles-1chain-classic-H3000": ((8000, 5, 3000, 4), "hub3000", 1, {"NNGP_TILES": "24", "NNGP_TILE_XW": "0"},
                                     _tiles(3000, 0, False), False),
}


@pytest.mark.parametrize("case", list(HUB_CASES))
def test_hub_column_required_paths(P, O, engine, monkeypatch, case):
    """Cases (a) to (d), and (f) for (a) and (c): each asserts through
    ctx.info that the intended engine, lanes per chain and batch kind ran with
    the hub's max_collen, then two calls (3 + 2 sweeps, other scalars per
    chain, the second call warm where the engine has a warm path) against the
    oracle; (f): every chain of sweep_chains bitwise equal to the same
    context's chain swept alone."""
    if engine != "tiles-default":
        pytest.skip("sets the engine itself")
    args, key, C, env, expect, single = HUB_CASES[case]
    _set_env(monkeypatch, **env)
    prob = hub_problem(P, *args)
    _check_context(P, O, case, key, prob, C, expect, batched_vs_single=single)


def _bitwise_pair(P, monkeypatch, prob, C, envs, expects, label):
    fields = _fields0(prob, C)
    out = []
    for env, expect in zip(envs, expects):
        _set_env(monkeypatch, **env)
        with P.ChainContext(*prob, device=0, n_chains=C) as ctx:
            info = ctx.info
            expect(info)
            _report(label, info, {})
            _setup(ctx, prob, C, fields)
            _two_calls(ctx, C)
            out.append(_get_fields(ctx, C))
    for k in range(C):
        np.testing.assert_array_equal(out[1][k], out[0][k], err_msg=f"chain {k}")
    return out[0]


def test_hub_column_r_global_equals_lds_bitwise(P, O, engine, monkeypatch):
    """(e) tiles, 1 chain, H = 1000: r in global memory (NNGP_TILE_R=global)
    == r in LDS on the same 512-thread cell layout, bitwise, after two calls
    (as test_tile_engine_r_in_global_memory_equals_lds_bitwise on uniform
    graphs); the LDS side matches the oracle."""
    if engine != "tiles-default":
        pytest.skip("sets the engine itself")
    prob = hub_problem(P, 6000, 5, 1000, 3)
    base = {"NNGP_TILES": "24", "NNGP_TILE_XW": "0"}

    def exp(rg):
        def expect(info):
            assert info["sweep_engine"] == 1 and info["tile_r_global"] == rg and info["max_collen"] == 1000, info
        return expect
    _bitwise_pair(P, monkeypatch, prob, 1, [base, dict(base, NNGP_TILE_R="global")], [exp(0), exp(1)],
                  "e-tiles-1chain-r-global-H1000")
    _set_env(monkeypatch, **base)
    _check_context(P, O, "e-tiles-1chain-r-lds-H1000", "hub1000", prob, 1, exp(0))


def test_hub_column_256_thread_tiles_match_oracle(P, O, engine, monkeypatch):
    """(e) tiles, 2 chains, H = 1000: 256-thread tiles cut into 2048-cell
    batches (as test_tile_engine_chain_split_equals_joint_bitwise on uniform
    graphs) match the oracle."""
    if engine != "tiles-default":
        pytest.skip("sets the engine itself")
    prob = hub_problem(P, 6000, 5, 1000, 3)
    env = {"NNGP_TILES": "24", "NNGP_TILE_NT": "256", "NNGP_TILE_BATCH_CELLS": "2048", "NNGP_TILE_CHAINS": "joint"}

    def expect(info):
        assert info["sweep_engine"] == 1 and info["tile_chain_split"] == 0, info["engine_note"]
        assert info["max_collen"] == 1000, info
    _set_env(monkeypatch, **env)
    _check_context(P, O, "e-tiles-2chains-joint-H1000", "hub1000", prob, 2, expect)


# ---------------------------------------------------------------- refusals
def _max_collen(H):
    def expect(info):
        assert info["max_collen"] == H, info
    return expect


def _uniform_context_still_sweeps(P, O):
    """After a refusal: a normal context on a uniform problem in the same
    process is created and sweeps correctly (nothing left counted or locked)."""
    prob = _cached(("uniform", 2000, 5), lambda: make_problem(P, 2000, 5, seed=12))
    _check_context(P, O, "uniform after a refusal", "uniform2000", prob, 1)


@pytest.mark.parametrize("n,m,H,seed,C,advice", [(12000, 5, 4200, 5, 1, False), (3000, 5, 600, 6, 3, True)])
def test_column_beyond_the_limits_is_refused(P, O, engine, n, m, H, seed, C, advice):
    """H = 4200 at 1 chain is beyond every limit (1024 colour entries, 3584 /
    4096 tile cells); H = 600 at 3 chains is beyond the 512 wave-local cells
    and the 336 colour entries.  The context is refused with NNGP_ERR_ARG and
    a message naming the column -- for the second the "fewer chains" advice --
    or, where a fallback reaches a layout that fits (the classic tiles' 4096
    cells take H = 600), it comes up and matches the oracle.  No sweep is
    launched by a refusal, and a uniform context created afterwards works."""
    prob = hub_problem(P, n, m, H, seed)
    try:
        ctx = P.ChainContext(*prob, device=0, n_chains=C)
    except P.NNGPError as e:
        print(f"\n[irregular] refusal H={H} C={C} [{engine}]: {e}")
        assert e.status == 1, e
        assert "column of B" in str(e) or str(H) in str(e), e
        if advice:
            assert "fewer chains" in str(e), e
    else:
        ctx.close()
        assert H <= 4096, "no layout of any engine holds this column"
        _check_context(P, O, f"not refused: H={H} C={C} [{engine}]", f"hub{H}", prob, C, _max_collen(H))
    _uniform_context_still_sweeps(P, O)


# ---------------------------------------------------------------- chain graph
CHAIN_COV = {"exponential_isotropic": 0.1, "matern15_isotropic": 0.05}  # covfun -> range (h = range / 5)
# per chain on the line of spacing h = 0.01: range 0.05 = 5 h for every chain
CHAIN_COVS = [("exponential_isotropic", [1.0, 0.05, 0.0]), ("matern15_isotropic", [1.0, 0.05, 0.0]),
              ("exponential_isotropic", [1.3, 0.05, 0.0])]


@pytest.mark.parametrize("m", [5, 15])
def test_chain_graph_sweeps_match_oracle(P, O, engine, m):
    """n = 3000 locations on a line in index order, m + 1 colours: two sweep
    calls at 3 chains (the factors, log-likelihood, the default solve and the
    beta_0 statistics with them) under all four engines."""
    prob = chain_problem(P, 3000, m, 0.01)

    def expect(info):
        assert info["n_colors"] == m + 1 and info["n_levels"] == 3000 and info["max_collen"] == m + 1, info
    _check_context(P, O, f"chain m={m} C=3 [{engine}]", f"chain{m}", prob, 3, expect, covs=CHAIN_COVS)


@pytest.mark.parametrize("covfun", list(CHAIN_COV))
@pytest.mark.parametrize("m", [5, 15])
def test_chain_graph_solve_plans_bitwise_and_match_oracle(P, O, engine, monkeypatch, m, covfun):
    """A DAG of 3000 levels of one row each: the sync-free solve (`dag`), the
    blocked plan (`levels`) and one launch per level (`level`) give the same
    bits, repeatedly, finish (a timed-out wait is an error status and leaves
    NaN: neither) and match the oracle's solve."""
    if engine != "tiles-default":
        pytest.skip("engine independent")
    n = 3000
    cp = [1.0, CHAIN_COV[covfun], 0.0]
    locs, NN, col, lm, y = prob = chain_problem(P, n, m, CHAIN_COV[covfun] / 5)
    rng = np.random.default_rng(m)
    us = [rng.normal(size=n) for _ in range(2)]
    got = {}
    for plan in ("dag", "levels", "level"):
        _set_env(monkeypatch, NNGP_TRI=plan)
        with P.ChainContext(*prob, device=0) as ctx:
            assert ctx.info["n_levels"] == n
            ctx.factor(0, covfun, cp)
            got[plan] = [ctx.tri_solve(0, u) for u in us]
            L = ctx.get_linv(0)
            rescues = ctx.tri_rescues()
        assert all(np.all(np.isfinite(x)) for x in got[plan])
        print(f"\n[irregular] chain m={m} {covfun} NNGP_TRI={plan}: rescues={rescues} "
              f"solve={_frac(got[plan][0], O.tri_solve(L, NN, us[0]), 1e-9, 1e-10):.3g} of the bar")
    for plan in ("levels", "level"):
        for a, b in zip(got["dag"], got[plan]):
            np.testing.assert_array_equal(a, b, err_msg=plan)
    np.testing.assert_allclose(L, O.vecchia_linv(covfun, cp, locs, NN), rtol=1e-9, atol=1e-10)
    for x, u in zip(got["dag"], us):
        np.testing.assert_allclose(x, O.tri_solve(L, NN, u), rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("m", [5, 15])
def test_chain_graph_ancillary_propose_matches_oracle(P, O, engine, m, C):
    """beta0 + exp(dls/2) B1^{-1} B0 (field - beta0) (update_Gaussian.R:127)
    on the chain graph, every chain of a 1- and a 3-chain context (the batched
    proposal runs one solve schedule for all chains)."""
    if engine != "tiles-default":
        pytest.skip("engine independent")
    n = 3000
    locs, NN, col, lm, y = prob = chain_problem(P, n, m, 0.01)
    fields = _fields0(prob, C)
    c1s = [(cf, [cp[0] * 1.2, cp[1] * 1.1, 0.0]) for cf, cp in CHAIN_COVS]
    dls = [0.2, -0.1, 0.3]
    with P.ChainContext(*prob, device=0, n_chains=C) as ctx:
        _setup(ctx, prob, C, fields, CHAIN_COVS)
        for k in range(C):
            ctx.select(k).factor(1, *c1s[k])
        if C == 1:
            ctx.select(0).ancillary_propose(B0[0], dls[0])
        else:
            ctx.ancillary_propose_chains((1 << C) - 1, B0[:C], dls[:C])
        worst = 0.0
        for k in range(C):
            ctx.select(k)
            L0, L1 = ctx.get_linv(0), ctx.get_linv(1)
            ctx.accept_field()
            got = ctx.get_field()
            w = O.tri_solve(L1, NN, O.linv_mult(L0, fields[k] - B0[k], NN))
            ref = B0[k] + np.exp(0.5 * dls[k]) * w
            worst = max(worst, _frac(got, ref, 1e-9, 1e-10))
            np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-10, err_msg=f"chain {k}")
    print(f"\n[irregular] chain m={m} ancillary C={C}: {worst:.3g} of the bar")


# ---------------------------------------------------------------- grid
def test_grid_graph_prep_bit_exact(P, O):
    locs, NN, col, lm, y = grid_problem(P, 64, 10)
    x = np.arange(64) / 63
    raw = np.array([(a, b) for a in x for b in x])
    np.testing.assert_array_equal(P.order_maxmin(raw), O.order_maxmin_exact(raw))
    np.testing.assert_array_equal(NN, O.find_ordered_nn(locs, 10))
    np.testing.assert_array_equal(col, O.greedy_coloring(NN))
    print(f"\n[irregular] grid 64x64 m=10: colours={col.max()} longest column={_collen(NN, len(locs)).max()}")


@pytest.mark.parametrize("C", [1, 3])
def test_grid_matches_oracle(P, O, engine, C):
    """g = 64, m = 10 (distance ties everywhere): factor, log-likelihood and
    two sweep calls against the oracle at 1 and 3 chains, all four engines."""
    prob = grid_problem(P, 64, 10)
    _check_context(P, O, f"grid C={C} [{engine}]", "grid64", prob, C)


# ---------------------------------------------------------------- group shard on one device
@pytest.mark.parametrize("shard_engine", ["tiles", "colors"])
def test_hub_column_group_shard(P, O, engine, monkeypatch, shard_engine):
    """Hub graph (n = 6000, m = 5, H = 1000) as a G = 4 shard on one device
    (the _shards / sweep_chains_group pattern of test_gpu_shard.py), tile and
    colour shard: the hub's draw goes to every other rank (tile shard: its
    remote-reader mask has every rank set).  Every rank bitwise equal to the
    1-rank shard after two calls; the 1-rank shard matches the oracle."""
    if engine != "tiles-default":
        pytest.skip("sets the engine itself")
    _set_env(monkeypatch, NNGP_ENGINE=shard_engine, NNGP_TILES="24")
    G = 4
    locs, NN, col, lm, y = prob = hub_problem(P, 6000, 5, 1000, 3)
    fields = _fields0(prob, 1)

    def expect(info):
        assert info["sweep_engine"] == (1 if shard_engine == "tiles" else 0) and info["max_collen"] == 1000, info

    want = _check_context(P, O, f"shard of 1 rank [{shard_engine}]", "hub1000", prob, 1, expect,
                          ctx_type=lambda: P.ShardContext(*prob, n_ranks=1, rank=0, device=0))
    ctxs = [P.ShardContext(*prob, n_ranks=G, rank=g, device=0) for g in range(G)]
    try:
        info = ctxs[0].info
        expect(info)
        assert info["n_ranks"] == G and sum(c.info["shard_owned"] for c in ctxs) == len(locs)
        assert info["shard_exchange_slots"] > 0
        _report(f"shard of {G} ranks [{shard_engine}]", info, {})
        for c in ctxs:
            _setup(c, prob, 1, fields)
        for ns, ls, lnv, seeds, bases in CALLS:
            P.sweep_chains_group(ctxs, ns, B0[:1], ls[:1], lnv[:1], seeds[:1], bases[:1])
        for g, c in enumerate(ctxs):
            np.testing.assert_array_equal(c.get_field(), want[0], err_msg=f"rank {g}")
    finally:
        for c in ctxs:
            c.close()
