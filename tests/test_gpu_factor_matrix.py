"""Every cell of the factor kernels' dispatch table against the long-double
reference (needs an MI355X), and the failing-row number of every kernel.

launch_factor / launch_factor_jobs (kernels.hip) choose BM in {8, 12, 16, 21,
run-time} by b = m + 1, FAM in {0, 1, 2} by the covariance, DS in {2, 3, 4} by
the coordinate dimension.  m in {7, 8, 11, 12, 15, 16, 20, 21, 31} puts b on
both sides of every template boundary (8|9, 12|13, 16|17, 21|22: the upper
side is a block padded in front), d in {1, 2, 3, 4} covers DS = 2 (twice), 3, 4.

Problem (highprec.dyadic_problem): distinct locations on the grid
(integers / 4096)^d, max-min ordered, m nearest earlier neighbours; every
range a power of two, so scaled coordinates and their differences are exact
and device and reference differ by their own arithmetic only.  n = 300; 64 in
the general-Matern cells, whose correlations come from mpmath.

Bounds: ctx.factor per row max(1e-10, 1e-14 cond(C_i)) max|row| against
highprec.vecchia_linv_hp, cond from the oracle's double covariance -- the
formula of test_gpu_parity._assert_rows_close;
Linv[NN == NA] == 0 exactly; precision_diag 1e-10 relative; factor_chains
bitwise equal to factor chain by chain (kernels.h).  Each case prints
"[matrix] ... worst err / (1e-14 cond max|row|)" per covariance (pytest -s);
the maxima per BM are recorded in DESIGN.md section 4 (0.03 to 0.05 on the
MI355X for every kernel, where the fp64 oracle itself reaches 0.045).  With
one real neighbour taken for padding in the BM = 12 blocks (gather_coords,
bs < BM) the default kernel's cells at b = 9 and, through their short leading
rows, b = 12 fail at every d, with the failing-row case at b = 9; nothing
else does.

The failing-row cases found the number to be the device's Morton row; the
kernels now report row_loc[row] (kernels.h), the caller's row.
"""
import re

import numpy as np
import pytest

import highprec as H

pytestmark = pytest.mark.gpu

MS = [7, 8, 11, 12, 15, 16, 20, 21, 31]
DS = [1, 2, 3, 4]
NUGGETS = [0.0, 0.1]
AXES = [0.25, 0.5, 0.125, 1.0]       # a different range per axis (scaledim)
AXES_M = [0.125, 0.25, 0.0625, 0.5]

_cache = {}


def _bm(b, fam=0):
    return "rt" if fam == 2 or b > 21 else next(B for B in (8, 12, 16, 21) if b <= B)


def _covs(d):
    """(covfun, covparms without the nugget) of the exponential and Matern 3/2
    cells at dimension d"""
    out = [("exponential_isotropic", [1.5, 0.25]), ("matern15_isotropic", [0.75, 0.0625])]
    if d >= 3:
        out += [("exponential_scaledim", [1.0] + AXES[:d]), ("exponential_spacetime", [2.0, 0.25, 0.5])]
    return out


def _covs_matern(m, d):
    out = []
    if m in (11, 31):
        out += [("matern_isotropic", [1.0, 0.0625, 1.0]), ("matern_isotropic", [1.25, 0.03125, 2.5])]
    if d >= 3:
        out += [("matern_scaledim", [1.0] + AXES_M[:d] + [2.5]), ("matern_spacetime", [1.0, 0.125, 0.25, 0.75])]
    return out


def _problem(P, n, m, d):
    key = ("prob", n, m, d)
    if key not in _cache:
        _cache[key] = H.dyadic_problem(P, n, m, d, seed=100 * d + n)  # the same points for every m
    return _cache[key]


def _reference(O, n, m, d, covfun, cp, prob):
    """(vecchia_linv_hp, cond per row), computed once per cell"""
    key = ("ref", n, m, d, covfun, tuple(cp))
    if key not in _cache:
        locs, NN = prob[0], prob[1]
        _cache[key] = (H.vecchia_linv_hp(covfun, cp, locs, NN), H.row_conds(O, covfun, cp, locs, NN))
    return _cache[key]


def _judge(O, ctx, n, m, d, covfun, cp, prob, label):
    NN = prob[1]
    ctx.factor(0, covfun, cp)
    got = ctx.get_linv(0)
    ref, kappa = _reference(O, n, m, d, covfun, cp, prob)
    err, tol, ratio = H.row_errors(got, ref, kappa)
    w = int(np.argmax(ratio))
    print(f"[matrix] {label} b={m + 1} BM={_bm(m + 1, H.FAMILY[covfun])} d={d} {covfun} nugget={cp[-1]}: worst err / "
          f"(1e-14 cond max|row|) = {ratio[w]:.3g} at row {w} (cond {kappa[w]:.3g}; largest cond {kappa.max():.3g})")
    bad = np.nonzero(~(err <= tol))[0]
    assert len(bad) == 0, [(int(i), err[i], tol[i], kappa[i]) for i in bad[:8]]
    assert np.all(got[NN == O.NA] == 0.0)
    # the diagonal of the precision from the device's own factor (the factor's
    # error, up to 1e-14 cond, is judged above)
    np.testing.assert_allclose(ctx.precision_diag(), O.precision_diag(got, NN), rtol=1e-10)
    return float(ratio[w])


def _clear_env(monkeypatch, **env):
    for k in ("NNGP_FACTOR_LANES", "NNGP_FACTOR_PAIR", "NNGP_FACTOR_JOBS", "NNGP_FACTOR_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run_cells(P, O, monkeypatch, n, m, d, covs, label, **env):
    _clear_env(monkeypatch, **env)
    prob = _problem(P, n, m, d)
    print()
    with P.ChainContext(*prob, device=0) as ctx:
        for covfun, base in covs:
            for nug in NUGGETS:
                _judge(O, ctx, n, m, d, covfun, base + [nug], prob, label)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("m", MS)
def test_factor_cells(P, O, monkeypatch, m, d):
    """factor_kernel<BM, FAM, DS> (b <= 21) and factor_kernel_rt<FAM, DS>
    (b = 22, 32), FAM 0 and 1"""
    _run_cells(P, O, monkeypatch, 300, m, d, _covs(d), "default")


@pytest.mark.parametrize("m,d", [(m, d) for m in MS for d in DS if _covs_matern(m, d)])
def test_factor_cells_general_matern(P, O, monkeypatch, m, d):
    """factor_kernel_rt<2, DS>: matern_isotropic (nu = 1.0, 2.5) at m = 11, 31;
    matern_scaledim (nu = 2.5) and matern_spacetime (nu = 0.75) at d = 3, 4"""
    _run_cells(P, O, monkeypatch, 64, m, d, _covs_matern(m, d), "default")


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("m", [m for m in MS if m + 1 <= 16])
def test_factor_cells_lane_groups(P, O, monkeypatch, m, d):
    """NNGP_FACTOR_LANES=16: factor_lanes_kernel<FAM, DS>, b <= 16"""
    _run_cells(P, O, monkeypatch, 300, m, d, _covs(d), "lanes16", NNGP_FACTOR_LANES="16")


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("m", [12, 15])
def test_factor_cells_lane_pairs(P, O, monkeypatch, m, d):
    """NNGP_FACTOR_PAIR=1: factor_pair_kernel<16, FAM, DS>, b = 13 and 16"""
    _run_cells(P, O, monkeypatch, 300, m, d, _covs(d), "pair", NNGP_FACTOR_PAIR="1")


# ---------------------------------------------------------------- multi-chain launch
def _chain_parms(covfun, base, d):
    """three chains: another variance, ranges (x 1, x 2, x 1/2) and nugget each"""
    out = []
    for var, s, nug in [(1.0, 1.0, 0.0), (1.5, 2.0, 0.1), (0.75, 0.5, 0.01)]:
        out.append([base[0] * var] + [r * s for r in base[1:]] + [nug])
    return out


CHAIN_CELLS = ([(m, d, "default") for m in (7, 11, 15, 20, 31) for d in DS] +
               [(m, d, "lanes16") for m in (7, 11, 15) for d in DS] + [(15, d, "pair") for d in DS])


@pytest.mark.parametrize("m,d,mode", CHAIN_CELLS)
def test_factor_chains_bitwise_equal_to_factor(P, monkeypatch, m, d, mode):
    """One cell per (BM, DS): factor_chains with 3 chains of different
    parameters == factor chain by chain, bitwise (kernels.h), FAM 0 and 1;
    also under the lane-group (b <= 16) and lane-pair (b = 16) opt-ins."""
    _clear_env(monkeypatch, **{"lanes16": {"NNGP_FACTOR_LANES": "16"}, "pair": {"NNGP_FACTOR_PAIR": "1"}}.get(mode, {}))
    prob = _problem(P, 300, m, d)
    with P.ChainContext(*prob, device=0, n_chains=3) as ctx:
        for covfun, base in _covs(d):
            cps = _chain_parms(covfun, base, d)
            st = ctx.factor_chains(0, 7, covfun, cps)
            assert (st == 0).all(), st
            jobs = [ctx.select(k).get_linv(0) for k in range(3)]
            assert not np.array_equal(jobs[0], jobs[1]) and not np.array_equal(jobs[1], jobs[2])
            for k in range(3):
                ctx.select(k).factor(0, covfun, cps[k])
                np.testing.assert_array_equal(ctx.get_linv(0), jobs[k], err_msg=f"{covfun}, chain {k}")
            ctx.select(0)


# ---------------------------------------------------------------- the failing-row number
K0, K1, N_FAIL = 137, 201, 300


def _failing_chain(P, O, m):
    """A one-neighbour chain stored with b = m + 1 columns (every column past
    the second NA: every row a short row), zig-zag on the x axis with gaps in
    [0.5, 2) -- except that points K0 and K1 coincide with their neighbour.
    With nugget -1e-3 exactly those two blocks are not positive definite
    (pivot 0.999 - 1 / 0.999 = -0.002); every other block is (correlation <=
    0.91 for the covariances used)."""
    key = ("fail", m)
    if key not in _cache:
        rng = np.random.default_rng(m)
        g = rng.uniform(0.5, 2.0, N_FAIL)
        x = np.zeros(N_FAIL)
        for i in range(1, N_FAIL):
            x[i] = x[i - 1] if i in (K0, K1) else (g[i] if x[i - 1] == 0.0 else 0.0)
        locs = np.column_stack([x, np.zeros(N_FAIL)])
        NN = np.full((N_FAIL, m + 1), O.NA, np.int32)
        NN[:, 0] = np.arange(1, N_FAIL + 1)
        NN[1:, 1] = np.arange(1, N_FAIL)
        _cache[key] = (locs, NN, P.naive_greedy_coloring(NN), np.arange(1, N_FAIL + 1, dtype=np.int32),
                       np.zeros(N_FAIL))
    return _cache[key]


def _row_of(msg):
    rows = re.findall(r"row (\d+)", str(msg))
    assert len(rows) == 1, msg
    return int(rows[0])


FAIL_CASES = ([(m, cf, "default") for m in (1, 8, 12, 16, 21, 31) for cf in ("exponential_isotropic", "matern15_isotropic")]
              + [(8, "matern_isotropic", "default")]
              + [(m, cf, "lanes16") for m in (1, 8, 12, 15) for cf in ("exponential_isotropic", "matern15_isotropic")]
              + [(m, cf, "pair") for m in (12, 15) for cf in ("exponential_isotropic", "matern15_isotropic")])


@pytest.mark.parametrize("m,covfun,mode", FAIL_CASES)
def test_failing_row_number(P, O, monkeypatch, m, covfun, mode):
    """NNGP_ERR_CHOL names 1 + the first failing row (atomicMin over the
    rows), the row the oracle names on the same blocks: factor_row,
    factor_kernel_rt, factor_lanes_kernel, factor_pair_kernel, and the
    multi-job launch, where only the chain with the bad nugget fails and the
    others' factors are bitwise those of factor alone."""
    from nngp_amd._lib import lib

    _clear_env(monkeypatch, **{"lanes16": {"NNGP_FACTOR_LANES": "16"}, "pair": {"NNGP_FACTOR_PAIR": "1"}}.get(mode, {}))
    prob = _failing_chain(P, O, m)
    locs, NN = prob[0], prob[1]
    mid = [1.0] if covfun == "matern_isotropic" else []
    bad, good = [1.0, 1.0] + mid + [-1e-3], [1.0, 1.0] + mid + [0.1]
    # the oracle takes GpGp's bsize = min(i + 1, b): the same blocks as two columns
    with pytest.raises(np.linalg.LinAlgError) as oe:
        O.vecchia_linv(covfun, bad, locs, NN[:, :2])
    assert _row_of(oe.value) == K0 + 1
    with P.ChainContext(*prob, device=0, n_chains=3) as ctx:
        with pytest.raises(P.NNGPError) as e:
            ctx.factor(0, covfun, bad)
        assert e.value.status == 3
        assert _row_of(e.value) == K0 + 1 == _row_of(oe.value)
        alone = []
        for k in (0, 2):
            ctx.select(k).factor(0, covfun, good)
            alone.append(ctx.get_linv(0))
        ctx.select(0)
        st = ctx.factor_chains(0, 7, covfun, [good, bad, good])
        assert list(st) == [0, 3, 0], st
        assert _row_of(lib.nngp_ctx_last_error(ctx._h).decode()) == K0 + 1
        for k, want in zip((0, 2), alone):
            np.testing.assert_array_equal(ctx.select(k).get_linv(0), want, err_msg=f"chain {k}")
        with pytest.raises(P.NNGPError) as e1:   # chain 1 holds no factor
            ctx.select(1).get_linv(0)
        assert e1.value.status == 4
        # the good factor itself: the two-column oracle on the same blocks
        ref = O.vecchia_linv(covfun, good, locs, NN[:, :2])
        np.testing.assert_allclose(alone[0][:, :2], ref, rtol=1e-9, atol=1e-10)
        assert np.all(alone[0][:, 2:] == 0.0)
