"""Chosen quantiles and exceedance probabilities on the device
(nngp_summary_probs, csrc/summary.hip: summary_probs_kernel) against numpy.

Bounds (eps = 2^-52), those derived in tests/test_gpu_summary.py from the
arithmetic:
  quantile: within [x_(j), x_(j+1)] and |dev - numpy| <= 8 eps max(|x_(j)|, |x_(j+1)|);
            exact ranks (g = 0) bitwise the sorted value;
  mean:     |dev - numpy| <= S eps mean|x|;
  sd:       relative difference <= (S + 4) eps.
Exceedance fractions are an integer count and one division, so they are
bitwise (x > t).sum(0) / S.  The select is exact and the interpolation is one
shared function of (x_(j), x_(j+1), g), so a quantile's bits may depend on its
column and its own q only: asked alone, among 16, in another order or beside
thresholds it is the same double, and equal to nngp_summary's for its three.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
DEFAULT = (0.025, 0.5, 0.975)
# 16 probabilities: 0, 1, a repeat, unsorted
P16 = (0.9, 0.0, 0.25, 1.0, 0.25, 0.05, 0.5, 0.975, 0.025, 0.75, 0.1, 0.333, 0.95, 0.5, 0.01, 0.6)
T8 = (0.0, 0.5, -np.inf, np.inf, -1.25, 2.0, 1e-3, -0.0)


def _dev(P, x, probs=None, thresholds=None, **kw):
    return P.get_summary(x, backend="hip", device=0, probs=probs, thresholds=thresholds, **kw)


def _check(got, x, probs, thr, what=""):
    """got: device summary of the S x n matrix x for (probs, thr); asserts the
    module's bounds against numpy."""
    x = np.asarray(x, np.float64)
    S, n = x.shape
    Q, K = len(probs), len(thr)
    assert got.shape == (n, 2 + Q + K), (what, got.shape)
    xs = np.sort(x, 0)
    for k, q in enumerate(probs):
        h = q * (S - 1)
        j = int(np.floor(h))
        a, b = xs[j], xs[min(j + 1, S - 1)]
        col = got[:, 1 + k]
        assert np.all((a <= col) & (col <= b)), (what, q)
        # numpy's own lerp of two equal infinities is NaN (inf - inf): where a
        # neighbour is infinite the bracket above and the exact rank below decide
        fin = np.isfinite(a) & np.isfinite(b)
        d = np.abs(col - np.quantile(x, q, axis=0))[fin]
        assert np.all(d <= (8 * EPS * np.maximum(np.abs(a), np.abs(b)))[fin]), (what, q, float(d.max(initial=0.0)))
        if h == j:
            np.testing.assert_array_equal(col, a, err_msg=f"{what} exact rank q={q}")
    finite = np.isfinite(x).all(0)
    d = np.abs(got[:, 0] - x.mean(0))[finite]
    assert np.all(d <= S * EPS * np.abs(x).mean(0)[finite]), (what, "mean", float(d.max(initial=0.0)))
    if S > 1:
        ref = x[:, finite].std(0, ddof=1)
        d = np.abs(got[finite, 1 + Q] - ref)
        assert np.all(d <= (S + 4) * EPS * np.abs(ref)), (what, "sd", float(d.max(initial=0.0)))
    else:
        assert np.all(np.isnan(got[:, 1 + Q]))
    for k, t in enumerate(thr):
        np.testing.assert_array_equal(got[:, 2 + Q + k], (x > t).sum(0) / S, err_msg=f"{what} threshold {t}")


@pytest.mark.parametrize("off", [False, True])
@pytest.mark.parametrize("S", [1, 2, 41, 65])
def test_default_request_is_the_old_entry_bitwise(P, S, off):
    rng = np.random.default_rng(S)
    x = 0.5 + rng.normal(size=(S, 130))
    kw = {"row_offset": rng.normal(size=S)} if off else {}
    old = P.get_summary(x, backend="hip", device=0, **kw)
    np.testing.assert_array_equal(_dev(P, x, probs=DEFAULT, **kw), old)
    np.testing.assert_array_equal(_dev(P, x, thresholds=(), **kw), old)


@pytest.mark.parametrize("S", [2, 3, 5, 64, 65, 257])
def test_sizes_against_numpy(P, S):
    """Q in {0, 1, 4, 7, 16} (both sides of the rounds of three ranks, and the
    maximum) with K in {0, 1, 8}, n = 130 (more than two wavefronts, not a
    multiple of 64)."""
    x = -0.2 + 1.3 * np.random.default_rng(S).normal(size=(S, 130))
    x[0, 5] = 0.5  # a threshold equal to a data value
    for Q, K in ((0, 0), (0, 8), (1, 1), (4, 0), (4, 8), (7, 1), (16, 0), (16, 8)):
        _check(_dev(P, x, probs=P16[:Q], thresholds=T8[:K]), x, P16[:Q], T8[:K], f"S={S} Q={Q} K={K}")


def test_request_independence(P):
    x = 0.1 + np.random.default_rng(9).normal(size=(65, 130))
    full = _dev(P, x, probs=P16, thresholds=T8)
    _check(full, x, P16, T8, "full request")
    order = np.random.default_rng(1).permutation(16)
    shuffled = _dev(P, x, probs=[P16[i] for i in order])
    no_probs = _dev(P, x, probs=(), thresholds=T8)
    for i, q in enumerate(P16):
        alone = _dev(P, x, probs=(q,))
        np.testing.assert_array_equal(alone[:, 1], full[:, 1 + i], err_msg=f"q={q} alone")
        np.testing.assert_array_equal(alone[:, [0, 2]], full[:, [0, 17]])
        np.testing.assert_array_equal(shuffled[:, 1 + int(np.nonzero(order == i)[0][0])], full[:, 1 + i])
    np.testing.assert_array_equal(full[:, 1 + 2], full[:, 1 + 4])  # the repeated 0.25
    np.testing.assert_array_equal(no_probs[:, 2:], full[:, 18:])
    for k, t in enumerate(T8):
        one = _dev(P, x, probs=(0.3, 0.7), thresholds=(t,))
        np.testing.assert_array_equal(one[:, 4], full[:, 18 + k], err_msg=f"threshold {t} alone")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_chunk_independence(P, n):
    x = 1.0 + np.random.default_rng(n).normal(size=(33, n))
    probs, thr = P16[:7], T8[:3]
    outs = [_dev(P, x, probs=probs, thresholds=thr, chunk_cols=w) for w in (64, 192, 0)]
    np.testing.assert_array_equal(outs[0], outs[2])
    np.testing.assert_array_equal(outs[1], outs[2])
    _check(outs[2], x, probs, thr, "chunks")


def test_position_independence(P):
    rng = np.random.default_rng(7)
    x = rng.normal(size=(65, 130))
    wide = 4.0 * rng.normal(size=(65, 1000))
    wide[:, 517] = x[:, 3]
    wide[:, 0] = x[:, 100]
    wide[:, 999] = x[:, 129]
    base = _dev(P, x, probs=P16[:7], thresholds=T8[:3])
    for kw in ({}, {"chunk_cols": 192}):
        got = _dev(P, wide, probs=P16[:7], thresholds=T8[:3], **kw)
        np.testing.assert_array_equal(got[517], base[3])
        np.testing.assert_array_equal(got[0], base[100])
        np.testing.assert_array_equal(got[999], base[129])


def test_blocks_and_offsets(P):
    """A column-major block that has to be copied, a one-row block and a
    row-suffix view, with row offsets: bitwise the device result on the
    stacked, centred matrix; thresholds apply after the offset."""
    rng = np.random.default_rng(3)
    n = 200
    a = np.asfortranarray(rng.normal(size=(7, n)))
    b = rng.normal(size=(1, n))
    big = rng.normal(size=(40, n))
    c = big[7:]
    assert c.base is big and c.flags.c_contiguous and not a.flags.c_contiguous
    off = rng.normal(size=41)
    stacked = np.vstack([a, b, c]) - off[:, None]
    probs, thr = P16[:5], (0.0, float(stacked[3, 8]))
    got = _dev(P, [a, b, c], probs=probs, thresholds=thr, row_offset=off)
    np.testing.assert_array_equal(got, _dev(P, stacked, probs=probs, thresholds=thr))
    np.testing.assert_array_equal(got, _dev(P, [a, b, c], probs=probs, thresholds=thr, row_offset=off, chunk_cols=64))
    _check(got, stacked, probs, thr, "blocks")


def test_ties_and_specials(P):
    rng = np.random.default_rng(11)
    S = 64
    x = rng.normal(size=(S, 9))
    x[:, 0] = 2.5  # constant
    x[:, 1] = rng.choice([-2.0, 5.0], size=S)  # two-valued
    x[:, 2] = np.where(rng.integers(0, 2, size=S) == 1, 0.0, -0.0)  # signed zeros
    x[rng.choice(S, 5, replace=False), 3] = np.inf
    x[rng.choice(S, 5, replace=False), 7] = -np.inf
    x[:3, 8] = np.inf
    x[3:5, 8] = -np.inf
    probs = (0.0, 0.3, 0.5, 1.0)
    thr = (0.0, 2.5, 5.0, -2.0, np.inf, -np.inf, float(x[10, 5]))
    clean = _dev(P, x, probs=probs, thresholds=thr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # numpy's inf - inf in its own lerp
        _check(clean, x, probs, thr, "ties")
    # the constant column: mean and quantiles 2.5, sd 0, then 2.5 > t for each threshold
    np.testing.assert_array_equal(clean[0], [2.5] * 5 + [0.0] + [float(2.5 > t) for t in thr])
    assert np.all(clean[2, 1:5] == 0.0) and clean[2, 6] == 0.0  # neither zero exceeds 0.0
    assert clean[3, 4] == np.inf and clean[7, 1] == -np.inf and clean[8, 1] == -np.inf and clean[8, 4] == np.inf
    bad = x.copy()
    bad[17, 4] = np.nan
    got = _dev(P, bad, probs=probs, thresholds=thr)
    assert np.all(np.isnan(got[4]))
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    np.testing.assert_array_equal(got[keep], clean[keep])
    np.testing.assert_array_equal(_dev(P, bad, probs=probs, thresholds=thr, chunk_cols=64)[keep], clean[keep])


def test_single_row(P):
    x = np.random.default_rng(1).normal(size=(1, 10))
    probs, thr = (0.0, 0.4, 1.0, 0.975), (0.0, -np.inf, np.inf)
    got = _dev(P, x, probs=probs, thresholds=thr)
    assert got.shape == (10, 9)
    for k in range(5):
        np.testing.assert_array_equal(got[:, k], x[0])
    assert np.all(np.isnan(got[:, 5]))
    np.testing.assert_array_equal(got[:, 6], (x[0] > 0.0).astype(float))
    np.testing.assert_array_equal(got[:, 7], np.ones(10))
    np.testing.assert_array_equal(got[:, 8], np.zeros(10))
    _check(got, x, probs, thr, "one row")


def test_errors_are_status_1_and_leave_the_device_alone(P):
    """The library's own argument checks (Python's ValueError comes first in
    get_summary, so the entry point is called directly): status 1, the output
    untouched, and the next good call unaffected."""
    x = np.random.default_rng(0).normal(size=(7, 5))
    rows, ptrs = (C.c_longlong * 1)(7), (C.c_void_p * 1)(x.ctypes.data)
    before = _dev(P, x, probs=P16[:4], thresholds=T8[:2])

    def status(probs, thr):
        p, t = np.asarray(probs, np.float64), np.asarray(thr, np.float64)
        out = np.full((2 + 17 + 9, 5), -7.0)
        st = P.lib.nngp_summary_probs(0, ptrs, rows, 1, 5, None, 0, p.ctypes.data if p.size else None, p.size,
                                      t.ctypes.data if t.size else None, t.size, out)
        assert np.all(out == -7.0)
        return st

    assert status(np.linspace(0, 1, 17), ()) == 1
    assert status((), np.arange(9.0)) == 1
    assert status((0.5, 1.0000001), ()) == 1
    assert status((np.nan,), ()) == 1
    assert status((0.5,), (np.nan,)) == 1
    np.testing.assert_array_equal(_dev(P, x, probs=P16[:4], thresholds=T8[:2]), before)
    for kw in ({"probs": np.linspace(0, 1, 17)}, {"thresholds": np.arange(9.0)}, {"probs": (1.0000001,)},
               {"probs": (np.nan,)}, {"thresholds": (np.nan,)}):
        with pytest.raises(ValueError):
            _dev(P, x, **kw)


def test_stats_report_the_last_call_of_either_entry(P):
    from nngp_amd import estimate

    x = np.random.default_rng(2).normal(size=(10, 300))
    _dev(P, x, probs=(0.5,), chunk_cols=64)
    assert estimate.summary_stats()["chunk_cols"] == 64 and estimate.summary_stats()["staged_bytes"] == 8 * 10 * 300
    P.get_summary(x, backend="hip", device=0, chunk_cols=128)
    assert estimate.summary_stats()["chunk_cols"] == 128
    _dev(P, x[:, :100], thresholds=(0.0,), chunk_cols=192)
    assert estimate.summary_stats()["chunk_cols"] == 100 and estimate.summary_stats()["staged_bytes"] == 8 * 10 * 100


@pytest.fixture(scope="module")
def toy_run(P, toy):
    """Vignette toy (n = 2000, m = 5), 2 chains, 30 iterations with
    field_thinning = .5, as tests/test_gpu_summary.py sets it up."""
    L = P.mcmc_nngp_initialize(toy["locs"], toy["observed_field"], X_locs=toy["X"],
                               stationary_covfun="exponential_isotropic", m=5, n_chains=2, seed=3)
    L = P.mcmc_nngp_run(L, n_cycles=1, n_iterations_update=30, n_chromatic=3, field_thinning=0.5,
                        Gelman_Rubin_Brooks_stop=(1.0, 1.0), verbose=False)
    yield L
    for c in L["_contexts"]:
        c.close()


FIELD_PROBS, FIELD_THR = (0.05, 0.25, 0.75, 0.95), (0.0, 0.5)
FIELD_COLS = ["mean", "q0.05", "q0.25", "q0.75", "q0.95", "sd", "p_gt_0", "p_gt_0.5"]


def test_estimate_field_backend(P, toy_run):
    L = toy_run
    ref = P.mcmc_nngp_estimate(L, field_probs=FIELD_PROBS, field_thresholds=FIELD_THR)
    got = P.mcmc_nngp_estimate(L, field_backend="hip", device=0, field_probs=FIELD_PROBS, field_thresholds=FIELD_THR)
    assert got.keys() == ref.keys() and got["field_columns"] == ref["field_columns"] == FIELD_COLS
    recs = list(L["records"].values())
    saved = recs[0]["saved_field"]
    it = int(recs[0]["iterations"][-1, 0])
    sel = saved > it * 0.5
    x = np.vstack([c["params"]["field"][sel] - c["params"]["beta_0"][saved[sel].astype(int) - 1, 0][:, None]
                   for c in recs])
    assert x.shape[0] >= 4 and x.shape[1] == L["locs"].shape[0]
    np.testing.assert_array_equal(ref["field"], P.get_summary(x, probs=FIELD_PROBS, thresholds=FIELD_THR))
    _check(got["field"], x, FIELD_PROBS, FIELD_THR, "estimate field")
    np.testing.assert_array_equal(got["field"][:, 6:], ref["field"][:, 6:])
    plain = P.mcmc_nngp_estimate(L, field_backend="hip", device=0)
    assert "field_columns" not in plain and plain["field"].shape == (x.shape[1], 5)
    np.testing.assert_array_equal(got["field"][:, [0, 5]], plain["field"][:, [0, 4]])


def test_predict_field_summary_backend(P, toy_run):
    L = toy_run
    rng = np.random.default_rng(5)
    lo, hi = L["locs"].min(0), L["locs"].max(0)
    pred = lo + (hi - lo) * rng.uniform(size=(300, L["locs"].shape[1]))
    stored = list(L["records"].values())[0]["saved_field"]
    n_s = int((stored > 0.5 * stored.max()).sum())
    z = [np.random.default_rng(99 + k).normal(size=(n_s, 300)) for k in range(len(L["records"]))]
    kw = dict(m=5, z_new=z, device=0, engine="batched", summary_probs=FIELD_PROBS, summary_thresholds=FIELD_THR)
    ref = P.mcmc_nngp_predict_field(L, pred, **kw)
    got = P.mcmc_nngp_predict_field(L, pred, summary_backend="hip", **kw)
    assert got["predicted_field_summary_columns"] == ref["predicted_field_summary_columns"] == FIELD_COLS
    for a, b in zip(got["predicted_field_samples"], ref["predicted_field_samples"]):
        np.testing.assert_array_equal(a, b)
    x = np.vstack(ref["predicted_field_samples"])
    np.testing.assert_array_equal(ref["predicted_field_summary"],
                                  P.get_summary(x, probs=FIELD_PROBS, thresholds=FIELD_THR))
    _check(got["predicted_field_summary"], x, FIELD_PROBS, FIELD_THR, "predict summary")
    np.testing.assert_array_equal(got["predicted_field_summary"][:, 6:], ref["predicted_field_summary"][:, 6:])
