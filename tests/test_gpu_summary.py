"""get_summary on the device (nngp_summary, csrc/summary.hip): mean, type-7
quantiles 0.025 / 0.5 / 0.975 and sd per column by an exact radix select,
against the host get_summary (numpy) throughout.

Bounds (eps = 2^-52), from the arithmetic, not from the results:
  quantile: within [x_(j), x_(j+1)] and |dev - numpy| <= 8 eps max(|x_(j)|, |x_(j+1)|)
            (at most three roundings of quantities <= 2 max per evaluation,
            one product possibly contracted); exact ranks (g = 0) bitwise;
  mean:     |dev - numpy| <= S eps mean|x| (recursive summation's first-order
            bound (S - 1) 2^-53 mean|x|, doubled for numpy's own rounding);
  sd:       relative difference <= (S + 4) eps (data with |mean| <= 10 sd).
Measured maxima on the MI355X over every case of this file, as fractions of
the bounds: quantile 0 and sd 0 (bitwise numpy's), mean 0 on every matrix of
two or more columns and 0.027 at n = 1 (a single column is contiguous for
numpy, which then sums pairwise; the kernel sums in row order and contracts
nothing).  The bounds stay as derived.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
QS = (0.025, 0.5, 0.975)


def _dev(P, x, **kw):
    return P.get_summary(x, backend="hip", device=0, **kw)


def _check_vs_host(P, got, x, what=""):
    """got: device summary of the S x n matrix x; asserts the module's bounds
    against the host get_summary and prints the measured maxima as fractions
    of the bounds."""
    x = np.asarray(x, np.float64)
    S, n = x.shape
    ref = P.get_summary(x) if S > 1 else np.column_stack([x[0]] * 4 + [np.full(n, np.nan)])
    assert got.shape == (n, 5)
    xs = np.sort(x, 0)
    worst_q = 0.0
    for k, q in enumerate(QS):
        h = q * (S - 1)
        j = int(np.floor(h))
        a, b = xs[j], xs[min(j + 1, S - 1)]
        assert np.all((a <= got[:, 1 + k]) & (got[:, 1 + k] <= b)), (what, q)
        bound = 8 * EPS * np.maximum(np.abs(a), np.abs(b))
        d = np.abs(got[:, 1 + k] - ref[:, 1 + k])
        worst_q = max(worst_q, float(np.max(d / np.where(bound > 0, bound, 1.0))))
        assert np.all(d <= bound), (what, q, float(d.max()))
        if h == j:
            np.testing.assert_array_equal(got[:, 1 + k], a)
    bound = S * EPS * np.abs(x).mean(0)
    d = np.abs(got[:, 0] - ref[:, 0])
    worst_mean = float(np.max(d / np.where(bound > 0, bound, 1.0)))
    assert np.all(d <= bound), (what, "mean", float(d.max()))
    worst_sd = 0.0
    if S > 1:
        d = np.abs(got[:, 4] - ref[:, 4])
        bound = (S + 4) * EPS * np.abs(ref[:, 4])
        worst_sd = float(np.max(d / np.where(bound > 0, bound, 1.0)))
        assert np.all(d <= bound), (what, "sd", float(d.max()))
    else:
        assert np.all(np.isnan(got[:, 4]))
    print(f"summary {what} S={S} n={n}: fraction of bound used: quantile {worst_q:.3g} mean {worst_mean:.3g} "
          f"sd {worst_sd:.3g}")


def test_exact_ranks_bitwise(P):
    """S = 41: q (S - 1) = 1, 20, 39 exactly, so the quantiles are rows 1, 20
    and 39 of the sorted matrix bit for bit."""
    assert [q * 40 for q in QS] == [1.0, 20.0, 39.0]
    x = 0.5 + np.random.default_rng(41).normal(size=(41, 1000))
    got = _dev(P, x)
    xs = np.sort(x, 0)
    for k, j in enumerate((1, 20, 39)):
        np.testing.assert_array_equal(got[:, 1 + k], xs[j])
    _check_vs_host(P, got, x, "exact ranks")


@pytest.mark.parametrize("S", [2, 3, 5, 64, 65, 257, 1000])
def test_interpolated_ranks_mean_sd(P, S):
    x = -2.0 + 1.3 * np.random.default_rng(S).normal(size=(S, 130))
    _check_vs_host(P, _dev(P, x), x, "interpolated")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_chunk_independence(P, n):
    """The same columns through chunks of 64, 192 and the automatic width
    (one launch here): bitwise the same five numbers."""
    x = 1.0 + np.random.default_rng(n).normal(size=(33, n))
    outs = [_dev(P, x, chunk_cols=w) for w in (64, 192, 0)]
    np.testing.assert_array_equal(outs[0], outs[2])
    np.testing.assert_array_equal(outs[1], outs[2])
    _check_vs_host(P, outs[2], x, "chunks")


def test_position_independence(P):
    rng = np.random.default_rng(7)
    x = rng.normal(size=(65, 130))
    wide = 4.0 * rng.normal(size=(65, 1000))
    wide[:, 517] = x[:, 3]
    wide[:, 0] = x[:, 100]
    wide[:, 999] = x[:, 129]
    base = _dev(P, x)
    for kw in ({}, {"chunk_cols": 192}):
        got = _dev(P, wide, **kw)
        np.testing.assert_array_equal(got[517], base[3])
        np.testing.assert_array_equal(got[0], base[100])
        np.testing.assert_array_equal(got[999], base[129])


def test_blocks_and_offsets(P):
    """Blocks of 7, 1 and 33 rows (a column-major array that has to be copied,
    a single row, a row-suffix view of a larger array) with row offsets:
    bitwise the device result on the stacked, centred matrix."""
    rng = np.random.default_rng(3)
    n = 200
    a = np.asfortranarray(rng.normal(size=(7, n)))
    b = rng.normal(size=(1, n))
    big = rng.normal(size=(40, n))
    c = big[7:]
    assert c.base is big and c.flags.c_contiguous and not a.flags.c_contiguous
    off = rng.normal(size=41)
    stacked = np.vstack([a, b, c]) - off[:, None]
    got = _dev(P, [a, b, c], row_offset=off)
    np.testing.assert_array_equal(got, _dev(P, stacked))
    np.testing.assert_array_equal(got, _dev(P, [a, b, c], row_offset=off, chunk_cols=64))
    _check_vs_host(P, got, stacked, "blocks")
    np.testing.assert_array_equal(P.get_summary([a, b, c], row_offset=off), P.get_summary(stacked))


def test_ties_and_specials(P):
    rng = np.random.default_rng(11)
    S = 64
    x = rng.normal(size=(S, 7))
    x[:, 0] = 2.5  # all equal
    x[:, 1] = rng.choice([-2.0, 0.0, 5.0], size=S)  # heavy ties
    x[:, 2] = np.where(rng.integers(0, 2, size=S) == 1, 0.0, -0.0)
    x[:, 5] = rng.choice([-2.0, 0.0, 5.0], size=S)
    clean = _dev(P, x)
    _check_vs_host(P, clean, x, "ties")
    np.testing.assert_array_equal(clean[0], [2.5, 2.5, 2.5, 2.5, 0.0])
    assert np.all(clean[2] == 0.0)
    bad = x.copy()
    bad[17, 4] = np.nan
    got = _dev(P, bad)
    assert np.all(np.isnan(got[4]))
    keep = [0, 1, 2, 3, 5, 6]
    np.testing.assert_array_equal(got[keep], clean[keep])
    np.testing.assert_array_equal(_dev(P, bad, chunk_cols=64)[keep], clean[keep])


def test_single_row(P):
    x = np.random.default_rng(1).normal(size=(1, 10))
    got = _dev(P, x)
    assert np.all(np.isnan(got[:, 4]))
    for k in range(4):
        np.testing.assert_array_equal(got[:, k], x[0])
    _check_vs_host(P, got, x, "one row")
    v = np.random.default_rng(2).normal(size=50)  # a vector is one column of 50 samples
    np.testing.assert_array_equal(_dev(P, v), _dev(P, v[:, None]))
    _check_vs_host(P, _dev(P, v), v[:, None], "vector")


def test_many_rows_one_column(P):
    """More rows than any register file or LDS holds: S = 100 000."""
    x = 3.0 + np.random.default_rng(5).normal(size=(100_000, 2))
    _check_vs_host(P, _dev(P, x), x, "long column")


def test_errors(P):
    for x in (np.empty((0, 5)), np.empty((3, 0))):
        with pytest.raises(P.NNGPError) as e:
            _dev(P, x)
        assert e.value.status == 1
    with pytest.raises(P.NNGPError) as e:
        _dev(P, np.zeros((3, 4)), chunk_cols=-1)
    assert e.value.status == 1


@pytest.fixture(scope="module")
def toy_run(P, toy):
    """Vignette toy (n = 2000, m = 5), 2 chains, 30 iterations with
    field_thinning = .5, as tests/test_gpu_predict.py sets it up."""
    L = P.mcmc_nngp_initialize(toy["locs"], toy["observed_field"], X_locs=toy["X"],
                               stationary_covfun="exponential_isotropic", m=5, n_chains=2, seed=3)
    L = P.mcmc_nngp_run(L, n_cycles=1, n_iterations_update=30, n_chromatic=3, field_thinning=0.5,
                        Gelman_Rubin_Brooks_stop=(1.0, 1.0), verbose=False)
    yield L
    for c in L["_contexts"]:
        c.close()


def _assert_same(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _assert_same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)) and not (a and isinstance(a[0], str)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _assert_same(u, v, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a, b, err_msg=path)
    else:
        assert a == b, path


def test_estimate_field_backend(P, toy_run):
    L = toy_run
    ref = P.mcmc_nngp_estimate(L)
    got = P.mcmc_nngp_estimate(L, field_backend="hip", device=0)
    assert got.keys() == ref.keys()
    for k in ref:
        if k != "field":
            _assert_same(got[k], ref[k], k)
    # the matrix res$field summarises (estimate.R:89-96)
    recs = list(L["records"].values())
    saved = recs[0]["saved_field"]
    it = int(recs[0]["iterations"][-1, 0])
    sel = saved > it * 0.5
    x = np.vstack([c["params"]["field"][sel] - c["params"]["beta_0"][saved[sel].astype(int) - 1, 0][:, None]
                   for c in recs])
    assert x.shape[0] >= 4 and x.shape[1] == L["locs"].shape[0]
    np.testing.assert_array_equal(ref["field"], P.get_summary(x))
    _check_vs_host(P, got["field"], x, "estimate field")


def test_predict_field_summary_backend(P, toy_run):
    L = toy_run
    rng = np.random.default_rng(5)
    lo, hi = L["locs"].min(0), L["locs"].max(0)
    pred = lo + (hi - lo) * rng.uniform(size=(300, L["locs"].shape[1]))
    stored = list(L["records"].values())[0]["saved_field"]
    n_s = int((stored > 0.5 * stored.max()).sum())
    z = [np.random.default_rng(99 + k).normal(size=(n_s, 300)) for k in range(len(L["records"]))]
    ref = P.mcmc_nngp_predict_field(L, pred, m=5, z_new=z, device=0)
    got = P.mcmc_nngp_predict_field(L, pred, m=5, z_new=z, device=0, summary_backend="hip")
    _assert_same(got["predicted_field_samples"], ref["predicted_field_samples"], "samples")
    np.testing.assert_array_equal(got["predicted_locs"], ref["predicted_locs"])
    _check_vs_host(P, got["predicted_field_summary"], np.vstack(ref["predicted_field_samples"]), "predict summary")
