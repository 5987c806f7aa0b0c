"""The two references of the Vecchia factor against each other, on the CPU:
tests/highprec.py (mpmath at 40 digits, np.longdouble) and the C oracle
(fp64).  Each then vouches for the other before either judges the device
(test_gpu_covariance_accuracy.py, test_gpu_factor_matrix.py).

Bounds:
  corr_mp vs oracle.bessel_k ...... 1e-12 relative (the oracle's trapezoid
      rule and libm lgamma / pow; DESIGN.md section 4 claims 1e-14 for it)
  covmat, exponential / Matern 3/2  1e-14 relative: with exact scaled
      coordinates the oracle's distance is within 1 ulp, which exp turns into
      (1 + dist) 2^-53 <= 4e-15 at the distances here (<= 32), plus 2 roundings
  covmat, general Matern ........... 1e-12 relative (bessel_k above)
  vecchia_linv ..................... per row max(1e-10, 1e-14 cond(C_i)) max|row|
      (test_gpu_parity._assert_rows_close)
"""
import mpmath
import numpy as np
import pytest

import highprec as H
from test_gpu_parity import _assert_rows_close

# covfun -> covparms for d-dimensional locations (ranges are powers of two)
CASES = {
    "exponential_isotropic": lambda d: [1.3, 0.25, 0.0],
    "matern15_isotropic": lambda d: [0.7, 0.0625, 0.1],
    "matern_isotropic": lambda d: [1.0, 0.0625, 1.0, 0.0],
    "exponential_scaledim": lambda d: [1.0] + [0.25, 0.5, 0.125, 1.0][:d] + [0.1],
    "matern_scaledim": lambda d: [1.0] + [0.125, 0.25, 0.0625, 0.5][:d] + [2.5, 0.0],
    "exponential_spacetime": lambda d: [2.0, 0.25, 0.5, 0.0],
    "matern_spacetime": lambda d: [1.0, 0.125, 0.25, 0.8, 0.1],
}


@pytest.mark.parametrize("nu", [0.05, 0.5, 1.0, 1.04, 2.0, 2.5, 3.0, 10.0])
def test_corr_mp_matches_oracle_bessel(O, nu):
    for x in [1e-6, 0.01, 0.3, 1.4999, 1.5, 1.5000001, 1.9, 7.0, 30.0, 59.0, 61.0, 300.0]:
        ref = H.corr_mp("matern_isotropic", nu, x)
        got = 2.0 ** (1.0 - nu) / float(mpmath.gamma(nu)) * x ** nu * O.bessel_k(nu, x)
        assert abs(got - ref) <= 1e-12 * ref, (nu, x, got, float(ref))


def test_integer_order_series_matches_mpmath():
    """The quick K_n of highprec (integer n) against mpmath.besselk's limit"""
    mp = H._MP
    for n in (0, 1, 2, 3, 10):
        for x in ("1e-12", "0.001", "0.75", "1.5", "9.25", "31", "60"):
            a, b = H._besselk_int(n, mp.mpf(x)), mp.besselk(n, mp.mpf(x))
            assert abs(a - b) <= mp.mpf(10) ** -37 * b, (n, x)


def test_closed_forms():
    """nu = 1/2 and 3/2 of the general Matern are the exponential and the
    Matern 3/2; distance 0 gives 1."""
    mp = H._MP
    for x in (1e-9, 0.5, 1.5, 20.0, 700.0):
        e = H.corr_mp("exponential_isotropic", None, x)
        assert abs(H.corr_mp("matern_isotropic", 0.5, x) - e) <= mp.mpf(10) ** -37 * e
        m = H.corr_mp("matern15_isotropic", None, x)
        assert abs(H.corr_mp("matern_isotropic", 1.5, x) - m) <= mp.mpf(10) ** -37 * m
    for cf in ("exponential_isotropic", "matern15_isotropic", "matern_isotropic"):
        assert H.corr_mp(cf, 0.7, 0.0) == 1


# every family at d = 1..4 (the spacetime covariances need d >= 2)
@pytest.mark.parametrize("covfun,d", [(c, d) for c in CASES for d in (1, 2, 3, 4)
                                      if d >= 2 or not c.endswith("spacetime")])
def test_references_agree(P, O, covfun, d):
    cp = CASES[covfun](d)
    locs, NN, _, _, _ = H.dyadic_problem(P, 60, 9, d, seed=10 * d + 1)
    ref = H.vecchia_linv_hp(covfun, cp, locs, NN)
    _assert_rows_close(O, covfun, cp, locs, NN, O.vecchia_linv(covfun, cp, locs, NN), ref.astype(np.float64))
    assert np.all(ref[NN == O.NA] == 0)
    sub = locs[:24]
    Ch, Co = H.covmat_hp(covfun, cp, sub), O.covmat(covfun, cp, sub)
    tol = 1e-12 if H.FAMILY[covfun] == 2 else 1e-14
    assert np.all(np.abs(Co - Ch) <= tol * np.abs(Ch)), float(np.max(np.abs(Co - Ch) / np.abs(Ch)))


def test_short_rows_and_failing_row(O):
    """NA entries inside the array (a one-neighbour chain stored with 4
    columns) are short rows; a non-PD block is reported by its 1-based row,
    the first one, as the oracle does on the same blocks."""
    n = 40
    NN = np.full((n, 4), O.NA, np.int32)
    NN[:, 0] = np.arange(1, n + 1)
    NN[1:, 1] = np.arange(1, n)
    x = np.cumsum(np.full(n, 0.5))
    x[[17, 29]] = x[[16, 28]]
    locs = np.column_stack([x, np.zeros(n)])
    good = H.vecchia_linv_hp("exponential_isotropic", [1.0, 1.0, 0.1], locs, NN)
    want = O.vecchia_linv("exponential_isotropic", [1.0, 1.0, 0.1], locs, NN[:, :2])
    np.testing.assert_allclose(good[:, :2].astype(np.float64), want, rtol=1e-13)
    assert np.all(good[:, 2:] == 0)
    for ref in (lambda nn: H.vecchia_linv_hp("exponential_isotropic", [1.0, 1.0, -1e-3], locs, nn),
                lambda nn: O.vecchia_linv("exponential_isotropic", [1.0, 1.0, -1e-3], locs, nn[:, :2])):
        with pytest.raises(np.linalg.LinAlgError, match="row 18$"):
            ref(NN)


@pytest.mark.parametrize("n,m", [(500, 6), (5, 10)])
def test_sparse_B_times_equals_dense_B(P, O, n, m):
    """B x and |B| |x| straight from (Linv, NN) against the oracle's dense B in
    long double, a vector and a 3-column matrix; at n = 5, m = 10 the NNarray
    keeps its m + 1 = 11 columns, so every row is short.  NA entries of Linv
    hold a nonzero value here: both sides must mask them by NN, not by value.
    Bound: either side sums at most b products per entry in long double, in its
    own order: 2 b 2^-64 x the sum of the absolute values of the products."""
    from conftest import make_problem

    locs, NN, _, _, _ = make_problem(P, n, m, seed=4)
    NN = H.pad_na(NN, m + 1)
    assert NN.shape == (n, m + 1) and (n > m or np.all((NN == O.NA).any(axis=1)))
    linv = H.vecchia_linv_hp("exponential_isotropic", [1.2, 0.07, 0.05], locs, NN).astype(np.float64)
    linv[NN == O.NA] = 7.0
    rng = np.random.default_rng(n)
    B = O.dense_B(linv, NN).astype(H.LD)
    for x in (rng.normal(size=n), rng.normal(size=(n, 3))):
        got, got_abs = H.sparse_B_times(linv, NN, x)
        want, want_abs = B @ x.astype(H.LD), np.abs(B) @ np.abs(x).astype(H.LD)
        assert got.shape == x.shape and got.dtype == H.LD
        bound = 2 * (m + 1) * H.LD(2.0) ** -64 * want_abs
        assert np.all(want_abs > 0)
        assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))
        assert np.all(np.abs(got_abs - want_abs) <= bound)
    # x_abs given: |B| x_abs
    xa = np.abs(rng.normal(size=n)) + 1.0
    _, got_abs = H.sparse_B_times(linv, NN, rng.normal(size=n), xa)
    assert np.all(np.abs(got_abs - np.abs(B) @ xa.astype(H.LD)) <= 2 * (m + 1) * H.LD(2.0) ** -64 * got_abs)
