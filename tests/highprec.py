"""High-precision references for the Vecchia factor (plain helpers, no
fixtures): the correlation functions with mpmath at 40 digits and
GpGp::vecchia_Linv in np.longdouble (x87 extended, 64-bit significand).

The C oracle (oracle/nngp_oracle.c) is plain fp64 like the device, so a
comparison with it cannot resolve errors below ~1e-13 of a row.  These
references can: tests/test_highprec_reference.py checks them and the oracle
against each other on the CPU, and the GPU modules
(test_gpu_covariance_accuracy.py, test_gpu_factor_matrix.py) then judge the
device against them.

Only numpy and mpmath (which torch's sympy dependency brings) are used.
"""
import mpmath
import numpy as np

LD = np.longdouble
# a platform whose long double is the 53-bit double gives no reference at all
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not extended precision here: no high-precision reference"

NA = -(2 ** 31)
_MP = mpmath.mp.clone()
_MP.dps = 40

FAMILY = {"exponential_isotropic": 0, "exponential_scaledim": 0, "exponential_spacetime": 0,
          "matern15_isotropic": 1,
          "matern_isotropic": 2, "matern_scaledim": 2, "matern_spacetime": 2}


def _besselk_int(n, x):
    """K_n(x), integer n >= 0, 0 < x <= 60, from the ascending series of K_0
    and K_1 (Abramowitz & Stegun 9.6.13, 9.6.11) and the upward recurrence:
    mpmath.besselk takes integer orders as a limit, ~100 times slower.  The
    series cancel from e^x down to e^-x, so they run with 2 x / ln 10 extra
    digits.  tests/test_highprec_reference.py holds it to mpmath.besselk."""
    prec = _MP.prec
    try:
        _MP.prec = prec + int(2.9 * float(x)) + 30
        x = +x
        y, lg = x * x / 4, _MP.log(x / 2)
        c = _MP.mpf(1)                       # (x^2/4)^k / (k!)^2
        h = _MP.mpf(0)                       # H_k
        i0 = s0 = i1 = s1 = _MP.mpf(0)
        k = 0
        while True:
            c1 = c / (k + 1)                 # (x^2/4)^k / (k! (k+1)!)
            i0 += c
            s0 += c * h
            i1 += c1
            s1 += c1 * (2 * h + _MP.mpf(1) / (k + 1) - 2 * _MP.euler)
            if k > 5 and c * (h + 3) < _MP.eps * _MP.mpf(2) ** (-int(2.9 * float(x))) * 1e-3:
                break
            k += 1
            h += _MP.mpf(1) / k
            c = c * y / (k * k)
        k0 = -(lg + _MP.euler) * i0 + s0
        k1 = 1 / x + lg * (x / 2) * i1 - (x / 4) * s1
        for j in range(1, n):
            k0, k1 = k1, k0 + 2 * j / x * k1
        out = k0 if n == 0 else k1
    finally:
        _MP.prec = prec
    return +out


def _besselk(v, d):
    if v == int(v) and d <= 60:
        return _besselk_int(int(v), d)
    return _MP.besselk(v, d)


def corr_mp(covfun, nu, dist):
    """Correlation at unit-range distance `dist` (a float, taken exactly, or
    an mpf), as a 40-digit mpf: exp(-d), (1 + d) exp(-d), or
    2^(1-nu) / Gamma(nu) d^nu K_nu(d) with `nu` taken exactly; 1 at d == 0."""
    fam = FAMILY[covfun]
    d = dist if isinstance(dist, _MP.mpf) else _MP.mpf(float(dist))
    if d == 0:
        return _MP.mpf(1)
    if fam == 0:
        return _MP.exp(-d)
    if fam == 1:
        return (1 + d) * _MP.exp(-d)
    v = _MP.mpf(float(nu))
    return _MP.power(2, 1 - v) / _MP.gamma(v) * _MP.power(d, v) * _besselk(v, d)


def mp_to_ld(v):
    """mpf -> np.longdouble (through 25 decimal digits: below 2^-64 relative)"""
    return LD(_MP.nstr(v, 25, min_fixed=0, max_fixed=0))


_memo = {}  # (family, nu, distance hi, lo) -> longdouble correlation


def corr_ld(covfun, nu, dists):
    """corr_mp of every entry of `dists` (float64 or longdouble array; every
    value is taken exactly), rounded to longdouble; equal distances are
    evaluated once."""
    dists = np.asarray(dists)
    u, inv = np.unique(dists.reshape(-1), return_inverse=True)
    out = np.empty(len(u), LD)
    for k, x in enumerate(u):
        # a longdouble distance goes to mpmath as hi + lo doubles (exact)
        hi = float(x)
        lo = float(LD(x) - LD(hi))
        key = (FAMILY[covfun], nu, hi, lo)
        if key not in _memo:
            _memo[key] = mp_to_ld(corr_mp(covfun, nu, _MP.mpf(hi) + _MP.mpf(lo)))
        out[k] = _memo[key]
    return out[inv].reshape(dists.shape)


def covparms_split(covfun, cp, d):
    """-> (variance, per-axis ranges (d,), nu or None, nugget) of a GpGp
    covparms vector for d-dimensional locations."""
    cp = [float(x) for x in cp]
    fam = FAMILY[covfun]
    kind = covfun.split("_")[1]
    if kind == "isotropic":
        ranges, k = [cp[1]] * d, 2
    elif kind == "scaledim":
        ranges, k = cp[1:1 + d], 1 + d
    elif kind == "spacetime":
        assert d >= 2
        ranges, k = [cp[1]] * (d - 1) + [cp[2]], 3
    else:
        raise ValueError(f"no high-precision reference for {covfun}")
    nu = cp[k] if fam == 2 else None
    assert len(cp) == k + (2 if fam == 2 else 1), (covfun, cp, d)
    return cp[0], np.array(ranges, LD), nu, cp[-1]


def _corr_of_dist(covfun, nu, dist):
    fam = FAMILY[covfun]
    if fam == 0:
        return np.exp(-dist)
    if fam == 1:
        return (1 + dist) * np.exp(-dist)
    return corr_ld(covfun, nu, dist)


def covmat_hp(covfun, cp, locs):
    """Dense covariance of `locs` (k x d) in longdouble: var (corr + nugget I)"""
    locs = np.asarray(locs, np.float64)
    if locs.ndim == 1:
        locs = locs[:, None]
    var, ranges, nu, nug = covparms_split(covfun, cp, locs.shape[1])
    sc = locs.astype(LD) / ranges
    diff = sc[:, None, :] - sc[None, :, :]
    dist = np.sqrt((diff * diff).sum(axis=-1))
    return LD(var) * (_corr_of_dist(covfun, nu, dist) + LD(nug) * np.eye(len(locs), dtype=LD))


def vecchia_linv_hp(covfun, cp, locs, NN):
    """GpGp::vecchia_Linv in longdouble: row i of the result is the last row
    of the inverse Cholesky factor of the covariance of locs[rev(NN[i, :bs])]
    (the point itself last), reversed; bs = the row's count of non-NA entries
    (they lead the row); entries beyond bs are 0.  Coordinate scaling,
    distances, correlations, Cholesky and back substitution all run in
    longdouble, vectorised over the rows of equal bs; the general Matern's
    correlations come from corr_mp.  Raises LinAlgError naming the first row
    (1-based) whose local covariance is not positive definite."""
    locs = np.asarray(locs, np.float64)
    if locs.ndim == 1:
        locs = locs[:, None]
    NN = np.asarray(NN)
    n, b = NN.shape
    var, ranges, nu, nug = covparms_split(covfun, cp, locs.shape[1])
    sc = locs.astype(LD) / ranges
    valid = NN != NA
    bsz = valid.sum(axis=1)
    assert all(valid[i, :bsz[i]].all() for i in range(n)), "NA entries must trail each row"
    out = np.zeros((n, b), LD)
    fail = []
    for bs in np.unique(bsz):
        rows = np.nonzero(bsz == bs)[0]
        idx = NN[rows, :bs][:, ::-1] - 1                       # locsub order: self last
        X = sc[idx]                                            # R x bs x d
        diff = X[:, :, None, :] - X[:, None, :, :]
        dist = np.sqrt((diff * diff).sum(axis=-1))             # R x bs x bs
        C = LD(var) * (_corr_of_dist(covfun, nu, dist) + LD(nug) * np.eye(bs, dtype=LD))
        L = np.zeros_like(C)
        bad = np.zeros(len(rows), bool)
        for j in range(bs):
            s = C[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(axis=1)
            bad |= ~(s > 0)
            s = np.where(s > 0, s, LD(1))
            L[:, j, j] = np.sqrt(s)
            if j + 1 < bs:
                t = C[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, None, j, :j]).sum(axis=2)
                L[:, j + 1:, j] = t / L[:, j, j][:, None]
        fail.extend(rows[bad].tolist())
        x = np.zeros((len(rows), bs), LD)                      # L^T x = e_last
        for r in range(bs - 1, -1, -1):
            s = (LD(1) if r == bs - 1 else LD(0)) - (L[:, r + 1:, r] * x[:, r + 1:]).sum(axis=1)
            x[:, r] = s / L[:, r, r]
        out[rows, :bs] = x[:, ::-1]
    if fail:
        raise np.linalg.LinAlgError(f"local covariance not positive definite at row {min(fail) + 1}")
    return out


def pad_na(NN, b):
    """NN with trailing all-NA columns up to b columns (find_ordered_nn stores
    min(m, n - 1) + 1 columns; GpGp keeps m + 1, the rest NA)"""
    NN = np.asarray(NN, np.int32)
    return np.column_stack([NN, np.full((NN.shape[0], max(0, b - NN.shape[1])), NA, np.int32)])


def sparse_B_times(Linv, NN, x, x_abs=None):
    """(B x, |B| x_abs) in longdouble for the sparse factor B[i, NN[i, g] - 1] =
    Linv[i, g] (NN 1-based with NA entries, as the oracle's dense_B reads it),
    without forming the n x n matrix: one vectorised pass per neighbour column
    g, NA entries masked out.  x is a vector (n,) or a matrix (n, k); x_abs
    defaults to |x| (pass the sum of absolute values where x is itself a sum).
    tests/test_highprec_reference.py holds it to dense_B."""
    Linv, NN = np.asarray(Linv).astype(LD), np.asarray(NN)
    x = np.asarray(x).astype(LD)
    x_abs = np.abs(x) if x_abs is None else np.asarray(x_abs).astype(LD)
    n, b = NN.shape
    assert Linv.shape == (n, b) and x.shape[0] == n and x_abs.shape == x.shape
    tail = (1,) * (x.ndim - 1)
    out, out_abs = np.zeros(x.shape, LD), np.zeros(x.shape, LD)
    for g in range(b):
        ok = NN[:, g] != NA
        idx = np.where(ok, NN[:, g], 1).astype(np.int64) - 1
        assert idx.min() >= 0 and idx.max() < n
        l = np.where(ok, Linv[:, g], LD(0)).reshape((n,) + tail)
        out += l * x[idx]
        out_abs += np.abs(l) * x_abs[idx]
    return out, out_abs


def row_conds(O, covfun, cp, locs, NN):
    """cond(C_i) of every row's local covariance, from the oracle's double
    covariance (as test_gpu_parity._assert_rows_close takes it)"""
    out = np.ones(NN.shape[0])
    for i in range(NN.shape[0]):
        idx = NN[i][NN[i] != NA] - 1
        if len(idx) > 1:
            out[i] = np.linalg.cond(O.covmat(covfun, cp, locs[idx]))
    return out


def row_errors(got, ref, kappa, eps=1e-14):
    """Per row: (max |got - ref|, the bound max(1e-10, eps cond(C_i)) max|ref row|
    of _assert_rows_close, err / (eps cond(C_i) max|ref row|))"""
    top = np.abs(ref).max(axis=1).astype(np.float64)
    err = np.abs(np.asarray(got, LD) - ref).max(axis=1).astype(np.float64)
    return err, np.maximum(1e-10, eps * kappa) * top, err / (eps * kappa * top)


def dyadic_problem(P, n, m, d, seed):
    """n distinct locations on the dyadic grid (integers / 4096)^d, max-min
    ordered, with their m nearest earlier neighbours and a greedy colouring:
    with power-of-two ranges the scaled coordinates and their differences are
    exact in fp64, so device, oracle and this module see the same distances
    up to the rounding of the sum of squares."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(4096 ** min(d, 2), n, replace=False)   # distinct in the first one or two axes
    cols = [cells % 4096] + ([cells // 4096] if d >= 2 else []) + [rng.integers(0, 4096, n) for _ in range(d - 2)]
    locs = np.column_stack(cols).astype(np.float64) / 4096.0
    locs = locs[P.order_maxmin(locs) - 1]
    NN = P.find_ordered_nn(locs, m)
    col = P.naive_greedy_coloring(NN)
    return locs, NN, col, np.arange(1, n + 1, dtype=np.int32), rng.normal(size=n)
