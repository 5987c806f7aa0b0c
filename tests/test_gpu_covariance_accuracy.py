"""The device's correlation functions against mpmath at 40 digits (needs an
MI355X): exp_nonpos, sqrt_pos and bessel_k of kernels.hip, read back through
a two-point Vecchia factor.

For a row with one neighbour, variance 1 and nugget t the local block is
[[1 + t, r], [r, 1 + t]], and -Linv[i, 1] / Linv[i, 0] = r / (1 + t) whatever
the pivot sqrt(1 + t - r^2 / (1 + t)) rounds to (it cancels): with t = 0 the
quotient is the correlation the kernel computed, times three roundings
(r * inv0, (L10 x1) * inv0, the division here, done in long double).

Graph: a chain with m = 1 (row i has neighbour i - 1), NNarray built by hand.
Coordinates: d = 2, even points at (0, 0), odd point i at (g, 0), range 1:
every distance is exactly the double g (sqrt(fl(g^2)) == g for a correctly
rounded sqrt, which is what sqrt_pos claims), seen once as g - 0 and once as
0 - g.  The reference is corr_mp at the same double.

Nugget.  At nugget 0 a block whose correlation rounds to 1 is singular and
the factor call fails as a whole (Matern 3/2 below a gap of ~1e-8, the
smoother general Materns further up).  The gaps whose reference correlation
exceeds 1 - 2^-40 therefore run in a second context with nugget 2^-10 (1 + t
exact), and the read-back is multiplied by 1 + t in long double; inv0 =
1/sqrt(1 + t) then enters twice, two more roundings.  Every other gap runs at
nugget 0.

Bounds, relative to corr_mp, for gaps <= 700 whose correlation is >= 1e-300:
  exponential, Matern 3/2 ... 16 * 2^-53: exp_nonpos claims 1 ulp, sqrt_pos
      correct rounding, Matern 3/2 adds one fma, the read-back at most 6
      roundings
  general Matern ............ 3e-14: 1e-14 is the stated bound of bessel_k,
      about 1e-14 goes to norm * pow (lgamma's argument reaches 12.8 at
      nu = 10 and its ulps are amplified by exp), the rest is the read-back.
Gaps beyond 708 (exp(-g) subnormal or 0): finite, >= 0, non-increasing in the
gap and at most 1e-300 -- at most max(1e-300, 2 x reference) for the general
Matern, whose g^nu factor keeps the true correlation above 1e-300 up to
g ~ 730 at nu = 10 while K_mu itself is already subnormal; the exponential at
gap 800 is exactly 0.

Each case prints "[covariance] <family>: worst <fraction of the bound> at gap
<g>" (pytest -s).  Measured on the MI355X, as fractions of the bounds:
exponential 0.12, Matern 3/2 0.15 (the lane-group kernel the same), general
Matern 0.52 at nu = 0.05 (gap 1.5), 0.25 at nu = 1.051, 0.18 at nu = 0.95, at
most 0.09 at every other nu; nu = 1/2 and 3/2 against the closed forms 0.05.
With the sign of the mu^2 coefficient of temme_g1g2's Taylor branch flipped,
nu = 0.96, 1.04 and 1.049 fail and nothing else does (integer nu has mu = 0).
"""
import numpy as np
import pytest

import highprec as H

pytestmark = pytest.mark.gpu

LD = np.longdouble
TAU = 2.0 ** -10
ULP16 = 16 * 2.0 ** -53
BOUND = {0: ULP16, 1: ULP16, 2: 3e-14}
NUS = [0.05, 0.25, 0.45, 0.4999, 0.5, 0.5001, 0.54, 0.55, 0.56, 0.95, 0.96, 1.0, 1.04, 1.049, 1.051, 1.5, 2.0, 2.5,
       3.0, 3.5, 5.0, 7.5, 10.0]
LN2_64 = 0.010830424696249145  # ln2 / 64, exp_nonpos's reduction step


def _around(x):
    return [np.nextafter(x, 0.0), x, np.nextafter(x, 1e9)]


def _body_gaps():
    g = list(np.geomspace(1e-12, 700.0, 520))
    g += _around(1.5) + [1.4999, 1.5000001]                       # series | Miller recurrence
    for k in (88, 87, 40, 10, 2, 1):                              # N = min(100, 12 + int(160 / x)) steps
        g += _around(160.0 / k)
    g += [1.818, 1.819]
    for k in (0, 1, 2, 5, 31, 63, 64, 100, 1000, 5000, 20000, 40000, 64000):
        g += _around((k + 0.5) * LN2_64)                          # rint half-way points of exp_nonpos
    return np.array(sorted(set(float(x) for x in g)))


BODY = _body_gaps()
TAIL = np.array([708.39, 708.4, 708.5, 709.0, 710.0, 720.0, 730.0, 740.0, 744.0, 744.5, 745.0, 745.13, 745.14,
                 745.2, 746.0, 750.0, 800.0, 1000.0])
GAPS = np.concatenate([BODY, TAIL])
assert 550 <= len(GAPS) <= 650 and np.all(np.diff(GAPS) > 0)

_cache = {}


def _reference(covfun, nu):
    key = ("ref", H.FAMILY[covfun], nu if H.FAMILY[covfun] == 2 else None)
    if key not in _cache:
        _cache[key] = H.corr_ld(covfun, nu, GAPS)
    return _cache[key]


def _chain(P, gaps):
    """-> (locs, NN, colouring, locs_match, y) of the zig-zag chain; rows
    2k + 1 and 2k + 2 both see gaps[k]"""
    n = 2 * len(gaps) + 1
    locs = np.zeros((n, 2))
    locs[1::2, 0] = gaps
    NN = np.full((n, 2), H.NA, np.int32)
    NN[:, 0] = np.arange(1, n + 1)
    NN[1:, 1] = np.arange(1, n)
    return locs, NN, P.naive_greedy_coloring(NN), np.arange(1, n + 1, dtype=np.int32), np.zeros(n)


def _read_back(P, covfun, nu, gaps, nugget):
    cp = [1.0, 1.0, nugget] if H.FAMILY[covfun] != 2 else [1.0, 1.0, nu, nugget]
    with P.ChainContext(*_chain(P, gaps), device=0) as ctx:
        ctx.factor(0, covfun, cp)
        L = ctx.get_linv(0)
    assert np.all(np.isfinite(L)) and np.all(L[1:, 0] > 0)
    r = -(L[1:, 1].astype(LD) / L[1:, 0].astype(LD)) * (LD(1) + LD(nugget))
    return r.reshape(len(gaps), 2)


def _device_corr(P, covfun, nu, lanes, monkeypatch):
    """The device's correlation at every gap of GAPS, read from both rows"""
    key = ("dev", covfun, nu if H.FAMILY[covfun] == 2 else None, lanes)
    if key not in _cache:
        if lanes:
            monkeypatch.setenv("NNGP_FACTOR_LANES", "16")
        else:
            monkeypatch.delenv("NNGP_FACTOR_LANES", raising=False)
        monkeypatch.delenv("NNGP_FACTOR_PAIR", raising=False)
        ref = _reference(covfun, nu)
        near1 = ref > LD(1) - LD(2.0 ** -40)
        out = np.zeros((len(GAPS), 2), LD)
        out[~near1] = _read_back(P, covfun, nu, GAPS[~near1], 0.0)
        if near1.any():
            out[near1] = _read_back(P, covfun, nu, GAPS[near1], TAU)
        _cache[key] = out
    return _cache[key]


def _check(label, fam, got, ref):
    body = np.arange(len(GAPS)) < len(BODY)
    judged = body & (ref >= 1e-300)
    rel = np.abs(got - ref[:, None]).max(axis=1) / ref
    worst = int(np.argmax(np.where(judged, rel, 0)))
    print(f"\n[covariance] {label}: worst {float(rel[worst] / BOUND[fam]):.3g} of the bound {BOUND[fam]:.3g} "
          f"at gap {GAPS[worst]!r} ({int(judged.sum())} gaps judged)")
    assert judged.sum() > 400
    over = np.nonzero(judged & ~(rel <= BOUND[fam]))[0]
    assert len(over) == 0, [(GAPS[k], float(rel[k])) for k in over[:10]]
    for side in (0, 1):
        t = got[~body, side]
        cap = np.maximum(LD(1e-300), 2 * ref[~body]) if fam == 2 else LD(1e-300)
        assert np.all(np.isfinite(t)) and np.all(t >= 0) and np.all(t <= cap), t
        assert np.all(np.diff(t) <= 0), t


@pytest.mark.parametrize("lanes", [False, True], ids=["default", "lanes16"])
@pytest.mark.parametrize("covfun", ["exponential_isotropic", "matern15_isotropic"])
def test_exponential_and_matern15(P, monkeypatch, covfun, lanes):
    """exp_nonpos and sqrt_pos through factor_kernel<8, FAM, 2> and, under
    NNGP_FACTOR_LANES=16, factor_lanes_kernel."""
    got = _device_corr(P, covfun, None, lanes, monkeypatch)
    _check(f"{covfun}{' lanes16' if lanes else ''}", H.FAMILY[covfun], got, _reference(covfun, None))
    if covfun == "exponential_isotropic":
        assert np.all(got[GAPS == 800.0] == 0)


@pytest.mark.parametrize("nu", NUS)
def test_general_matern(P, monkeypatch, nu):
    """norm * pow * bessel_k through factor_kernel_rt<2, 2>: the Taylor branch
    of temme_g1g2 (|mu| < 0.05: nu = 0.96, 1.0, 1.04, 1.049, 2.0, 3.0, 5.0,
    10.0), its other branch right next to it (0.95, 1.051), the pm == 0 /
    sg == 0 guards (integer nu; sg == 0 also at gap 2), mu = +-1/2 (0.5, 1.5,
    2.5, 3.5, 7.5) and its neighbours, and the upward recurrence to nu = 10."""
    got = _device_corr(P, "matern_isotropic", nu, False, monkeypatch)
    _check(f"matern_isotropic nu={nu}", 2, got, _reference("matern_isotropic", nu))


@pytest.mark.parametrize("nu,covfun", [(0.5, "exponential_isotropic"), (1.5, "matern15_isotropic")])
def test_general_matern_agrees_with_closed_forms(P, monkeypatch, nu, covfun):
    """matern_isotropic at nu = 1/2, 3/2 against the device's own exponential
    and Matern 3/2, within the sum of the two bounds."""
    a = _device_corr(P, "matern_isotropic", nu, False, monkeypatch)
    b = _device_corr(P, covfun, None, False, monkeypatch)
    ref = _reference(covfun, None)
    judged = (np.arange(len(GAPS)) < len(BODY)) & (ref >= 1e-300)
    rel = np.abs(a - b).max(axis=1) / ref
    print(f"\n[covariance] matern_isotropic nu={nu} vs {covfun}: worst {float(rel[judged].max()):.3g} "
          f"(bound {ULP16 + 3e-14:.3g})")
    assert np.all(rel[judged] <= ULP16 + 3e-14)
