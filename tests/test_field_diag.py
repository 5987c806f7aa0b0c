"""CPU checks of the per-location field diagnostics: the shared header
csrc/field_diag.h compiled for the host (plain, and once with the address and
undefined sanitizers as a stand-alone program), the numpy backend of
field_diagnostics against diagnose._ess_1d, Gelman_Rubin_Brooks and the
long-double reference tests/field_diag_ref.py, and the Python entry points'
behaviour without a GPU.

Bound on ess (eps = 2^-52; tests/cpp/field_diag_check.cpp derives it):
8 (S + P) eps / min(1, d^2) relative, d = 1 - sum phi at the selected order.
It is an a-priori bound: the stand-alone program uses at most 0.15 of it (it
prints the fraction), and for rho = 0.99 (d about 0.01 to 0.03) it lies 1e3
to 1e4 times above the errors seen, about 3e-13.  The tight check of the
strongly correlated columns is the GPU module's (8 x the host backend's own
error against the long-double reference)."""
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import field_diag_ref as R  # noqa: E402

EPS = 2.0 ** -52


def _build_and_run(tmp_path, name, extra):
    exe = tmp_path / name
    inc = next(ROOT.glob("*_amd")) / "csrc"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", *extra, f"-I{inc}",
                    str(ROOT / "tests" / "cpp" / "field_diag_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    print(r.stdout)


def test_field_diag_header_matches_long_double(tmp_path):
    """field_diag_ess / field_diag_combine built for the host with hipcc: order
    and ess against the long double restatement for S in {4, 5, 37, 300, 1000}
    x rho in {0, .5, .9, .99}, the crafted acf arrays, the combination's
    special values and the largest order for S up to 9999."""
    _build_and_run(tmp_path, "field_diag_check", ["-O2"])


def test_field_diag_header_under_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined on the
    host code: every phi / acf index stays inside its array."""
    _build_and_run(tmp_path, "field_diag_check_san", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined"])


@pytest.fixture(scope="module")
def case300():
    blocks = R.ar1_blocks(300, 50, 3, seed=300)
    return SimpleNamespace(blocks=blocks, ref=R.field_diag_ld(blocks))


def _ess_bound(S, d):
    P = min(S - 1, int(10 * np.log10(S))) if S >= 4 else 0
    return 8 * (S + P) * EPS / np.minimum(1.0, d * d)


def test_host_backend_is_ess_1d_per_column(P, case300):
    """One chain at a time the host backend's ess column is _ess_1d of every
    column (both within the bound of the long-double value, so within twice
    the bound of each other), and its order is the reference's."""
    from nngp_amd import diagnose as D

    assert np.all(case300.ref["aic_gap"] >= 1e-6)
    for k, b in enumerate(case300.blocks):
        got, order = P.field_diagnostics([b], return_order=True)
        want = np.array([D._ess_1d(b[:, j]) for j in range(b.shape[1])])
        bound = _ess_bound(300, case300.ref["d"][k])
        ref = case300.ref["ess_k"][k].astype(np.float64)
        assert np.all(np.abs(got[:, 1] - want) <= 2 * bound * ref)
        assert np.all(np.abs(got[:, 1] - ref) <= bound * ref)
        np.testing.assert_array_equal(got[:, 1], got[:, 2])
        np.testing.assert_array_equal(order[0], case300.ref["order"][k])
        assert np.all(np.isnan(got[:, 0])) and np.all(np.isnan(got[:, 4]))  # one chain: no Bv


def test_host_backend_against_reference(P, case300):
    got, order = P.field_diagnostics(case300.blocks, return_order=True)
    ref = case300.ref["out"].astype(np.float64)
    np.testing.assert_array_equal(order, case300.ref["order"])
    bound = sum(_ess_bound(300, d) * e.astype(np.float64) for d, e in zip(case300.ref["d"], case300.ref["ess_k"]))
    assert np.all(np.abs(got[:, 1] - ref[:, 1]) <= bound)
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=304 * EPS, atol=0)
    np.testing.assert_allclose(got[:, [0, 4]], ref[:, [0, 4]], rtol=1e-9, atol=0)
    assert np.median(got[::3, 0]) > 1.5 > np.median(got[1::3, 0])  # the shifted columns stand out


def test_host_r_hat_is_gelman_rubin_brooks(P, case300):
    """A 3-column "field" passed as the hyperparameters with n = S: the
    individual PSRFs of Gelman_Rubin_Brooks (the same formula through np.cov)."""
    S = 300
    recs = {str(k): {"params": {"f": b[:, :3]}} for k, b in enumerate(case300.blocks)}
    g = P.Gelman_Rubin_Brooks(recs, burn_in=0.0, n=S)
    got = P.field_diagnostics([b[:, :3] for b in case300.blocks])
    np.testing.assert_allclose(got[:, 0], g["R_hat"][1:], rtol=4 * (S + 4) * EPS, atol=0)
    np.testing.assert_allclose(got[:, 3], np.diag(g["within_variance"]), rtol=(S + 4) * EPS, atol=0)


def test_host_offsets_blocks_and_specials(P):
    rng = np.random.default_rng(5)
    S, n, m = 37, 20, 2
    blocks = R.ar1_blocks(S, n, m, seed=37)
    off = rng.normal(size=m * S)
    centred = [b - off[k * S:(k + 1) * S, None] for k, b in enumerate(blocks)]
    a, oa = P.field_diagnostics(blocks, row_offset=off, return_order=True)
    b, ob = P.field_diagnostics(centred, return_order=True)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(oa, ob)
    sp = [x.copy() for x in centred]
    for k in range(m):
        sp[k][:, 0] = 0.5          # constant everywhere
        sp[k][:, 1] = 1.0 + k      # constant per chain
    sp[1][7, 2] = np.nan
    got, order = P.field_diagnostics(sp, return_order=True)
    assert np.isnan(got[0, 0]) and got[0, 1] == m * S and got[0, 2] == S and got[0, 3] == 0 and got[0, 4] == 0
    assert np.isinf(got[1, 0]) and got[1, 3] == 0 and got[1, 4] == 0.5
    assert np.all(np.isnan(got[2])) and np.all(order[:, :3] == 0)
    np.testing.assert_array_equal(got[3:], b[3:])
    short = P.field_diagnostics([x[:3] for x in centred])  # S < 4: no fit
    np.testing.assert_array_equal(short[:, 1], np.full(n, 6.0))
    with pytest.raises(ValueError):
        P.field_diagnostics(blocks, backend="cuda")
    with pytest.raises(ValueError):
        P.field_diagnostics(blocks, row_offset=off[:-1])


def test_field_diagnostics_of_a_run_list(P):
    """Field_diagnostics selects the rows mcmc_nngp_estimate selects for
    res["field"] and centres them by beta_0 of the saved iterations."""
    rng = np.random.default_rng(9)
    n, it = 30, 40
    saved = np.arange(2, it + 1, 2, dtype=float)  # field_thinning = .5
    recs = {}
    for k in range(3):
        recs[f"chain_{k + 1}"] = {"iterations": np.array([[0, 0.0], [it, 1.0]]), "saved_field": saved,
                                  "params": {"beta_0": rng.normal(size=(it, 1)),
                                             "field": R.ar1_blocks(len(saved), n, 1, seed=k, shift=False)[0]}}
    L = {"records": recs}
    got = P.Field_diagnostics(L, burn_in=0.5)
    sel = saved > it * 0.5
    blocks = [c["params"]["field"][sel] - c["params"]["beta_0"][saved[sel].astype(int) - 1] for c in recs.values()]
    want = P.field_diagnostics(blocks)
    for j, nm in enumerate(["R_hat", "ess", "ess_min", "W", "Bv"]):
        np.testing.assert_array_equal(got[nm], want[:, j])
    d = got["digest"]
    assert d["R_hat_max"] == want[:, 0].max() and want[d["R_hat_argmax"], 0] == d["R_hat_max"]
    assert d["ess_min"] == want[:, 1].min() and d["ess_median"] == np.median(want[:, 1])
    assert d["share_R_hat_above_1.1"] == np.mean(want[:, 0] > 1.1) and d["n_locations"] == d["n_finite_R_hat"] == n
    # a constant column has no finite R_hat: it leaves the quantiles' and the share's denominator alike
    w2 = want.copy()
    w2[:10, 0] = np.nan
    w2[10, 0] = np.inf
    from nngp_amd import diagnose as D
    d2 = D.field_digest(w2)
    assert d2["n_finite_R_hat"] == n - 11 and d2["share_R_hat_above_1.1"] == np.mean(want[11:, 0] > 1.1)
    assert d2["R_hat_q0.5"] == np.quantile(want[11:, 0], 0.5) and d2["R_hat_max"] == np.inf
    np.testing.assert_array_equal([d["R_hat_q0.5"], d["R_hat_q0.9"], d["R_hat_q0.99"]],
                                  np.quantile(want[:, 0], [0.5, 0.9, 0.99]))
    with pytest.raises(ValueError):
        P.mcmc_nngp_run(L, field_diagnostics="cuda")


def test_hip_backend_argument_errors_and_no_gpu(P):
    """NNGP_ERR_ARG is decided before any HIP call, so it is the answer with
    or without a device; a valid call without a device is NNGP_ERR_NODEV, never
    a host fallback."""
    from nngp_amd import _lib

    x = np.zeros((5, 4))
    for blocks, kw in (([x[:1]], {}), ([np.zeros((10000, 1))], {}), ([x] * 17, {}), ([np.zeros((5, 0))], {}),
                       ([x], {"chunk_cols": -1})):
        with pytest.raises(P.NNGPError) as e:
            P.field_diagnostics(blocks, backend="hip", **kw)
        assert e.value.status == 1
    import ctypes as C
    out = np.zeros((5, 4))
    assert P.lib.nngp_field_diag(0, (C.c_void_p * 1)(None), 1, 5, 4, None, 0, out, None) == 1  # a null block
    seen = P.lib.nngp_device_normals(0, 1, 0, 1, np.zeros(1))
    if seen == _lib.NNGP_OK:
        pytest.skip("GPU present")
    assert seen == _lib.NNGP_ERR_NODEV, seen
    with pytest.raises(P.NNGPError) as e:
        P.field_diagnostics([np.random.default_rng(0).normal(size=(7, 5))], backend="hip")
    assert e.value.status == 6
