"""CPU checks of the widened summaries (chosen quantiles and exceedance
probabilities, nngp_summary_probs): the general column routine of
csrc/summary_select.h compiled for the host, plain and under the address and
undefined-behaviour sanitizers (a stand-alone program), and the Python entry
points on the host backend against numpy."""
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = "/opt/rocm/bin/hipcc"
PROBS = (0.9, 0.0, 0.25, 1.0, 0.25, 0.05)  # unsorted, with 0, 1 and a repeat
THR = (0.0, 0.5, -np.inf, np.inf)


def _build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    inc = next(ROOT.glob("*_amd")) / "csrc"
    subprocess.run([HIPCC, "-std=c++17", *flags, f"-I{inc}", str(ROOT / "tests" / "cpp" / "summary_probs_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_summary_column_probs_matches_sort(tmp_path):
    """summary_column_probs for S in {1, 2, 3, 5, 41, 64, 65, 257}, Q in
    {0, 1, 2, 3, 4, 6, 7, 16} (both sides of every round of three ranks, and
    the maximum) and 0..8 thresholds at both digit widths, on normal, constant,
    three-valued, signed-zero, subnormal / 1e300 and decreasing columns: every
    quantile bitwise summary_lerp of std::sort's neighbours, the same bits
    when asked alone, exceedance fractions bitwise the plain count / S, the
    default request bitwise summary_column, NaN columns all NaN."""
    r = _build_and_run(tmp_path, "summary_probs_check", ["-O2"])
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def test_summary_column_probs_under_sanitizers(tmp_path):
    """The same stand-alone host program built with the address and
    undefined-behaviour sanitizers: no out-of-bounds access of the
    probabilities, thresholds, counters or the strided output, no undefined
    shift or conversion in the select."""
    r = _build_and_run(tmp_path, "summary_probs_check_san",
                       ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined"])
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _numpy_summary(x, probs, thr):
    """mean, np.quantile 'linear', sd and (x > t).sum(0) / S of an S x n matrix"""
    S = x.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # sd of one row, NaN columns
        cols = [x.mean(0)] + [np.quantile(x, p, axis=0) for p in probs] + [x.std(0, ddof=1)]
    bad = np.isnan(x).any(0)
    cols += [np.where(bad, np.nan, (x > t).sum(0) / S) for t in thr]
    return np.column_stack(cols)


@pytest.mark.parametrize("S", [1, 2, 5, 41])
def test_host_backend_matches_numpy(P, S):
    x = 0.3 + np.random.default_rng(S).normal(size=(S, 9))
    x[0, 2] = 0.5  # a threshold equal to a data value
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = P.get_summary(x, probs=PROBS, thresholds=THR)
        only_thr = P.get_summary(x, thresholds=(0.5,))
        only_probs = P.get_summary(x, probs=(0.5,))
        none = P.get_summary(x, probs=(), thresholds=())
        five = P.get_summary(x)
    assert got.shape == (9, 2 + len(PROBS) + len(THR))
    np.testing.assert_array_equal(got, _numpy_summary(x, PROBS, THR))
    np.testing.assert_array_equal(got[:, 1 + PROBS.index(0.0)], x.min(0))
    np.testing.assert_array_equal(got[:, 1 + PROBS.index(1.0)], x.max(0))
    np.testing.assert_array_equal(got[:, -2:], np.column_stack([np.ones(9), np.zeros(9)]))  # -inf, +inf
    # probs=None with a threshold: the default three, then the exceedance column
    assert only_thr.shape == (9, 6)
    np.testing.assert_array_equal(only_thr[:, :5], five)
    np.testing.assert_array_equal(only_thr[:, 5], (x > 0.5).sum(0) / S)
    assert only_probs.shape == (9, 3) and none.shape == (9, 2)
    np.testing.assert_array_equal(only_probs[:, 1], five[:, 2])
    np.testing.assert_array_equal(none, five[:, [0, 4]])


def test_host_backend_nan_column(P):
    x = np.random.default_rng(3).normal(size=(12, 4))
    clean = P.get_summary(x, probs=PROBS, thresholds=THR)
    x[7, 1] = np.nan
    got = P.get_summary(x, probs=PROBS, thresholds=THR)
    assert np.all(np.isnan(got[1]))
    np.testing.assert_array_equal(got[[0, 2, 3]], clean[[0, 2, 3]])


def test_host_backend_blocks_offsets_and_defaults(P):
    """Blocks with row offsets are the stacked, centred matrix (thresholds
    apply after the offset); without the new arguments nothing changes."""
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=(4, 6)), rng.normal(size=(9, 6))
    off = rng.normal(size=13)
    stacked = np.vstack([a, b]) - off[:, None]
    want = P.get_summary(stacked, probs=PROBS, thresholds=THR)
    np.testing.assert_array_equal(P.get_summary([a, b], row_offset=off, probs=PROBS, thresholds=THR), want)
    np.testing.assert_array_equal(want, _numpy_summary(stacked, PROBS, THR))
    np.testing.assert_array_equal(P.get_summary(stacked, probs=None, thresholds=None), P.get_summary(stacked))
    np.testing.assert_array_equal(P.get_summary(stacked, probs=(0.025, 0.5, 0.975)), P.get_summary(stacked))
    assert P.get_summary(stacked, probs=None, thresholds=None).shape == (6, 5)


def test_summary_columns(P):
    from nngp_amd import estimate

    assert P.summary_columns() == estimate.SUMMARY_COLS == ["mean", "q0.025", "median", "q0.975", "sd"]
    assert P.summary_columns() is not estimate.SUMMARY_COLS
    assert P.summary_columns(probs=(0.05, 0.5, 1), thresholds=(0.0, 2.5, -1e-3, np.inf)) == \
        ["mean", "q0.05", "q0.5", "q1", "sd", "p_gt_0", "p_gt_2.5", "p_gt_-0.001", "p_gt_inf"]
    assert P.summary_columns(thresholds=(1.0,)) == ["mean", "q0.025", "q0.5", "q0.975", "sd", "p_gt_1"]
    assert P.summary_columns(probs=()) == ["mean", "sd"]


BAD_REQUESTS = [({"probs": np.linspace(0, 1, 17)}, "at most 16 probs"),
                ({"thresholds": np.arange(9.0)}, "at most 8 thresholds"),
                ({"probs": (0.5, 1.0000001)}, r"probs must lie in \[0, 1\]"),
                ({"probs": (-1e-9,)}, r"probs must lie in \[0, 1\]"),
                ({"probs": (0.5, np.nan)}, r"probs must lie in \[0, 1\]"),
                ({"thresholds": (0.0, np.nan)}, "thresholds must not be NaN"),
                ({"probs": np.zeros((2, 2))}, "1-D")]


@pytest.mark.parametrize("kw,msg", BAD_REQUESTS)
def test_argument_errors_same_wording_on_both_backends(P, kw, msg):
    """A bad request is a ValueError before anything else happens: the hip
    backend raises the same words without touching a device."""
    x = np.random.default_rng(0).normal(size=(7, 5))
    for backend in ("host", "hip"):
        with pytest.raises(ValueError, match=msg):
            P.get_summary(x, backend=backend, **kw)
    with pytest.raises(ValueError, match=msg):
        P.summary_columns(**kw)


def test_library_rejects_bad_requests_before_any_device_call(P):
    """nngp_summary_probs itself: NNGP_ERR_ARG for every bad request, also on
    a machine without a GPU (the check comes before the first HIP call), and
    the output is not written."""
    import ctypes as C

    x = np.random.default_rng(0).normal(size=(7, 5))
    rows, ptrs = (C.c_longlong * 1)(7), (C.c_void_p * 1)(x.ctypes.data)

    def call(probs, thr, n_probs=None, n_thr=None):
        p, t = np.asarray(probs, np.float64), np.asarray(thr, np.float64)
        out = np.full((2 + 16 + 8, 5), -7.0)
        st = P.lib.nngp_summary_probs(0, ptrs, rows, 1, 5, None, 0, p.ctypes.data if p.size else None,
                                      p.size if n_probs is None else n_probs, t.ctypes.data if t.size else None,
                                      t.size if n_thr is None else n_thr, out)
        assert np.all(out == -7.0)
        return st

    assert call(np.linspace(0, 1, 17), ()) == 1
    assert call((), np.arange(9.0)) == 1
    assert call((0.5,), (), n_probs=-1) == 1
    assert call((), (0.5,), n_thr=-1) == 1
    assert call((), (), n_probs=2) == 1  # null array, positive count
    assert call((), (), n_thr=1) == 1
    assert call((0.5, 1.0000001), ()) == 1
    assert call((-0.1,), ()) == 1
    assert call((np.nan,), ()) == 1
    assert call((0.5,), (np.nan,)) == 1
    assert b"threshold" in P.lib.nngp_ctx_last_error(None)
    # what nngp_summary rejects, through the new entry
    assert P.lib.nngp_summary_probs(0, ptrs, rows, 1, 0, None, 0, None, 0, None, 0, np.zeros(8)) == 1
    assert P.lib.nngp_summary_probs(0, ptrs, rows, 1, 5, None, -1, None, 0, None, 0, np.zeros(10)) == 1


def test_hip_backend_without_gpu_fails_loudly(P):
    """No silent host fallback for the widened summary either: without a
    device the hip backend raises NNGP_ERR_NODEV."""
    from nngp_amd import _lib

    seen = P.lib.nngp_device_normals(0, 1, 0, 1, np.zeros(1))
    if seen == _lib.NNGP_OK:
        pytest.skip("GPU present")
    assert seen == _lib.NNGP_ERR_NODEV, seen
    x = np.random.default_rng(0).normal(size=(7, 5))
    with pytest.raises(P.NNGPError) as e:
        P.get_summary(x, backend="hip", probs=(0.1, 0.9), thresholds=(0.0,))
    assert e.value.status == 6


def _records(rng, n_chains=2, it=20, n=17):
    """A small synthetic run: the parts of mcmc_nngp_list that
    mcmc_nngp_estimate reads (fields saved every other iteration)."""
    saved = np.arange(2, it + 1, 2, dtype=float)
    recs = {}
    for k in range(n_chains):
        recs[f"chain_{k + 1}"] = {
            "iterations": np.array([[it, 0.0]]), "saved_field": saved,
            "params": {"log_scale": rng.normal(size=(it, 1)), "log_noise_variance": rng.normal(size=(it, 1)),
                       "shape": rng.normal(size=(it, 1)), "beta_0": rng.normal(size=(it, 1)),
                       "field": 0.4 + rng.normal(size=(len(saved), n))}}
    return {"records": recs, "X": {"X_mean": np.zeros(0), "names": []},
            "space_time_model": {"covfun": {"stationary_covfun": "exponential_isotropic", "shape_params": ["log_range"]}}}


def test_estimate_field_probs_and_thresholds(P):
    L = _records(np.random.default_rng(4))
    probs, thr = (0.05, 0.25, 0.75, 0.95), (0.0, 0.5)
    ref = P.mcmc_nngp_estimate(L)
    got = P.mcmc_nngp_estimate(L, field_probs=probs, field_thresholds=thr)
    assert "field_columns" not in ref and ref["field"].shape == (17, 5)
    assert got["field_columns"] == ["mean", "q0.05", "q0.25", "q0.75", "q0.95", "sd", "p_gt_0", "p_gt_0.5"]
    recs = list(L["records"].values())
    saved = recs[0]["saved_field"]
    sel = saved > 20 * 0.5
    x = np.vstack([c["params"]["field"][sel] - c["params"]["beta_0"][saved[sel].astype(int) - 1, 0][:, None]
                   for c in recs])
    assert x.shape == (10, 17)
    np.testing.assert_array_equal(got["field"], _numpy_summary(x, probs, thr))
    np.testing.assert_array_equal(got["field"][:, [0, 5]], ref["field"][:, [0, 4]])
    for k in ("covariance_params", "fixed_effects"):
        np.testing.assert_array_equal(got[k]["summary"] if k == "fixed_effects" else
                                      got[k]["sampled_covparams"]["summary"],
                                      ref[k]["summary"] if k == "fixed_effects" else
                                      ref[k]["sampled_covparams"]["summary"])
    only_thr = P.mcmc_nngp_estimate(L, field_thresholds=(0.0,))
    assert only_thr["field_columns"] == ["mean", "q0.025", "q0.5", "q0.975", "sd", "p_gt_0"]
    np.testing.assert_array_equal(only_thr["field"][:, :5], ref["field"])
