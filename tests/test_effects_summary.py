"""effects_summary / nngp_effects_summary without a GPU: the host backend
against numpy, mcmc_nngp_predict_fixed_effects' unchanged defaults, and the
argument checks of the C entry, which are made before any HIP call (so they
answer NNGP_ERR_ARG on a machine without a device too)."""
import ctypes as C

import numpy as np
import pytest

PROBS, THR = (0.9, 0.0, 0.25, 1.0, 0.25), (0.0, -np.inf, 1.5)


def _problem(S=23, n=37, q=4, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(S, q)), rng.normal(size=(n, q)), rng.normal(size=(S, n))


def test_host_backend_is_get_summary_of_the_product(P):
    coef, X, add = _problem()
    np.testing.assert_array_equal(P.effects_summary(coef, X), P.get_summary(coef @ X.T))
    np.testing.assert_array_equal(P.effects_summary(coef, X, addend=add, backend="host"),
                                  P.get_summary(coef @ X.T + add))
    got, samples = P.effects_summary(coef, X, addend=[add[:10], add[10:10], add[10:]], probs=PROBS, thresholds=THR,
                                     return_samples=True)
    np.testing.assert_array_equal(samples, coef @ X.T + add)
    np.testing.assert_array_equal(got, P.get_summary(coef @ X.T + add, probs=PROBS, thresholds=THR))
    assert got.shape == (37, 2 + len(PROBS) + len(THR))
    with pytest.raises(ValueError):
        P.effects_summary(coef, X, addend=add[:5])
    with pytest.raises(ValueError):
        P.effects_summary(coef, X[:, :3])
    with pytest.raises(ValueError):
        P.effects_summary(coef, X, backend="cuda")


def _run_list(rng, chains=2, iters=40, p=3, thin=2):
    """A small synthetic mcmc_nngp_list: what mcmc_nngp_predict_fixed_effects reads."""
    saved = np.arange(thin, iters + 1, thin, dtype=np.float64)
    recs = {}
    for k in range(chains):
        recs[f"chain_{k + 1}"] = {"iterations": np.column_stack([np.arange(1, iters + 1), np.zeros(iters)]),
                                  "saved_field": saved,
                                  "params": {"beta_0": rng.normal(size=(iters, 1)), "beta": rng.normal(size=(iters, p))}}
    return {"records": recs, "X": {"names": [f"V{j + 1}" for j in range(p)], "X_mean": rng.normal(size=p)}}


def _fixed_effects_before(L, Xp, burn_in, match, intercept):
    """mcmc_nngp_predict_fixed_effects as it stood before effects_summary."""
    first = next(iter(L["records"].values()))
    stored = first["saved_field"] if match else np.arange(1, int(first["iterations"][-1, 0]) + 1)
    stored = stored[stored > burn_in * stored.max()].astype(int)
    mm = np.column_stack([np.ones(len(Xp)), Xp])
    subset = list(range(mm.shape[1]))
    if not intercept:
        mm, subset = mm[:, 1:], subset[1:]
    out = []
    for chain in L["records"].values():
        bm = np.column_stack([chain["params"]["beta_0"], chain["params"]["beta"]])[stored - 1].copy()
        bm[:, 0] = bm[:, 0] - bm[:, 1:] @ L["X"]["X_mean"]
        out.append(bm[:, subset] @ mm.T)
    return out


@pytest.mark.parametrize("match,intercept", [(True, False), (False, True)])
def test_predict_fixed_effects_defaults_unchanged(P, match, intercept):
    rng = np.random.default_rng(3)
    L = _run_list(rng)
    Xp = rng.normal(size=(11, 3))
    kw = dict(burn_in=0.5, match_field_thinning=match, add_intercept=intercept)
    got = P.mcmc_nngp_predict_fixed_effects(L, Xp, **kw)
    ref = _fixed_effects_before(L, Xp, 0.5, match, intercept)
    assert list(got) == ["X_predicted", "predicted_fixed_effects_samples", "predicted_fixed_effects_summary"]
    assert got["X_predicted"] is Xp and len(got["predicted_fixed_effects_samples"]) == 2
    for a, b in zip(got["predicted_fixed_effects_samples"], ref):
        assert a.shape == ((10 if match else 20), 11)
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got["predicted_fixed_effects_summary"], P.get_summary(np.vstack(ref)))
    # keep_samples=False: the same summary, no samples
    lean = P.mcmc_nngp_predict_fixed_effects(L, Xp, keep_samples=False, **kw)
    assert lean["predicted_fixed_effects_samples"] is None
    np.testing.assert_array_equal(lean["predicted_fixed_effects_summary"], got["predicted_fixed_effects_summary"])
    wide = P.mcmc_nngp_predict_fixed_effects(L, Xp, summary_probs=PROBS, summary_thresholds=THR, **kw)
    assert wide["predicted_fixed_effects_summary_columns"] == P.summary_columns(PROBS, THR)
    np.testing.assert_array_equal(wide["predicted_fixed_effects_summary"],
                                  P.get_summary(np.vstack(ref), probs=PROBS, thresholds=THR))
    with pytest.raises(ValueError):
        P.mcmc_nngp_predict_fixed_effects(L, Xp, summary_backend="cuda")


def test_symbols_exported(P):
    from nngp_amd import _lib

    lib = C.CDLL(str(_lib.LIB_PATH))
    for s in ("nngp_effects_summary", "nngp_effects_stats"):
        assert s in _lib.ABI_SYMBOLS and hasattr(lib, s)
        assert getattr(_lib.lib, s).argtypes is not None
    assert P.effects_stats and P.mcmc_nngp_predict_response


def _call(lib, **over):
    """nngp_effects_summary on a valid 5 x 3 (q = 2) problem with some arguments replaced."""
    S, n, q = int(over.get("S", 5)), int(over.get("n", 3)), int(over.get("q", 2))
    keep = {"coef": np.ones((2, 5)), "X": np.ones((2, 3)), "out": np.empty((16 + 8 + 2, 3)),
            "probs": np.array([0.5, 0.1]), "thr": np.array([0.0]), "add": np.ones((5, 3)),
            "sd": np.ones(5), "ctr": np.arange(5, dtype=np.uint64)}
    a = {"coef": keep["coef"].ctypes.data, "X": keep["X"].ctypes.data, "out": keep["out"].ctypes.data,
         "blocks": None, "rows": None, "n_blocks": 0, "noise_sd": None, "counter": None, "chunk_cols": 0,
         "probs": keep["probs"].ctypes.data, "n_probs": 2, "thr": keep["thr"].ctypes.data, "n_thr": 1}
    for k, v in over.items():
        if k in ("S", "n", "q"):
            continue
        if isinstance(v, np.ndarray):
            keep[k + "_arg"] = v
            v = v.ctypes.data
        a[k] = v
    if isinstance(a["blocks"], (list, tuple)):
        bl = a["blocks"]
        keep["bl"] = [b for b in bl if b is not None]
        a["rows"] = (C.c_longlong * len(bl))(*a["rows"])
        a["blocks"] = (C.c_void_p * len(bl))(*[None if b is None else b.ctypes.data for b in bl])
        a["n_blocks"] = len(bl)
    return lib.nngp_effects_summary(-1, a["coef"], S, q, a["X"], n, a["blocks"], a["rows"], a["n_blocks"],
                                    a["noise_sd"], 7, a["counter"], a["chunk_cols"], a["probs"], a["n_probs"],
                                    a["thr"], a["n_thr"], a["out"], None)


BAD = {
    "n_probs 17": dict(n_probs=17),
    "n_probs -1": dict(n_probs=-1),
    "n_thresholds 9": dict(n_thr=9),
    "null probs, positive count": dict(probs=None),
    "null thresholds, positive count": dict(thr=None),
    "NaN probability": dict(probs=np.array([0.5, np.nan])),
    "probability above 1": dict(probs=np.array([0.5, 1.0000001])),
    "negative probability": dict(probs=np.array([-1e-9, 0.5])),
    "NaN threshold": dict(thr=np.array([np.nan])),
    "null coef": dict(coef=None),
    "null X": dict(X=None),
    "null out": dict(out=None),
    "n 0": dict(n=0),
    "n_samples 0": dict(S=0),
    "n_samples 2^31": dict(S=2 ** 31),
    "q 0": dict(q=0),
    "q 1025": dict(q=1025),
    "addend rows short": dict(blocks=[np.ones((4, 3))], rows=[4]),
    "addend rows long": dict(blocks=[np.ones((3, 3)), np.ones((3, 3))], rows=[3, 3]),
    "null addend block": dict(blocks=[np.ones((2, 3)), None], rows=[2, 3]),
    "NaN noise_sd": dict(noise_sd=np.array([1.0, 1.0, np.nan, 1.0, 1.0]), counter=np.arange(5, dtype=np.uint64)),
    "negative noise_sd": dict(noise_sd=np.array([1.0, -1e-300, 1.0, 1.0, 1.0]), counter=np.arange(5, dtype=np.uint64)),
    "noise_sd without counter": dict(noise_sd=np.ones(5)),
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_err_arg_before_any_hip_call(P, case):
    from nngp_amd import _lib

    assert _call(_lib.lib, **BAD[case]) == _lib.NNGP_ERR_ARG, case
    assert _lib.lib.nngp_ctx_last_error(None)


def test_good_arguments_pass_the_checks(P):
    """The call the bad cases are one change away from: past the argument
    checks (no device here: NNGP_ERR_NODEV; with one it succeeds)."""
    from nngp_amd import _lib

    good = [dict(), dict(blocks=[np.ones((2, 3)), np.ones((0, 3)), np.ones((3, 3))], rows=[2, 0, 3]),
            dict(noise_sd=np.array([0.0, 1.0, np.inf, 2.0, 3.0]), counter=np.arange(5, dtype=np.uint64)),
            dict(n_probs=0, probs=None, n_thr=0, thr=None)]
    for kw in good:
        assert _call(_lib.lib, **kw) in (_lib.NNGP_OK, _lib.NNGP_ERR_NODEV), kw
