"""The tile sweep's r layout in LDS and its fused field write (needs an MI355X).

The 3-chain wave-local tile kernel keeps r chain-major in LDS
(tiles.hip tile_r_index), the other instantiations interleaved, and every
one-GPU tile call writes the field from the sweep kernel's closing section
instead of an epilogue kernel (TileLaunch::slot_dpos; capi.hip
enqueue_sweep_body).  Both only move bytes, so everything here is pinned to
references that do not depend on either: the oracle's local-form sweep
(update_Gaussian.R:257-275), the cold-call context, 1-chain contexts.

Small fields forced onto several LDS tiles (NNGP_TILES): the tiles have odd
and even row counts, rows shared between tiles (ghost cells) and batches with
padding cells.  C = 3 runs the chain-major instantiation (also on an
interior-first layout, NNGP_TILE_SPLIT=1), C = 1 and 2 the interleaved ones.

Tolerances are the existing tests': tile sweep against the oracle rtol 1e-8,
atol 1e-9 (tests/test_gpu_parity.py, the tile-engine cases); warm against
cold calls 1e-10 max|field| and r drift 1e-11 max|B w|
(tests/test_gpu_warm_calls.py).
"""
import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

COV = "exponential_isotropic"
CPS = [[1.0, 0.1, 0.0], [0.7, 0.05, 0.0], [1.3, 0.08, 0.0]]
B0S, LSS, LNVS, SEEDS = [0.1, -0.2, 0.3], [0.0, 0.2, -0.3], [-0.5, -0.2, -0.9], [5, 6, 7]
# (n, m, tiles)
SHAPES = [(4001, 5, 8), (12000, 10, 24)]

_problems = {}


def _problem(P, n, m):
    """One problem (and its start fields) per shape, shared and left unchanged."""
    if (n, m) not in _problems:
        prob = make_problem(P, n, m, seed=n + m)
        rng = np.random.default_rng(m)
        _problems[(n, m)] = (prob, [rng.normal(size=n) for _ in range(3)])
    return _problems[(n, m)]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _open(P, monkeypatch, prob, C, tiles, fields, b0s=B0S, warm=True, split=False):
    locs, NN, col, lm, y = prob
    for v in ("NNGP_ENGINE", "NNGP_TILE_XW", "NNGP_TILE_WL", "NNGP_TILE_NT", "NNGP_TILE_CHAINS", "NNGP_TILE_R"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("NNGP_TILES", str(tiles))
    if split:
        monkeypatch.setenv("NNGP_TILE_SPLIT", "1")
    else:
        monkeypatch.delenv("NNGP_TILE_SPLIT", raising=False)
    if warm:
        monkeypatch.delenv("NNGP_SWEEP_WARM", raising=False)
    else:
        monkeypatch.setenv("NNGP_SWEEP_WARM", "0")
    ctx = P.ChainContext(locs, NN, col, lm, y, device=0, n_chains=C)
    monkeypatch.delenv("NNGP_SWEEP_WARM", raising=False)
    monkeypatch.delenv("NNGP_TILE_SPLIT", raising=False)
    info = ctx.info
    assert info["sweep_engine"] == 1 and info["n_tiles"] == tiles and not info["tile_r_global"], info
    for k in range(C):
        ctx.select(k)
        ctx.factor(0, COV, CPS[k])
        ctx.set_field(fields[k])
        ctx.set_mu(None, b0s[k])
    return ctx


def _fields(ctx, C):
    return [ctx.select(k).get_field() for k in range(C)]


def _oracle(O, prob, L, field, k, base, n_sweeps, b0=None):
    locs, NN, col, lm, y = prob
    n = len(field)
    b0 = B0S[k] if b0 is None else b0
    z = O.sweep_normals(SEEDS[k], base, n_sweeps, n)
    return O.sweep("local", field, L, NN, col, O.precision_diag(L, NN), np.ones(n, np.int32), y, np.full(n, b0), lm,
                   b0, LSS[k], LNVS[k], z)


@pytest.mark.parametrize("n,m,tiles", SHAPES)
@pytest.mark.parametrize("C,split", [(1, False), (2, False), (3, False), (3, True)])
def test_two_calls_match_oracle(P, O, monkeypatch, n, m, tiles, C, split):
    """Two calls, of 2 sweeps and then 1, per-chain factors and beta_0:
    every chain's field after each call against the oracle's local-form sweep
    with the same Philox normals."""
    prob, fields = _problem(P, n, m)
    ctx = _open(P, monkeypatch, prob, C, tiles, fields, split=split)
    try:
        Ls = [ctx.select(k).get_linv(0) for k in range(C)]
        ctx.sweep_chains(2, B0S[:C], LSS[:C], LNVS[:C], SEEDS[:C], [3] * C)
        got1 = _fields(ctx, C)
        ctx.sweep_chains(1, B0S[:C], LSS[:C], LNVS[:C], SEEDS[:C], [5] * C)
        got2 = _fields(ctx, C)
    finally:
        ctx.close()
    for k in range(C):
        ref1 = _oracle(O, prob, Ls[k], fields[k], k, 3, 2)
        np.testing.assert_allclose(got1[k], ref1, rtol=1e-8, atol=1e-9, err_msg=f"call 1 chain {k}")
        ref2 = _oracle(O, prob, Ls[k], ref1, k, 5, 1)
        np.testing.assert_allclose(got2[k], ref2, rtol=1e-8, atol=1e-9, err_msg=f"call 2 chain {k}")


@pytest.mark.parametrize("C", [1, 3])
def test_warm_shifted_and_cold_calls(P, monkeypatch, C):
    """A cold call, a warm one, shifted ones (beta_0 moved) and a cold one
    again (chain 0: new field): get_field after every call against the
    NNGP_SWEEP_WARM=0 context; then 20 shifted one-sweep calls, after which the
    r the kernel wrote back matches a fresh B (field - beta_0)."""
    n, m, tiles = SHAPES[1]
    prob, fields = _problem(P, n, m)
    new_field = np.random.default_rng(99).normal(size=n)
    shifts = [[0.0] * 3, [0.0] * 3, [0.31, -0.07, 1e-9], [-0.5, 0.02, 0.0], [0.0] * 3]
    res = {}
    for warm in (True, False):
        ctx = _open(P, monkeypatch, prob, C, tiles, fields, warm=warm)
        b0 = list(B0S[:C])
        try:
            res[warm] = []
            for call, d in enumerate(shifts):
                b0 = [a + x for a, x in zip(b0, d)]
                if call == 4:
                    ctx.select(0).set_field(new_field)
                ctx.sweep_chains(2 if call % 2 else 1, b0, LSS[:C], LNVS[:C], SEEDS[:C], [10 * call] * C)
                res[warm].append(_fields(ctx, C))
            if warm:
                rng = np.random.default_rng(16)
                for call in range(20):
                    b0 = [a + x for a, x in zip(b0, rng.normal(scale=0.05, size=C))]
                    ctx.sweep_chains(1, b0, LSS[:C], LNVS[:C], SEEDS[:C], [100 + call] * C)
                for k in range(C):
                    ctx.select(k)
                    r = ctx.get_sweep_r()
                    fresh = ctx.spmv(0, ctx.get_field() - b0[k])
                    e = _rel(r, fresh)
                    print(f"r drift chain {k}: {e:.3e}")
                    assert e <= 1e-11, (k, e)
        finally:
            ctx.close()
    for call in range(len(shifts)):
        for k in range(C):
            e = _rel(res[True][call][k], res[False][call][k])
            print(f"warm vs cold call {call} chain {k}: {e:.3e}")
            assert e <= 1e-10, (call, k, e)
    for k in range(C):  # the first call is cold on both
        assert np.array_equal(res[True][0][k], res[False][0][k])


def test_fused_field_write_respects_chain_mask(P, monkeypatch):
    """nngp_sweep on chain 1 of a 3-chain context: the fields of chains 0 and
    2 keep their bits; chain 1's field is, bitwise, what the same chain gets
    when the context sweeps every chain at once (batched = single), and equals
    a 1-chain context's to rounding -- its layout cuts the batches for another
    chain count, so the lanes' partial sums of a column add up in another
    order: rtol 1e-11, atol 1e-12, the bound
    test_batched_chains_bitwise_equal_single_chain_contexts sets for the same
    comparison."""
    n, m, tiles = SHAPES[1]
    prob, fields = _problem(P, n, m)
    ctx = _open(P, monkeypatch, prob, 3, tiles, fields)
    try:
        before = _fields(ctx, 3)
        ctx.select(1).sweep(2, B0S[1], LSS[1], LNVS[1], SEEDS[1], 4)
        after = _fields(ctx, 3)
        # a second, warm call of chain 1 alone
        ctx.select(1).sweep(1, B0S[1], LSS[1], LNVS[1], SEEDS[1], 6)
        after2 = _fields(ctx, 3)
    finally:
        ctx.close()
    for k in (0, 2):
        assert np.array_equal(before[k], fields[k])
        assert np.array_equal(after[k], fields[k]), k
        assert np.array_equal(after2[k], fields[k]), k
    assert not np.array_equal(after[1], fields[1]) and not np.array_equal(after2[1], after[1])
    ctx = _open(P, monkeypatch, prob, 3, tiles, fields)
    try:
        ctx.sweep_chains(2, B0S, LSS, LNVS, SEEDS, [4] * 3)
        batched = ctx.select(1).get_field()
    finally:
        ctx.close()
    assert np.array_equal(after[1], batched)
    ctx = _open(P, monkeypatch, prob, 1, tiles, [fields[1]], b0s=[B0S[1]])
    try:
        ctx.factor(0, COV, CPS[1])
        ctx.sweep(2, B0S[1], LSS[1], LNVS[1], SEEDS[1], 4)
        one = ctx.get_field()
    finally:
        ctx.close()
    print(f"chain 1 vs 1-chain context: {np.abs(after[1] - one).max():.3e}")
    np.testing.assert_allclose(after[1], one, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("C", [1, 3])
def test_field_is_current_on_the_stream(P, monkeypatch, C):
    """A log-likelihood right after a sweep call, no host read in between,
    against the log-likelihood of a fresh context given the swept field."""
    n, m, tiles = SHAPES[1]
    prob, fields = _problem(P, n, m)
    mask = (1 << C) - 1
    ctx = _open(P, monkeypatch, prob, C, tiles, fields)
    try:
        ctx.sweep_chains(2, B0S[:C], LSS[:C], LNVS[:C], SEEDS[:C], [0] * C)
        ll1 = ctx.loglik_chains(0, mask, B0S[:C], LSS[:C])
        ctx.sweep_chains(1, B0S[:C], LSS[:C], LNVS[:C], SEEDS[:C], [2] * C)  # warm
        ll2 = ctx.loglik_chains(0, mask, B0S[:C], LSS[:C])
        swept = _fields(ctx, C)
    finally:
        ctx.close()
    ctx = _open(P, monkeypatch, prob, C, tiles, swept)
    try:
        ref2 = ctx.loglik_chains(0, mask, B0S[:C], LSS[:C])
    finally:
        ctx.close()
    assert np.all(np.isfinite(ll1)) and not np.array_equal(ll1, ll2)
    for k in range(C):
        e = abs(ll2[k] - ref2[k]) / abs(ref2[k])
        print(f"loglik chain {k}: {ll2[k]!r} vs {ref2[k]!r} ({e:.1e})")
        assert e <= 1e-12, (k, ll2[k], ref2[k])


@pytest.mark.parametrize("path", ["one_sweep", "timed", "injected"])
def test_every_call_path_writes_the_field(P, O, monkeypatch, path):
    """One sweep per call, the three-part timed call (prologue, colours and
    epilogue as separate launches) and injected normals: each leaves the swept
    field (against the oracle)."""
    n, m, tiles = SHAPES[0]
    C = 3
    prob, fields = _problem(P, n, m)
    ctx = _open(P, monkeypatch, prob, C, tiles, fields)
    try:
        Ls = [ctx.select(k).get_linv(0) for k in range(C)]
        if path == "one_sweep":
            ctx.sweep_chains(1, B0S, LSS, LNVS, SEEDS, [7] * C)
            refs = [_oracle(O, prob, Ls[k], fields[k], k, 7, 1) for k in range(C)]
        elif path == "timed":
            ms, kms = ctx.sweep_timed(2, B0S, LSS, LNVS, SEEDS, [7] * C, per_kernel=True)
            assert ms > 0 and kms > 0
            refs = [_oracle(O, prob, Ls[k], fields[k], k, 7, 2) for k in range(C)]
        else:
            z = np.random.default_rng(3).normal(size=(2, n))
            ctx.select(2).sweep(2, B0S[2], LSS[2], LNVS[2], 1, 0, z=z)
            locs, NN, col, lm, y = prob
            refs = [fields[0], fields[1],
                    O.sweep("local", fields[2], Ls[2], NN, col, O.precision_diag(Ls[2], NN), np.ones(n, np.int32), y,
                            np.full(n, B0S[2]), lm, B0S[2], LSS[2], LNVS[2], z)]
        got = _fields(ctx, C)
    finally:
        ctx.close()
    for k in range(C):
        np.testing.assert_allclose(got[k], refs[k], rtol=1e-8, atol=1e-9, err_msg=f"{path} chain {k}")
