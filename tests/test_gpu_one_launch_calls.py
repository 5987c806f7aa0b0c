"""One-launch tile sweep calls against the captured-graph calls (needs an
MI355X).

A warm tile call of a one-GPU context is one stream operation: the tile
launch takes the chains' scalars and its call id as kernel arguments
(kernels.h TileCall), no bump kernel runs before it, the scalars are uploaded
only for the kernels that still read them from device memory (capi.hip
ensure_scalars), and the sticky timeout word is fetched at the next host sync
(tile_timeout_check).  NNGP_SWEEP_GRAPH=1 keeps the earlier call (captured
graph, bump kernel, upload and timeout copy per call): the oracle here.
Nothing arithmetic differs, so every comparison between the two is bitwise.

Setup as bench.py's parity check: n = 20,000, m = 10, exponential_isotropic,
NNGP_TILES=16; C = 1, 2, 3 chains.  The sequences exercise the ways a stale
argument could hide: every scalar changes between calls; a masked
(single-chain) call follows a shifted call (the other chain's staged shift
must not be applied again: also against a NNGP_SWEEP_WARM=0 context, to
1e-10 max|field| as tests/test_gpu_warm_calls.py); a cold call follows warm
ones (the lazy scalar upload before the prologue kernels); 40 one-sweep calls
with consecutive call ids and shared granule slots; an injected timeout; two
tile contexts on one device (launches chained by an event).
"""
import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

COV = "exponential_isotropic"
N, M = 20_000, 10
CPS = [[1.0, 0.08, 0.0], [1.2, 0.06, 0.0], [0.8, 0.1, 0.0]]
_cache = {}


def _problem(P, seed=99):
    if seed not in _cache:
        prob = make_problem(P, N, M, seed=seed)
        rng = np.random.default_rng(seed + 1)
        _cache[seed] = (prob, [rng.normal(size=N) for _ in range(3)])
    return _cache[seed]


def _open(P, monkeypatch, C, graph=False, warm=True, inject=None, seed=99):
    """A C-chain tile context; the switches are read when it is created."""
    prob, fields = _problem(P, seed)
    monkeypatch.delenv("NNGP_ENGINE", raising=False)
    monkeypatch.setenv("NNGP_TILES", "16")
    for var, val in (("NNGP_SWEEP_GRAPH", "1" if graph else None), ("NNGP_SWEEP_WARM", None if warm else "0"),
                     ("NNGP_TILE_INJECT_TIMEOUT", inject)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    ctx = P.ChainContext(*prob, device=0, n_chains=C)
    for var in ("NNGP_SWEEP_GRAPH", "NNGP_SWEEP_WARM", "NNGP_TILE_INJECT_TIMEOUT"):
        monkeypatch.delenv(var, raising=False)
    assert ctx.info["sweep_engine"] == 1, ctx.info
    for k in range(C):
        ctx.select(k)
        ctx.factor(0, COV, CPS[k])
        ctx.set_field(fields[k])
        ctx.set_mu(None, 0.1 * k)
    return ctx


def _fields(ctx, C):
    return [ctx.select(k).get_field() for k in range(C)]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _sequence(P, ctx, C):
    """-> field snapshots (lists of C arrays) after the stages of the call
    sequence; the same calls whatever the context's switches."""
    snaps = []
    b0 = [0.1 * k for k in range(C)]
    ls = [0.0, 0.2, -0.1][:C]
    lnv = [-0.5, -0.4, -0.6][:C]
    # every scalar changes between the calls; 1, 2, 3 sweeps; calls 2 and 3 are
    # warm with beta_0 moved (shifted)
    for call, ns in enumerate((1, 2, 3)):
        if call:
            b0 = [b + 0.07 * (k + 1) * call for k, b in enumerate(b0)]
            ls = [x + 0.05 * call for x in ls]
            lnv = [x - 0.03 * call for x in lnv]
        ctx.sweep_chains(ns, b0, ls, lnv, [11 + 7 * call + k for k in range(C)], [100 * call + k for k in range(C)])
    snaps.append(_fields(ctx, C))
    # another shifted call of every chain, then masked calls: chain 1 alone
    # (its beta_0 moves again), then chain 0 alone with its beta_0 unchanged --
    # chain 0's shift of the call before must not be applied a second time
    b0 = [b - 0.21 - 0.1 * k for k, b in enumerate(b0)]
    ctx.sweep_chains(2, b0, ls, lnv, [41 + k for k in range(C)], [400] * C)
    order = [1, 0] if C > 1 else [0]
    for j, k in enumerate(order):
        if j == 0 and C > 1:
            b0[k] += 0.3
        P.context.ChainView(ctx, k).sweep(2, b0[k], ls[k] + 0.01, lnv[k], 51 + k, 500 + j)
    snaps.append(_fields(ctx, C))
    # a cold chain among warm ones: a new current factor for the last chain
    ctx.select(C - 1).factor(0, COV, [1.1, 0.07, 0.0])
    b0 = [b + 0.05 for b in b0]
    ctx.sweep_chains(2, b0, ls, lnv, [61 + k for k in range(C)], [600] * C)
    ctx.sweep_chains(1, b0, ls, lnv, [61 + k for k in range(C)], [602] * C)
    snaps.append(_fields(ctx, C))
    return snaps


@pytest.mark.parametrize("C", [1, 2, 3])
def test_call_sequence_equals_graph_calls(P, monkeypatch, C):
    """The sequence on a default context, on a NNGP_SWEEP_GRAPH=1 context
    (bitwise) and on a NNGP_SWEEP_WARM=0 context (every call rebuilds w and r:
    <= 1e-10 max|field|, which a shift applied twice -- 0.21 or more -- misses
    by nine orders of magnitude)."""
    res = {}
    for name, kw in (("new", {}), ("graph", {"graph": True}), ("cold", {"warm": False})):
        ctx = _open(P, monkeypatch, C, **kw)
        try:
            res[name] = _sequence(P, ctx, C)
        finally:
            ctx.close()
    for stage, (a, b, c) in enumerate(zip(res["new"], res["graph"], res["cold"])):
        for k in range(C):
            assert np.array_equal(a[k], b[k]), (stage, k, _rel(a[k], b[k]))
            e = _rel(a[k], c[k])
            print(f"C={C} stage {stage} chain {k}: one-launch vs rebuilt-every-call {e:.3e}")
            assert e <= 1e-10, (stage, k, e)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_forty_calls_back_to_back(P, monkeypatch, C):
    """40 one-sweep calls with nothing read in between: call ids one apart,
    every call rewriting the same granule slots."""
    res = []
    for graph in (False, True):
        ctx = _open(P, monkeypatch, C, graph=graph)
        try:
            b0 = [0.1 * k for k in range(C)]
            for call in range(40):
                ctx.sweep_chains(1, b0, [0.0] * C, [-0.5] * C, [71 + k for k in range(C)], [call] * C)
            res.append(_fields(ctx, C))
        finally:
            ctx.close()
    for k in range(C):
        assert np.array_equal(res[0][k], res[1][k]), k
        assert np.isfinite(res[0][k]).all()


@pytest.mark.parametrize("C", [1, 2, 3])
def test_injected_timeout_reported_at_first_sync(P, monkeypatch, C):
    """NNGP_TILE_INJECT_TIMEOUT=1 on the one-launch path: the first host sync
    after the first call reports the tile timeout (nothing copies the word
    behind the launch: it is fetched at the sync), once; the next call runs
    clean and leaves the fields of the same two calls on a fresh context."""
    b0 = [0.1 * k for k in range(C)]
    args = ([0.0] * C, [-0.5] * C, [81 + k for k in range(C)])
    ctx = _open(P, monkeypatch, C, inject="1")
    try:
        ctx.sweep_chains(2, b0, *args, [0] * C)
        with pytest.raises(P.NNGPError, match="timed out"):
            ctx.select(0).get_field()
        ctx.sweep_chains(2, b0, *args, [2] * C)
        got = _fields(ctx, C)
    finally:
        ctx.close()
    ref_ctx = _open(P, monkeypatch, C)
    try:
        ref_ctx.sweep_chains(2, b0, *args, [0] * C)
        ref_ctx.sweep_chains(2, b0, *args, [2] * C)
        ref = _fields(ref_ctx, C)
    finally:
        ref_ctx.close()
    for k in range(C):
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("C", [1, 2, 3])
def test_two_tile_contexts_alternating(P, monkeypatch, C):
    """Two tile contexts on device 0 (their launches chained by the device's
    tile event), calls alternating between them, warm and shifted: both equal
    their NNGP_SWEEP_GRAPH=1 twins bitwise."""
    res = []
    for graph in (False, True):
        ctxs = [_open(P, monkeypatch, C, graph=graph, seed=99), _open(P, monkeypatch, C, graph=graph, seed=77)]
        try:
            for call in range(4):
                for q, ctx in enumerate(ctxs):
                    b0 = [0.1 * k + 0.05 * call * (q + 1) for k in range(C)]
                    ctx.sweep_chains(1 + call % 2, b0, [0.1 * q] * C, [-0.5] * C, [91 + 10 * q + k for k in range(C)],
                                     [10 * call] * C)
            res.append([_fields(ctx, C) for ctx in ctxs])
        finally:
            for ctx in ctxs:
                ctx.close()
    for q in range(2):
        for k in range(C):
            assert np.array_equal(res[0][q][k], res[1][q][k]), (q, k)
