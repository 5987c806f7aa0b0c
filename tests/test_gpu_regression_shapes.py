"""The nngp_design_* primitives (regress.hip) over their launch shapes and
limits, judged as tests/test_gpu_regression_device.py judges them: chain by
chain against long double, within the a-priori bounds of _check_against_numpy
((n_obs + 2) U mean statistics, (n + 4b + 2 ql) U t, (n + 4b) U Gram matrix,
(ql + 3) eps field, (p + 1) eps mu, each x the sum of the absolute values of
the products), refreshed == 1, a symmetric Gram matrix, and batched == one
chain at a time, bitwise.

What the shapes reach:
  row groups ....... b = m + 1 on both sides of 4|5, 8|9, 16|17 and b = 32:
                     design_sx_kernel<G> / design_spmv_kernel<G>, G = 4..32;
                     n = 5 with b = 11: NA lanes inside every row's group
  row-group stride . n = 70,000 > 8192 blocks x 8 rows at G = 32 (b = 17);
                     b = 5 (G = 8, 32 rows per block) at the same n does not stride
  tile tails ....... n and n_obs one below, at and one above 256 (a wave row of
                     the 4 x 256 tile), 1024 (the tile), and several blocks
  reduction stride . n_obs = 1024 x 1024 + 1025: design_mean_stats past its
                     1024 blocks, design_mu past 4096 x 256, reg_reduce of 4096
                     partials
  column limits .... p_locs = 31 (q = 32, 528 Gram pairs), 32 refused
  chains ........... C = 1, 2, 4, split masks at C = 4

Not reached: the grid stride of design_gram / design_tstats (and of
design_other / design_field / design_gather) starts beyond 1,048,576
locations, which a test of a few seconds does not hold; those loops have the
form of design_mean_stats's and design_mu's, which the reduction-stride case
runs, but they are not run here themselves.

Measured on an MI355X, the worst max error / bound over all cases of this
module (each case prints its own), as a fraction of the unchanged bound:
  mean statistics 0.105   t 0.0155   Gram matrix 0.0233   field 0.301   mu 0.374
(the sums sit far inside their worst-case bounds; the two elementwise results,
with bounds of a few eps, come within a factor of three).
"""
import numpy as np
import pytest

from test_gpu_regression_device import (COV, CPS, _assert_same, _chain_inputs, _check_against_numpy, _open,
                                        _primitives, _primitives_on, _synthetic)

pytestmark = pytest.mark.gpu


def _case(P, O, pr, C):
    """All chains in one call within the bounds; one chain at a time == batched, bitwise."""
    inp = _chain_inputs(pr, C)
    batched = _primitives(P, pr, inp, [(1 << C) - 1])
    _check_against_numpy(O, pr, inp, batched)
    _assert_same(batched, _primitives(P, pr, inp, [1 << k for k in range(C)]))
    return inp, batched


def _cols(p, ql, seed=1):
    """ql distinct columns of 0..p-1, not in order"""
    return [int(c) for c in np.random.default_rng(seed).permutation(p)[:ql]]


@pytest.mark.parametrize("n,m", [(600, m) for m in (1, 3, 4, 7, 8, 15, 16, 31)] + [(5, 10)])
def test_row_groups(P, O, n, m):
    """b = m + 1 = 2, 4 | 5, 8 | 9, 16 | 17, 32: every instantiation of the
    row-group kernels on both sides of each threshold; n = 5, m = 10: b = 11
    with at most 5 entries in a row."""
    pr = _synthetic(P, 4, [3, 1], n=n, m=m)
    assert pr["NN"].shape == (n, m + 1)
    _case(P, O, pr, 3)


@pytest.mark.parametrize("m", [16, 4])
def test_row_group_grid_stride(P, O, m):
    """70,000 locations: 8192 blocks of 8 rows end at 65,536, so the 32-lane
    groups of b = 17 take a second pass; b = 5 is the unstrided control."""
    _case(P, O, _synthetic(P, 2, [1], n=70000, m=m), 2)


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025, 4097])
def test_location_tile_tails(P, O, n):
    _case(P, O, _synthetic(P, 3, [2, 0], n=n, m=5), 3)


@pytest.mark.parametrize("n_obs", [1024, 1025, 2049])
def test_observation_tile_tails(P, O, n_obs):
    pr = _synthetic(P, 3, [2, 0], n=700, m=5, n_obs=n_obs)
    assert len(pr["y"]) == n_obs and not np.array_equal(pr["first_obs"], np.arange(1, 701))
    _case(P, O, pr, 3)


def test_reduction_grid_stride(P, O):
    """1024 x 1024 + 1025 observations of 2,000 locations, p = 1, p_locs = 0:
    every block of design_mean_stats adds a second tile into its partials, one
    block a third; design_mu strides; reg_reduce sums 4096 partials."""
    pr = _synthetic(P, 1, [], n=2000, m=5, n_obs=1024 * 1024 + 1025)
    _case(P, O, pr, 2)


@pytest.mark.parametrize("p", [31, 70])
def test_31_interweaved_columns(P, O, p):
    """q = 32: 528 Gram pairs per chain, 4 chains"""
    _case(P, O, _synthetic(P, p, _cols(p, 31), n=300, m=6), 4)


def test_32_interweaved_columns_are_refused(P, O):
    """design_set refuses p_locs = 32 (NNGP_ERR_ARG) and the context goes on:
    a design of 31 columns set on it afterwards passes its case."""
    from nngp_amd._lib import NNGP_ERR_ARG

    pr = _synthetic(P, 40, _cols(40, 31), n=300, m=6)
    inp = _chain_inputs(pr, 4)
    with _open(P, pr, 4, design=False) as ctx:
        with pytest.raises(P.NNGPError) as e:
            ctx.design_set(pr["X"], pr["first_obs"], list(range(32)))
        assert e.value.status == NNGP_ERR_ARG
        with pytest.raises(P.NNGPError):  # and no design was left behind
            ctx.design_mean_stats_chains(1, inp["b0"])
        ctx.design_set(pr["X"], pr["first_obs"], pr["locs_cols"])
        _check_against_numpy(O, pr, inp, _primitives_on(ctx, pr, inp, [0b1111]))


@pytest.fixture(scope="module")
def prob4(P):
    return _synthetic(P, 4, [3, 1])


@pytest.mark.parametrize("C", [1, 2, 4])
def test_chain_counts(P, O, prob4, C):
    _case(P, O, prob4, C)


def test_split_masks_of_four_chains(P, prob4):
    """0b1010 then 0b0101 == 0b1111, bitwise, and so in the other order"""
    inp = _chain_inputs(prob4, 4)
    batched = _primitives(P, prob4, inp, [0b1111])
    _assert_same(batched, _primitives(P, prob4, inp, [0b1010, 0b0101]))
    _assert_same(batched, _primitives(P, prob4, inp, [0b0101, 0b1010]))


def test_chains_outside_the_mask_keep_field_and_mu(P, prob4):
    """After a commit of all four chains, a commit of 0b1010 with other
    coefficients changes chains 1 and 3 and leaves the field and mu of chains 0
    and 2 bit for bit; statistics calls change no chain's state."""
    inp = _chain_inputs(prob4, 4)
    with _open(P, prob4, 4) as ctx:
        for k in range(4):
            ctx.select(k).factor(0, COV, CPS[k])
            ctx.set_field(inp["fields"][k])
        ctx.design_commit_chains(0b1111, inp["shift"], inp["bl_old"], inp["bl_new"], inp["b0_new"], inp["beta"])
        before = [(ctx.select(k).get_field(), ctx.get_mu()) for k in range(4)]
        ctx.design_mean_stats_chains(0b1010, inp["b0"])
        ctx.design_interweave_stats_chains(0b1010, inp["shift"], inp["bl_old"])
        ctx.design_commit_chains(0b1010, inp["shift"] + 1.0, inp["bl_new"], inp["bl_old"], inp["b0_new"] - 1.0,
                                 inp["beta"][::-1])
        after = [(ctx.select(k).get_field(), ctx.get_mu()) for k in range(4)]
    for k in range(4):
        for a, b, what in zip(before[k], after[k], ("field", "mu")):
            assert np.array_equal(a, b) == (k in (0, 2)), (k, what)
