"""The per-block / per-row gradient assertions of tests/_gradcheck.py bite where one tolerance over the whole flat gradient does not:
on the CPU, with torch's fp32 autograd of the nav network standing in for a kernel, a 0.1 % defect planted in one parameter block, one
ragged-tile column or one observation-gradient row passes  max|g - gref| <= 5e-6 max|gref|  (the form the chain-kernel tests had
alone) and fails assert_blocks / assert_rows."""
import types

import pytest
import torch

from _gradcheck import assert_blocks, assert_rows, pinned_reference, torch_activations
from visfly_amd.ppo import MlpPolicy

DIMS = {"state": 13, "target": 3}
M = 777


@pytest.fixture(scope="module")
def case():
    """policy, the pinned fp64 reference (computed once, never written to), the stand-in kernel's flat gradient and observation
    gradients: shapes and seeds of test_ppo_gpu.py::test_chain_backward_vs_torch_and_block_tile_kernel[nav, bptt, M = 777] -- the
    actor update of BPTT / SHAC: no value-head gradient, observation gradients wanted.  (There every block but the action head's is
    below 4e-3 of the largest entry; with a value-head gradient only pi:0 and pi:1 are.)"""
    pol = MlpPolicy(DIMS, {k: [128, 64] for k in DIMS}, [64, 64], [64, 64], "cpu", seed=9)
    g = torch.Generator().manual_seed(M)
    obs = {k: torch.randn((M, d), generator=g) for k, d in DIMS.items()}
    d_mean = torch.randn((M, 4), generator=g) / M
    net = pol.to_torch()
    saved = torch_activations(pol, net, obs)
    ref = pinned_reference(pol, obs, saved, d_mean, None, True, second_head=False)
    return pol, ref, ref.grad32.float(), {k: v.float() for k, v in ref.d_in32.items()}


def _layer(pol, src, dst):
    return next(ly for ly in pol.layers if ly.src == src and ly.dst == dst)


def _with_grad(ref, grad):
    """the reference with another flat gradient (and its fp32 rounding as torch's fp32 result)"""
    return types.SimpleNamespace(**{**vars(ref), "grad": grad, "grad32": grad.float().double()})


def _old_assertion_accepts(g, ref):
    return (g.double() - ref.grad).abs().max().item() <= 5e-6 * ref.grad.abs().max().item()


def test_unmodified_gradient_passes(case):
    pol, ref, g, d_in = case
    assert ref.units == M * (2 * (128 + 64) + 4 * 64) and ref.flips <= 1e-6 * ref.units
    assert _old_assertion_accepts(g, ref)
    err, dist = assert_blocks(pol, g, ref, "torch fp32")
    assert err == dist                                   # the stand-in IS torch's fp32 autograd
    for k in DIMS:
        assert_rows(d_in[k], ref.d_in[k], ref.d_in32[k], k)


@pytest.mark.parametrize("defect", ["extractor weight block", "pi bias block", "ragged column 12 of x:state:0"])
def test_a_defect_inside_one_block_passes_the_global_bound_and_fails_the_block_bound(case, defect):
    pol, ref, g, _ = case
    g = g.clone()
    if defect == "extractor weight block":
        ly = _layer(pol, "x:target:0", "feat")
        g[ly.w_off:ly.w_off + ly.K * ly.No] *= 1 + 1e-3
    elif defect == "pi bias block":
        ly = _layer(pol, "pi:0", "pi:1")
        g[ly.b_off:ly.b_off + ly.No] *= 1 + 1e-3
    else:
        ly = _layer(pol, "obs:state", "x:state:0")
        assert (ly.K, ly.No) == (13, 128)
        g[ly.w_off:ly.w_off + ly.K * ly.No].view(ly.No, ly.K)[:, 12] *= 1 + 1e-3
    assert _old_assertion_accepts(g, ref), "the planted defect is one the whole-gradient tolerance lets through"
    with pytest.raises(AssertionError, match=ly.dst):
        assert_blocks(pol, g, ref, defect)


def test_ragged_column_is_held_on_its_own_scale(case):
    """a column of the ragged tile far below the block's largest entry: the defect is under 2e-5 of the BLOCK and is still found"""
    pol, ref, g, _ = case
    ly = _layer(pol, "obs:state", "x:state:0")
    w = ref.grad[ly.w_off:ly.w_off + ly.K * ly.No].view(ly.No, ly.K)
    small = ref.grad.clone()
    small[ly.w_off:ly.w_off + ly.K * ly.No].view(ly.No, ly.K)[:, 12] *= 1e-3          # a reference whose column 12 is 1000 x smaller
    scaled = _with_grad(ref, small)
    g = small.float()
    col = g[ly.w_off:ly.w_off + ly.K * ly.No].view(ly.No, ly.K)[:, 12]
    col *= 1 + 1e-3
    assert 1e-3 * w[:, 12].abs().max().item() * 1e-3 < 2e-5 * w.abs().max().item()
    with pytest.raises(AssertionError, match="input column 12"):
        assert_blocks(pol, g, scaled, "small ragged column")


def test_a_block_no_gradient_reaches_must_be_left_alone(case):
    """the value trunk without a value-head gradient: exactly what was there before the call -- zeros, or the test's fill value"""
    pol, ref, g, _ = case
    vf = [ly for ly in pol.layers if ly.dst == "value" or ly.dst.startswith("vf:")]
    assert all(not bool(ref.grad[ly.w_off:ly.b_off + ly.No].any()) for ly in vf)
    filled = g.clone()
    for ly in vf:
        filled[ly.w_off:ly.b_off + ly.No] = 3.0
    assert_blocks(pol, filled, ref, "fill value kept", untouched=3.0)
    with pytest.raises(AssertionError, match="value"):
        assert_blocks(pol, filled, ref, "fill value where zeros were put")
    g = g.clone()
    g[vf[-1].b_off] = 1e-30
    with pytest.raises(AssertionError, match="value"):
        assert_blocks(pol, g, ref, "value trunk written")


def test_a_defect_in_one_row_of_an_observation_gradient_fails_the_row_bound(case):
    pol, ref, _, d_in = case
    got = d_in["state"].clone()
    row = int(ref.d_in["state"].abs().max(dim=1).values.argmin())       # the row with the smallest gradient: far below the tensor's max
    got[row] *= 1 + 1e-3
    want = ref.d_in["state"]
    with pytest.raises(AssertionError, match="1 rows outside"):
        assert_rows(got, want, ref.d_in32["state"], "state")
