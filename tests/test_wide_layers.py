"""Hidden layers up to 512 wide (the td policies' default net_arch [256, 256]): what needs no GPU -- MlpPolicy accepts them and plans
no one-launch path for them, the dispatch predicate of the vf_linear_* entry points, and the width-agnostic plumbing (to_torch,
reference-named state dict, archive) at these widths.  The kernels themselves: tests/test_wide_layers_gpu.py."""
import types
import warnings

import pytest
import torch
import torch.nn as nn

from visfly_amd import checkpoint
from visfly_amd.ppo import MlpPolicy

OBS = {"state": 13, "target": 3}


def _mlp(dims):
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    return nn.Sequential(*mods)


class _Extractor(nn.Module):
    def __init__(self, state, target):
        super().__init__()
        self.state_extractor = _mlp([13] + state)
        self.target_extractor = _mlp([3] + target)

    def forward(self, obs):
        return torch.cat([self.state_extractor(obs["state"]), self.target_extractor(obs["target"])], dim=-1)


class _Trunks(nn.Module):
    def __init__(self, feat, pi, vf):
        super().__init__()
        self.policy_net = _mlp([feat] + pi)
        self.value_net = _mlp([feat] + vf)


class _ReferenceShapedPolicy(nn.Module):
    """the module structure of the reference's actor-critic policy (SB3 attribute names), hand-built from nn.Sequential stacks"""

    def __init__(self, state, target, pi, vf):
        super().__init__()
        self.log_std = nn.Parameter(torch.full((4,), -0.5))
        self.features_extractor = _Extractor(state, target)
        self.pi_features_extractor = self.features_extractor
        self.vf_features_extractor = self.features_extractor
        self.mlp_extractor = _Trunks(state[-1] + target[-1], pi, vf)
        self.action_net = nn.Linear(pi[-1], 4)
        self.value_net = nn.Linear(vf[-1], 1)

    def forward(self, obs):
        f = self.features_extractor(obs)
        return self.action_net(self.mlp_extractor.policy_net(f)), self.value_net(self.mlp_extractor.value_net(f))


ARCHS = {
    "trunks_256": dict(state=[128, 64], target=[128, 64], pi=[256, 256], vf=[256, 256]),
    "extractor_256_128": dict(state=[256, 128], target=[256, 128], pi=[256, 256], vf=[256, 256]),
    "layer_512": dict(state=[128, 64], target=[96, 32], pi=[512, 64], vf=[64, 512]),
}


def _policy(a, seed=3):
    return MlpPolicy(OBS, {"state": a["state"], "target": a["target"]}, a["pi"], a["vf"], "cpu", seed=seed)


@pytest.mark.parametrize("name", list(ARCHS))
def test_wide_policy_constructs_and_runs_layer_by_layer(name):
    """layers above 128 are accepted (up to 512) and such a network gets no one-launch plan and no chain class: every consumer of
    `_plan is None` then takes the per-layer route"""
    pol = _policy(ARCHS[name])
    assert pol.wide and pol._plan is None and pol.chain_shape is None
    assert max(max(ly.K, ly.No) for ly in pol.layers) in (256, 512)
    assert pol.pack_map() == (None, None)
    assert pol.forward_act(None, None, None) is False and pol.forward_steps(None, 32, 2) is None
    assert pol.backward_data_supported(64) is False
    assert pol.ppo_update(None, None, None, None, None, None, None, None) is False
    assert pol.twin_q_update(None, None, None, 1) is False
    assert pol.n_params == sum(ly.K * ly.No + ly.No for ly in pol.layers) + 4


def test_narrow_policy_keeps_its_plan():
    pol = MlpPolicy(OBS, {"state": [128, 64], "target": [128, 64]}, [128, 128], [128, 128], "cpu")
    assert not pol.wide and pol._plan is not None and pol.chain_shape is not None


def test_513_is_still_refused():
    for kw in (dict(pi=[513], vf=[64]), dict(pi=[64], vf=[64, 513])):
        with pytest.raises(ValueError, match="up to 512"):
            MlpPolicy(OBS, {"state": [128, 64], "target": [128, 64]}, kw["pi"], kw["vf"], "cpu")
    with pytest.raises(ValueError, match="up to 512"):
        MlpPolicy(OBS, {"state": [513, 64], "target": [128, 64]}, [64], [64], "cpu")
    MlpPolicy(OBS, {"state": [512, 64], "target": [128, 64]}, [64], [64], "cpu")


def test_fallback_warning_names_the_wide_kernels():
    pol = _policy(ARCHS["trunks_256"])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pol._warn_fallback("forward")
        pol._warn_fallback("forward")
    assert len(w) == 1 and "wider than 128" in str(w[0].message) and "layer by layer" in str(w[0].message)


def test_dispatch_predicate():
    """the predicate the four vf_linear_* entry points dispatch on: up to 128 x 128 the weight-stationary kernels keep serving (so
    every earlier result keeps its bits), one past it on either side the streamed-operand kernels take over"""
    import __graft_entry__ as ge
    ge.build()
    from visfly_amd import _lib
    lib = _lib.lib()
    for K, No in [(128, 128), (128, 64), (64, 128), (1, 1), (13, 128)]:
        assert lib.vf_linear_is_wide(K, No) == 0
    for K, No in [(129, 128), (128, 129), (129, 1), (1, 129), (256, 256), (512, 512)]:
        assert lib.vf_linear_is_wide(K, No) == 1
    # the scratch query answers for both: partial blocks of No*K + No floats
    for M, K, No in [(1, 256, 256), (25600, 256, 256), (25600, 512, 512), (524288, 512, 512), (200, 130, 200), (25600, 128, 128)]:
        n = int(lib.vf_linear_bwd_scratch_floats(M, K, No))
        assert n > 0 and n % (No * K + No) == 0
        assert n * 4 <= 64 << 20, "scratch of one layer stays below 64 MiB"


@pytest.mark.parametrize("name", list(ARCHS))
def test_to_torch_agrees_with_a_hand_built_stack(name):
    a = ARCHS[name]
    pol = _policy(a)
    ref = _ReferenceShapedPolicy(a["state"], a["target"], a["pi"], a["vf"])
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in checkpoint.policy_state_dict(pol).items()}
    assert got == want
    assert checkpoint.load_policy_state_dict(pol, ref.state_dict()) == []
    obs = {"state": torch.randn(37, 13), "target": torch.randn(37, 3)}
    m0, v0 = ref(obs)
    m1, v1 = pol.to_torch()(obs)
    assert torch.equal(m0, m1) and torch.equal(v0, v1)
    assert torch.equal(pol.log_std.cpu(), ref.log_std.detach())


def test_archive_round_trip_keeps_shapes(tmp_path):
    a = ARCHS["extractor_256_128"]
    pol = _policy(a)
    n = pol.n_params
    tr = types.SimpleNamespace(policy=pol, exp_avg=torch.randn(n), exp_avg_sq=torch.rand(n), _opt_step=7, lr=5e-5,
                               betas=(0.9, 0.999), adam_eps=1e-8, weight_decay=1e-5, num_timesteps=12345, gamma=0.99)
    path = checkpoint.save(tr, str(tmp_path / "PPO_wide"))
    sd, osd, data = checkpoint.read_archive(path)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in checkpoint.policy_state_dict(pol).items()}
    assert sd["mlp_extractor.policy_net.2.weight"].shape == (256, 256)
    assert sd["features_extractor.state_extractor.0.weight"].shape == (256, 13)
    pol2 = _policy(a, seed=11)
    assert not torch.equal(pol2.flat, pol.flat)
    checkpoint.load_policy_state_dict(pol2, sd)
    assert torch.equal(pol2.flat[:pol2.n_params], pol.flat[:pol.n_params])


def test_td_policy_kwargs_accept_a_plain_list():
    """SB3's get_actor_critic_arch: a list net_arch is the actor's AND the critics' hidden sizes"""
    pk = checkpoint.policy_kwargs_from_reference(dict(net_arch=[256, 256], activation_fn="relu"), ["state"])
    assert pk["pi"] == [256, 256] and pk["vf"] == [256, 256]
    pk = checkpoint.policy_kwargs_from_reference(
        dict(net_arch=dict(pi=[256, 256], vf=[256, 256]), activation_fn="relu",
             features_extractor_kwargs=dict(net_arch=dict(state=dict(layer=[256, 128])))), ["state"])
    assert pk["extractor"] == {"state": [256, 128]} and pk["pi"] == [256, 256]
