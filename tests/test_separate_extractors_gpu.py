"""Separate pi / vf feature extractors on the GPU: the two-wave chain kernels of such a network (csrc/vf_mlp_chain_sep.hpp: k_chain_forward_sep,
k_ppo_update_sep, served through the plugin of the shape) against the reference's fixture, torch in fp64, the layer-by-layer and the
block-tile kernels on the same layer table; that the two sides do not depend on each other, bit for bit; and PPO end to end.

Shapes: the smallest that cross every edge -- one branch per side / a critic with a second branch the actor does not read, different depths
and widths per role, a Tanh trunk; M over the partial last tile, the tile boundary and many tiles."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import test_separate_extractors as H
from _gradcheck import assert_blocks, assert_blocks_agree, pinned_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
from visfly_amd._jit import PREBUILD_SEP as SHAPES      # name -> (observation widths, pi extractor, pi, vf, vf extractor, activations); built ahead
CASES = ["sep_sym", "sep_asym", "sep_asym_tanh"]
ROWS = [1, 31, 33, 65, 1057]
# ... and the YAMLs' sizes on both sides, whose fused step runs the variant that keeps the ReLU masks as bits: two row counts
CASES_ROWS = [(n, M) for n in CASES for M in ROWS] + [("sep_default", 33), ("sep_default", 1057)]
_ACT = {1: "relu", 2: "tanh"}


def make(name, **kw):
    from visfly_amd.ppo import MlpPolicy
    dims, ext, pi, vf, vext, acts = SHAPES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pol = MlpPolicy(dims, ext, pi, vf, DEV, seed=9, activation=_ACT[acts[0]], vf_extractor=vext, **kw)
    assert pol.chain_jit and pol.sep, "the shape has a generated chain class"
    return pol, dims


def head_tol(pol, head, want):
    """the forward tolerance of the layer entry points (tests/_gradcheck.py: 1e-5 sqrt(K), relative to 1 + the row's largest |z|) for
    the rows `want` of head `head`"""
    K = next(ly.K for ly in pol.layers if ly.dst == head)
    return 1e-5 * np.sqrt(K) * (1 + want.abs().reshape(want.shape[0], -1).max(dim=1, keepdim=True).values)


def assert_heads(pol, mean, value, m0, v0, what):
    for head, got, want in (("mean", mean, m0), ("value", value.reshape(-1, 1), v0.reshape(-1, 1))):
        err = (got.double() - want.double()).abs()
        tol = head_tol(pol, head, want.double())
        print(f"{what} {head}: worst err / tolerance {(err / tol).max().item():.3e}")
        assert bool((err <= tol).all()), (what, head, (err / tol).max().item())


@pytest.fixture(scope="module")
def lib():
    from visfly_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("form", list(H.FORMS))
def test_forward_of_the_plugin_equals_the_reference_fixture(form, lib):
    pol, fx = H.load_fixture(form, device=DEV)
    assert pol.chain_jit
    obs = {k: torch.from_numpy(fx["obs_" + k]).to(DEV) for k in pol.obs_keys}
    n0 = lib.vf_chain_plugin_launches()
    mean, value = pol.forward(obs)
    assert lib.vf_chain_plugin_launches() == n0 + 1, "the plugin served the forward"
    # the reference's evaluate_actions: values and the squashed Gaussian's log-prob of the recorded actions
    actions = torch.from_numpy(fx["actions"]).to(DEV)
    lp = H.squashed_log_prob(mean.double(), pol.log_std.double(), actions.double())
    v64 = torch.from_numpy(fx["values64"]).to(DEV)
    net = pol.to_torch().double().to(DEV)
    m0, v0 = net({k: v.double() for k, v in obs.items()})
    assert_heads(pol, mean, value, m0, v64, f"fixture {form}")
    assert (v0.reshape(-1) - v64).abs().max().item() <= 4 * np.abs(fx["values32"].astype(np.float64) - fx["values64"]).max()
    # log-prob: the head tolerance carried through d log_prob / d mean = (g - mean) / std^2, per row
    std = pol.log_std.double().exp()
    g = torch.atanh(actions.double().clamp(-1 + 1.2e-7, 1 - 1.2e-7))
    slope = ((g - m0).abs() / std ** 2).sum(dim=1)
    tol = head_tol(pol, "mean", m0).reshape(-1) * slope + 4 * np.abs(fx["log_prob32"].astype(np.float64) - fx["log_prob64"]).max()
    err = (lp - torch.from_numpy(fx["log_prob64"]).to(DEV)).abs()
    assert bool((err <= tol).all()), (err / tol).max().item()


@pytest.mark.parametrize("name,M", CASES_ROWS)
def test_forward_vs_torch_layer_by_layer_and_block_tile(name, M, lib):
    pol, dims = make(name)
    g = torch.Generator(device=DEV).manual_seed(M)
    obs = {k: torch.randn((M, d), device=DEV, generator=g) for k, d in dims.items()}
    ref = pol.to_torch().double().to(DEV)
    m0, v0 = ref({k: v.double() for k, v in obs.items()})
    n0 = lib.vf_chain_plugin_launches()
    mean, value = pol.forward(obs)
    mean, value = mean.clone(), value.clone()
    assert lib.vf_chain_plugin_launches() == n0 + 1, "the plugin served the forward"
    assert_heads(pol, mean, value, m0, v0, f"{name} M={M} plugin vs fp64")
    mean_pi, none = pol.forward(obs, save_activations=False, need_value=False)
    assert none is None and lib.vf_chain_plugin_launches() == n0 + 2 and torch.equal(mean_pi, mean), "role 0 alone: the same mean, bit for bit"
    saved = {k: v.clone() for k, v in pol._buffers(M, 0).items() if isinstance(v, torch.Tensor) and k.split(":")[0] in ("x", "vx", "pi", "vf", "feat", "vfeat")}
    assert {"feat", "vfeat"} <= set(saved)
    for path in ("layer by layer", "block tile"):
        if path == "layer by layer":
            pol.fused = False
        else:
            lib.vf_chain_plugin_set_enabled(0)
        try:
            m1, v1 = pol.forward(obs)
            assert lib.vf_chain_plugin_launches() == n0 + 2, path
            assert_heads(pol, mean, value, m1, v1, f"{name} M={M} plugin vs {path}")
            assert_heads(pol, m1, v1, m0, v0, f"{name} M={M} {path} vs fp64")
            # every saved activation (what the weight gradients read) equals that path's
            b = pol._buffers(M, 0)
            for k, v in saved.items():
                assert (b[k] - v).abs().max().item() <= 4e-6 * max(v.abs().max().item(), 1e-3), (path, k)
        finally:
            pol.fused = True
            lib.vf_chain_plugin_set_enabled(1)


def _minibatch(pol, dims, B, T=None):
    g = torch.Generator(device=DEV).manual_seed(B)
    T = T or B
    obs = {k: torch.randn((T, d), device=DEV, generator=g) for k, d in dims.items()}
    mean, _ = pol.forward(obs)
    actions = torch.tanh(mean + 0.7 * torch.randn((T, 4), device=DEV, generator=g)).contiguous()
    old_lp = H.squashed_log_prob(mean, pol.log_std, actions).float() + 0.3 * torch.randn(T, device=DEV, generator=g)
    return obs, actions, old_lp.contiguous(), torch.randn(B, device=DEV, generator=g), torch.randn(T, device=DEV, generator=g), g


@pytest.mark.parametrize("name,B", CASES_ROWS)
def test_fused_step_equals_separate_launches_and_the_fp64_network(name, B, lib):
    """vf_ppo_update on the plugin (k_ppo_update_sep: per role forward + its part of the loss + reverse chain, one launch) vs forward /
    vf_ppo_loss / backward on the generic kernels, both against the pinned fp64 reference; statistics; untouched= fill"""
    from visfly_amd import _lib
    pol, dims = make(name, log_std_init=-0.3)
    obs, actions, old_lp, adv, ret, _ = _minibatch(pol, dims, B)
    scratch = torch.zeros(16 * max(1024, (B + 31) // 32), device=DEV)
    st = _lib.current_stream(torch.device(DEV))
    res = {}
    for fused in (True, False):
        stats = torch.zeros(16, device=DEV)
        pol.grad.fill_(3.0)
        cfg = _lib.PpoLossCfg(0.2, 0.01, 0.5, 1.0 / B, pol.grad.data_ptr() + 4 * pol.log_std_off, None)
        n0 = lib.vf_chain_plugin_launches()
        if fused:
            assert pol.ppo_update(obs, actions, old_lp, adv, ret, cfg, stats, scratch)
            assert lib.vf_chain_plugin_launches() == n0 + 1, "the plugin served the fused step"
        else:
            lib.vf_chain_plugin_set_enabled(0)
            try:
                m, v = pol.forward(obs)
                d_mean, d_value = torch.empty((B, 4), device=DEV), torch.empty(B, device=DEV)
                _lib.check(lib.vf_ppo_loss(m.data_ptr(), v.data_ptr(), pol.log_std.data_ptr(), actions.data_ptr(), old_lp.data_ptr(),
                                           adv.data_ptr(), ret.data_ptr(), d_mean.data_ptr(), d_value.data_ptr(), stats.data_ptr(), B,
                                           C.byref(cfg), scratch.data_ptr(), st))
                pol.backward(d_mean, d_value, None)
            finally:
                lib.vf_chain_plugin_set_enabled(1)
            assert lib.vf_chain_plugin_launches() == n0
            pin = pinned_reference(pol, obs, pol._buffers(B, 0), d_mean, d_value, False)     # the loss kernel's head gradients as the seed
        res[fused] = (pol.grad.clone(), stats.clone())
    (g1, s1), (g0, s0) = res[True], res[False]
    assert torch.allclose(s1[:9], s0[:9], rtol=2e-5, atol=1e-6 * max(1.0, s0[:9].abs().max().item())), (s1, s0)
    assert torch.allclose(g1[pol.log_std_off:], g0[pol.log_std_off:], rtol=1e-4, atol=1e-7)
    assert_blocks_agree(pol, g1, g0, 5e-6, f"sep ppo update {name} B={B}")
    assert_blocks(pol, g1, pin, f"sep ppo update {name} B={B} fused", untouched=3.0)
    assert_blocks(pol, g0, pin, f"sep ppo update {name} B={B} separate", untouched=3.0)


@pytest.mark.parametrize("B", [33, 1057])
@pytest.mark.parametrize("name", ["sep_sym", "sep_asym"])
def test_fused_step_on_an_indexed_minibatch(name, B, lib):
    """vf_ppo_loss_cfg.row_index: the same statistics and gradient, bit for bit, as the call on the gathered rows; the observation rows
    are left in minibatch order for the weight gradients (an input both sides read: by role 0; one only the critic reads: by role 1)"""
    from visfly_amd import _lib
    pol, dims = make(name, log_std_init=-0.3)
    T = 3 * B + 17
    obs, actions, old_lp, adv, ret, g = _minibatch(pol, dims, B, T)
    rows = torch.randperm(T, device=DEV, generator=g)[:B].contiguous()
    scratch = torch.zeros(16 * max(1024, (B + 31) // 32), device=DEV)
    res = {}
    for indexed in (True, False):
        stats = torch.zeros(16, device=DEV)
        pol.grad.fill_(3.0)
        cfg = _lib.PpoLossCfg(0.2, 0.01, 0.5, 1.0 / B, pol.grad.data_ptr() + 4 * pol.log_std_off, None)
        n0 = lib.vf_chain_plugin_launches()
        if indexed:
            assert pol.ppo_update(obs, actions, old_lp, adv, ret, cfg, stats, scratch, row_index=rows)
            copies = {k: pol._buffers(B, 0)["obs:" + k].clone() for k in dims}
        else:
            o = {k: v[rows].contiguous() for k, v in obs.items()}
            assert pol.ppo_update(o, actions[rows].contiguous(), old_lp[rows].contiguous(), adv, ret[rows].contiguous(), cfg, stats, scratch)
            for k in dims:
                assert torch.equal(copies[k], o[k]), k
        assert lib.vf_chain_plugin_launches() == n0 + 1
        res[indexed] = (pol.grad.clone(), stats.clone())
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][0], res[False][0])
    b = pol._buffers(B, 0)
    pin = pinned_reference(pol, o, b, b["d:mean"], b["d:value"], False)
    assert_blocks(pol, res[False][0], pin, f"indexed sep ppo update {name} B={B}", untouched=3.0)


@pytest.mark.parametrize("name", CASES + ["sep_default"])
def test_the_two_sides_are_independent_bit_for_bit(name, lib):
    from visfly_amd import _lib
    B = 1057
    pol, dims = make(name, log_std_init=-0.3)
    obs, actions, old_lp, adv, ret, g = _minibatch(pol, dims, B)
    scratch = torch.zeros(16 * max(1024, (B + 31) // 32), device=DEV)
    blocks = {s: [(ly.w_off, ly.b_off + ly.No) for ly in pol.layers if ly.side == s] for s in ("pi", "vf")}
    assert all(blocks.values()) and sum(hi - lo for s in blocks for lo, hi in blocks[s]) == pol.log_std_off

    def run():
        stats = torch.zeros(16, device=DEV)
        pol.grad.fill_(3.0)
        cfg = _lib.PpoLossCfg(0.2, 0.01, 0.5, 1.0 / B, pol.grad.data_ptr() + 4 * pol.log_std_off, None)
        n0 = lib.vf_chain_plugin_launches()
        mean, value = pol.forward(obs)
        mean, value = mean.clone(), value.clone()
        assert pol.ppo_update(obs, actions, old_lp, adv, ret, cfg, stats, scratch)
        assert lib.vf_chain_plugin_launches() == n0 + 2
        return mean, value, pol.grad.clone()

    flat0 = pol.flat.clone()
    m0, v0, g0 = run()
    for moved, kept in (("vf", "pi"), ("pi", "vf")):
        pol.flat.copy_(flat0)
        for lo, hi in blocks[moved]:          # every parameter of that side
            pol.flat[lo:hi] += 0.05 * torch.randn(hi - lo, device=DEV, generator=g)
        pol.mark_updated()
        m1, v1, g1 = run()
        same, other = (m1, m0) if kept == "pi" else (v1, v0), (v1, v0) if kept == "pi" else (m1, m0)
        assert torch.equal(*same), f"perturbing the {moved} side moved the {kept} side's head"
        assert not torch.equal(*other)
        for lo, hi in blocks[kept]:
            assert torch.equal(g1[lo:hi], g0[lo:hi]), f"perturbing the {moved} side moved a gradient block of the {kept} side"
        assert any(not torch.equal(g1[lo:hi], g0[lo:hi]) for lo, hi in blocks[moved])
        # the log_std gradient belongs to the pi side
        assert torch.equal(g1[pol.log_std_off:], g0[pol.log_std_off:]) == (kept == "pi")


def _env(N, seed=1):
    from visfly_amd.envs import NavigationEnv
    from _golden import ENV_DYN
    return NavigationEnv(num_agent_per_scene=N, seed=seed, dynamics_kwargs=dict(ENV_DYN), device=DEV, max_episode_steps=6, tensor_output=True)


PPO_KW = dict(n_steps=8, batch_size=160, n_epochs=2, learning_rate=3e-4, seed=3)


@pytest.mark.parametrize("form", list(H.FORMS))
def test_ppo_learns_on_the_chain_path_like_layer_by_layer(form, lib):
    """one learn() iteration of PPO on NavigationEnv with either reference form: the plugin's kernels against the same trainer forced
    layer by layer; the roll-out runs launch by launch and says so once"""
    from visfly_amd import _lib
    from visfly_amd.ppo import PPO
    flats = []
    for chain in (True, False):
        env = _env(64)
        _lib._warned.discard("vf_ppo_rollout")
        n0 = lib.vf_chain_plugin_launches()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ppo = PPO(env, policy_kwargs=H.reference_kwargs(form), **PPO_KW)
            pol = ppo.policy
            assert pol.sep and pol.chain_jit and pol.spec["vf_extractor"] == H.FORMS[form][3] and ppo.obs_keys == ["state", "target"]
            if not chain:
                pol.fused = pol.fused_backward = False
            ppo.learn(8 * 64)
            ppo.collect_rollouts()
        torch.cuda.synchronize()
        served = lib.vf_chain_plugin_launches() - n0
        said = [x for x in w if "vf_ppo_rollout" in str(x.message)]
        if chain:
            assert len(said) == 1 and "one launch per step" in str(said[0].message), [str(x.message) for x in w]
            assert not [x for x in w if "block-tile" in str(x.message)]
            # 2 epochs x 4 minibatches (160, 160, 160, 32 rows) fused steps + the forwards of two roll-outs
            assert served >= 8 + 2 * 8, served
        else:
            assert served == 0
        assert not ppo.fused_rollout
        flats.append(pol.flat.clone())
        env.close()
    d = (flats[0] - flats[1]).abs().max().item()
    print(f"{form}: parameters after one iteration, chain vs layer by layer: {d:.3e}")
    assert d <= 2e-5, d


def test_collect_rollouts_matches_the_replay_of_its_own_actions(lib):
    """launch by launch: a second trainer on a second env of the same seed, stepped with the first one's recorded actions, fills the same
    observation / value / reward rows and the same advantages, bit for bit"""
    from visfly_amd.ppo import PPO
    bufs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = PPO(_env(64), policy_kwargs=H.reference_kwargs("asym"), **PPO_KW)
        a.collect_rollouts()
        b = PPO(_env(64), policy_kwargs=H.reference_kwargs("asym"), **PPO_KW)
        b.collect_rollouts(replay=dict(eps=torch.zeros_like(a.buf.actions), actions=a.buf.actions.clone()))
    torch.cuda.synchronize()
    for k in a.obs_keys:
        assert torch.equal(a.buf.obs[k], b.buf.obs[k]), k
    for f in ("values", "rewards", "episode_starts", "advantages", "returns"):
        assert torch.equal(getattr(a.buf, f), getattr(b.buf, f)), f
    assert bool(a.buf.episode_starts[1:].any()), "episodes ended inside the roll-out (TimeLimit bootstrap through the critic's own extractor)"
    # the deterministic head of the replay: a = tanh(mean) where eps = 0
    mean, value = b.policy.forward({k: b.buf.obs[k][3] for k in b.obs_keys}, save_activations=False)
    assert torch.equal(value.reshape(-1), b.buf.values[3])


@pytest.mark.parametrize("form", list(H.FORMS))
def test_save_load_predict_and_evaluate(form, tmp_path, lib):
    import json
    import os
    from visfly_amd import checkpoint
    from visfly_amd.evaluate import evaluate_policy
    from visfly_amd.ppo import PPO
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ppo = PPO(_env(64), policy_kwargs=H.reference_kwargs(form), **PPO_KW)
        ppo.learn(8 * 64)
        path = ppo.save(str(tmp_path / "sep"))
        sd, opt, data = checkpoint.read_archive(path)
        gold = json.load(open(os.path.join(H.GOLD, "sep_keys.json")))[form]
        assert {k: list(v.shape) for k, v in sd.items()} == gold["shapes"] and data["policy_spec"]["vf_extractor"] == H.FORMS[form][3]
        again = PPO.load(path, _env(64))
        assert again.policy.spec == ppo.policy.spec and torch.equal(again.policy.flat, ppo.policy.flat)
        assert torch.equal(again.exp_avg, ppo.exp_avg) and again._opt_step == ppo._opt_step == 8
        # a trainer whose network shares its extractor refuses the archive before a tensor is compared, as for activations
        shared = PPO(_env(64), policy_kwargs=dict(H.reference_kwargs("sym"), share_features_extractor=True), **PPO_KW)
        before = shared.policy.flat.clone()
        with pytest.raises(ValueError, match="vf_extractor"):
            shared.set_parameters(path)
        assert torch.equal(shared.policy.flat, before)
        obs = again.env.reset()
        act, _ = again.predict(obs, deterministic=True)
        mean, value = again.policy.forward({k: obs[k].contiguous() for k in again.obs_keys}, save_activations=False)
        assert torch.allclose(act, torch.tanh(mean), rtol=0, atol=2e-6) and torch.equal(again.predict_values(obs), value.reshape(-1))
        res = evaluate_policy(again, _env(33, seed=11))
        loop = evaluate_policy(again, _env(33, seed=11), persistent=False)
    assert res.path == "loop" and torch.equal(res.ep_return, loop.ep_return) and int(res.ep_length.min()) >= 1
