"""The twin critic over a TWO-branch extractor on the register-chained kernels (visfly_amd/_jit.py: generated classes with NB = 2 and the
pass-through action tile; PREBUILD_CRITIC["critic_gate"] = SHAC's critic over StateGateExtractor on the racing envs, ["critic_nav"] = over
StateTargetExtractor on NavigationEnv; __graft_entry__.build() pre-builds both, so no test waits for a compiler):

1. forward, both Q heads and the flat parameter gradient against a float64 torch replica (MlpPolicy.to_torch(), torch's own concat);
2. the fused critic step (vf_twin_q_update_in3: one launch of the plugin's k_twin_q_update_chain) against the three-launch step;
3. forward_steps with three inputs against separate forward calls, bit for bit;
4. SHAC end to end, persistent launches against the launch-by-launch loop, bit for bit, with the critic on the plugin throughout;
5. one learn() iteration: every trainable critic layer moves, both branches included.

Row counts: 33 = one full 32-row tile + one row; 1000 = 31 full tiles + 8 rows (more than one wave, a ragged last one).
The default two-branch critic ([128, 64] x 2: 132 columns into qf0 / qf1) is no chain class and is not part of these tests."""
import os
import warnings

import pytest
import torch

from _gradcheck import assert_blocks, assert_blocks_agree, pinned_reference       # (what tests/test_chain_jit_gpu.py checks its classes with)
from _golden import ENV_DYN, RACING_DYN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CRITICS = ["critic_gate", "critic_nav"]


def make_critic(name, seed):
    """the critic SHAC builds (ortho_init=False, no log_std) -- the plugin's file is there BEFORE the policy asks for it"""
    from visfly_amd import _jit
    from visfly_amd.ppo import MlpPolicy
    dims, ext, pi, vf, heads, pas = _jit.PREBUILD_CRITIC[name]
    sh = _jit.shape_of(dims, ext, pi, vf, heads, pas)
    assert sh is not None and os.path.exists(_jit.path_of(sh)), "the build pre-compiles the two-branch critic classes"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pol = MlpPolicy(dims, ext, pi, vf, DEV, seed=seed, ortho_init=False, head_dims=heads, passthrough=pas, log_std_param=False)
    assert pol.chain_jit and pol.chain_shape == sh
    return pol, dims, ext


def critic_inputs(dims, M, seed):
    """random rows; the gate column holds integer indices 0..3 as float32 (what the racing envs write), the action lies in (-1, 1)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs = {k: torch.randn((M, d), device=DEV, generator=g) for k, d in dims.items()}
    if "gate" in obs:
        obs["gate"] = torch.randint(0, 4, (M, 1), device=DEV, generator=g).float()
    obs["action"] = torch.tanh(obs["action"])
    return obs, g


# ---- 1. forward and gradient against float64 torch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CRITICS)
def test_forward_and_gradient_vs_torch_float64(name):
    from visfly_amd import _lib
    lib = _lib.lib()
    M = 33
    pol, dims, ext = make_critic(name, 11)
    obs, g = critic_inputs(dims, M, M + 7)
    d_q0 = torch.randn((M, 1), device=DEV, generator=g) / M
    d_q1 = torch.randn((M, 1), device=DEV, generator=g) / M
    ref = pol.to_torch().double().to(DEV)
    q0r, q1r = ref({k: v.double() for k, v in obs.items()})
    ((q0r * d_q0.double()).sum() + (q1r * d_q1.double()).sum()).backward()
    gref = ref.flat_grad().to(DEV).float()[:pol.n_params]
    n0 = lib.vf_chain_plugin_launches()
    q0, q1 = pol.forward(obs)
    assert lib.vf_chain_plugin_launches() == n0 + 1, "the plugin served the forward"
    assert q0.shape == q1.shape == (M, 1)
    for got, want, what in ((q0, q0r, "Q1"), (q1, q1r, "Q2")):
        err = (got.double() - want).abs()
        bound = 1e-3 * want.abs() + 1e-5 * want.abs().max() + 1e-6
        print(f"{name} {what}: max abs err {err.max().item():.3e}, max |Q| {want.abs().max().item():.3e}")
        assert bool((err <= bound).all()), (name, what, err.max().item())
    # the saved feature rows: branch 0, branch 1, then the action columns (what the trunks' weight gradients read)
    feat = sum(v[-1] for v in ext.values())
    b = pol._buffers(M, 0)
    assert b["feat"].shape == (M, feat + 4) and torch.equal(b["feat"][:, feat:], obs["action"])
    # (fp32 sums of <= 64 terms against fp64: a few 1e-7 of the largest feature; 1e-5 leaves room for nothing but rounding)
    assert (b["feat"][:, :feat].double() - ref.acts["feat"][:, :feat]).abs().max().item() <= 1e-5 * ref.acts["feat"][:, :feat].abs().max().item()
    pin = pinned_reference(pol, obs, b, d_q0, d_q1, False)
    pol.grad.fill_(0.0)
    n1 = lib.vf_chain_plugin_launches()
    pol.backward(d_q0, d_q1, None)
    assert lib.vf_chain_plugin_launches() > n1, "the plugin's reverse chain ran"
    grad = pol.grad[:pol.n_params].clone()
    scale = gref.abs().max().item()
    err = (grad - gref).abs().max().item()
    print(f"{name}: flat gradient max abs err {err:.3e} of max |g| {scale:.3e}")
    assert scale > 0 and err <= 2e-4 * scale, (err, scale)
    assert_blocks(pol, grad, pin, f"two-branch twin critic {name} M={M}")           # every layer on its own scale
    # the gate branch's first layer gets a gradient although its column carries none back
    for ly in pol.layers:
        if not ly.frozen:
            assert bool(grad[ly.w_off:ly.w_off + ly.K * ly.No].any()), (ly.src, ly.dst)


# ---- 2. the fused critic step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [33, 1000])
@pytest.mark.parametrize("name", CRITICS)
def test_fused_critic_step_equals_the_three_launch_step(name, M):
    from visfly_amd import _lib
    from visfly_amd.ppo import _ptr
    L = _lib.lib()
    st = _lib.current_stream(torch.device(DEV))
    c, dims, _ = make_critic(name, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        obs, g = critic_inputs(dims, M, M)
        target = torch.randn(M, device=DEV, generator=g)
        out = {}
        for fused in (False, True):
            c.grad.fill_(0.0)
            loss = torch.empty(1, device=DEV)
            if fused:
                n0 = L.vf_chain_plugin_launches()
                assert c.twin_q_update(obs, target, loss, M) is True, "the two-branch critic class must run on the fused step"
                assert L.vf_chain_plugin_launches() == n0 + 1 and c._fused_twin_q is not False
            else:
                q0, q1 = c.forward(obs, save_activations=True)
                dq0, dq1 = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
                scr = torch.empty(int(L.vf_twin_q_loss_scratch_doubles(M)), dtype=torch.float64, device=DEV)
                _lib.check(L.vf_twin_q_loss(_ptr(q0.view(-1)), _ptr(q1.view(-1)), _ptr(target), _ptr(dq0), _ptr(dq1), _ptr(loss), scr.data_ptr(), M, M, st))
                c.backward(dq0.view(M, 1), dq1.view(M, 1), None)
                pin = pinned_reference(c, obs, c._buffers(M, 0), dq0.view(M, 1), dq1.view(M, 1), False)
            out[fused] = (float(loss), c.grad[:c.n_params].clone())
    (l0, g0), (l1, g1) = out[False], out[True]
    print(f"{name} M={M}: loss separate {l0:.9e} fused {l1:.9e}")
    assert abs(l0 - l1) <= 1e-6 * max(1.0, abs(l0)), (l0, l1)
    scale = g0.abs().max().item()
    print(f"{name} M={M}: max |fused - separate| {(g1 - g0).abs().max().item():.3e} of max |g| {scale:.3e}")
    assert scale > 0 and (g1 - g0).abs().max().item() <= 2e-6 * scale, ((g1 - g0).abs().max().item(), scale)
    assert_blocks_agree(c, g1, g0, 2e-6, f"two-branch critic step {name} M={M}")
    assert_blocks(c, g1, pin, f"two-branch critic step {name} M={M} fused")
    assert_blocks(c, g0, pin, f"two-branch critic step {name} M={M} separate")


# ---- 3. the target critic over a recorded horizon -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CRITICS)
def test_forward_steps_equals_separate_forwards(name):
    from visfly_amd import _lib
    lib = _lib.lib()
    m_step, n_steps = 64, 3
    pol, dims, _ = make_critic(name, 5)
    obs, _ = critic_inputs(dims, m_step * n_steps, 21)
    assert len(pol.obs_keys) == 3
    n0 = lib.vf_chain_plugin_launches()
    out = pol.forward_steps(obs, m_step, n_steps)
    assert out is not None and lib.vf_chain_plugin_launches() == n0 + 1, "one launch of the plugin over the three blocks"
    q0, q1 = out[0].clone(), out[1].clone()
    for s in range(n_steps):
        rows = slice(s * m_step, (s + 1) * m_step)
        a, b = pol.forward({k: v[rows].contiguous() for k, v in obs.items()}, save_activations=False)
        assert torch.equal(a.view(torch.int32), q0[rows].view(torch.int32)), (name, s, "Q1")
        assert torch.equal(b.view(torch.int32), q1[rows].view(torch.int32)), (name, s, "Q2")
    assert lib.vf_chain_plugin_launches() == n0 + 1 + n_steps


# ---- 4. / 5. SHAC -------------------------------------------------------------------------------------------------------------------
NAV_EXT = {"state": [64, 64], "target": [32]}


def shac_setup(config, N, max_episode_steps):
    """-> (env, policy_kwargs, name of the critic's class)"""
    import visfly_amd.envs as E
    if config == "racing2_gate":
        from test_gate_extractor_gpu import policy_kwargs, racing_env
        return racing_env("racing2", N, RACING_DYN, max_episode_steps=max_episode_steps), policy_kwargs(True), "critic_gate"
    spawn = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}}]}}
    env = E.NavigationEnv(num_agent_per_scene=N, seed=5, dynamics_kwargs=dict(ENV_DYN), device=DEV, max_episode_steps=max_episode_steps,
                          requires_grad=True, tensor_output=True, random_kwargs=spawn)
    pk = dict(features_extractor_class="StateTargetExtractor",
              features_extractor_kwargs={"net_arch": {k: {"layer": list(v)} for k, v in NAV_EXT.items()}},
              net_arch=dict(pi=[64], qf=[64]), activation_fn="relu", share_features_extractor=False)
    return env, pk, "critic_nav"


SHAC_CONFIGS = ["racing2_gate", "nav_target"]


@pytest.mark.parametrize("config", SHAC_CONFIGS)
def test_shac_persistent_launches_equal_the_loop_with_the_critic_on_the_plugin(config):
    from visfly_amd import _jit, _lib
    from visfly_amd.shac import SHAC
    lib = _lib.lib()
    N, H, steps = 1000, 8, 2
    res = []
    for fused in (True, False):
        env, pk, cname = shac_setup(config, N, 6)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            algo = SHAC(env, policy_kwargs=dict(pk), horizon=H, gradient_steps=steps, learning_rate=1e-3, seed=7)
            assert algo.policy.chain_jit and algo.critic.chain_jit and algo.critic_target.chain_jit
            assert algo.critic.chain_shape == _jit.prebuild_shape(cname) and len(algo.critic.obs_keys) == 3
            algo.fused_rollout = algo.fused_reverse = fused
            used = []
            orig = env.rollout_policy
            env.rollout_policy = lambda *a, **k: used.append(orig(*a, **k)) or used[-1]
            out = {}
            n0 = lib.vf_chain_plugin_launches()
            for it in range(3):
                algo._update()
                b = algo._buf
                for k in ("action", "reward", "done", "ep_done", "next_value", "returns"):
                    out[f"{k}{it}"] = b[k].clone()
                for k, v in b["obs"].items():
                    out[f"obs:{k}{it}"] = v.clone()
                out[f"grad{it}"] = algo.policy.grad.clone()
                out[f"loss{it}"] = algo._last_losses[0].clone().reshape(1)
                out[f"critic_loss{it}"] = algo._last_losses[1].clone().reshape(1)
            torch.cuda.synchronize()
            launches = lib.vf_chain_plugin_launches() - n0
            out["actor"], out["critic"], out["target"] = algo.policy.flat.clone(), algo.critic.flat.clone(), algo.critic_target.flat.clone()
        assert used == ([True] * 3 if fused else []), used
        assert algo.critic._fused_twin_q is not False, "the critic updates are the fused step"
        assert launches >= 3 * steps, launches
        bad = [str(x.message) for x in w if "vf_twin_q_update" in str(x.message) or "block-tile" in str(x.message) or "falling back" in str(x.message)]
        assert not bad, bad
        assert all(bool(torch.isfinite(v.float()).all()) for v in out.values())
        res.append(out)
        env.close()
    n_done = sum(int(res[0][f"done{it}"].sum()) for it in range(3))
    print(f"{config}: done flags in the three horizons: {n_done}")
    assert n_done > 0, "no episode ended inside the horizons"
    for k in res[0]:
        a, b = res[0][k], res[1][k]
        same = torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert same, f"{config}: {k} differs (max abs {float((a.float() - b.float()).abs().max()):.3e})"


# The critic loss is mse(returns, min(Q1, Q2)) (shac.py:267-270): a row's gradient goes to the head that IS the minimum and to that head's
# trunk only.  Two freshly initialised heads differ by a row-independent offset (their biases and their trunks' mean activations: nn.Linear's
# default init gives |mean Q1 - mean Q2| ~ 0.1-0.5) while Q varies by 0.02-0.09 over the rows, so for most seeds ONE head is the minimum on
# every row and the other trunk rightly gets no gradient in the first updates.  Measured with the float64 torch replica of the initial critic
# on the 512 rows of the first horizon, trainer seeds 0..29: one head takes every row for 13 of 30 seeds on RacingEnv2 (seed 4, the gate
# tests' seed, among them) and for 23 of 30 on NavigationEnv.  "Every layer moves" can only be asked where both heads are the minimum
# somewhere: the seeds below are, per configuration, the FIRST of 0..29 for which Q1 is the minimum on 25-75 % of those rows (350 / 512 and
# 195 / 512), and the test asserts that property on the rows of its own horizon before it asks for movement.
LEARN_SEEDS = {"racing2_gate": 21, "nav_target": 5}


@pytest.mark.parametrize("config", SHAC_CONFIGS)
def test_one_learn_iteration_moves_every_critic_layer(config):
    from visfly_amd import _lib
    from visfly_amd.shac import SHAC
    lib = _lib.lib()
    N, H = 64, 8
    env, pk, _ = shac_setup(config, N, 32)
    algo = SHAC(env, policy_kwargs=dict(pk), horizon=H, gradient_steps=2, learning_rate=1e-3, seed=LEARN_SEEDS[config])
    c = algo.critic
    assert c.chain_jit
    before = c.flat.clone()
    initial = c.to_torch().double().to(DEV)
    n0 = lib.vf_chain_plugin_launches()
    algo.learn(H * N)
    torch.cuda.synchronize()
    assert lib.vf_chain_plugin_launches() - n0 >= 2 and c._fused_twin_q is not False
    b = algo._buf
    with torch.no_grad():
        q0, q1 = initial({**{k: b["obs"][k].view(H * N, -1).double() for k in c.obs_keys[:2]}, "action": b["action"].view(H * N, 4).double()})
    first = int((q0 <= q1).sum())
    print(f"{config}: rows of the horizon on which Q1 / Q2 of the initial critic is the minimum: {first} / {H * N - first}")
    assert 0 < first < H * N, "one head is the minimum on every row: its twin's trunk gets no gradient, by the loss's definition"
    trainable = [ly for ly in c.layers if not ly.frozen]
    assert {ly.src for ly in trainable if ly.first} == {"obs:" + k for k in c.obs_keys[:2]}, "both branches are in the table"
    for ly in trainable:
        moved = [not torch.equal(before[o:o + n], c.flat[o:o + n]) for o, n in ((ly.w_off, ly.K * ly.No), (ly.b_off, ly.No))]
        assert moved == [True, True], (config, ly.src, ly.dst, moved)
    for ly in c.layers:
        if ly.frozen:         # the identity layer behind the trainable parameters stays the identity
            assert torch.equal(c.flat[ly.w_off:ly.w_off + ly.K * ly.No].view(ly.No, ly.K), torch.eye(ly.K, device=DEV))
    for p in (algo.policy, c, algo.critic_target):
        assert bool(torch.isfinite(p.flat).all()) and bool(torch.isfinite(p.grad).all())
    assert all(v == v and abs(v) != float("inf") for v in algo.logs.values() if isinstance(v, float))
    env.close()
