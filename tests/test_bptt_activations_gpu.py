"""BPTT with Tanh / ELU / LeakyReLU actors (MTDPolicy takes any activation_fn, td_policies.py:297): both of BPTT's actors -- the one-head
MlpPolicy actor and the reference's two-head Actor -- through every path a horizon takes.  The per-step path against a float64 torch replica
and against the torch.autograd-scheduled path; the two persistent launches (the BPTT plugin of a generated class that carries the
activation, visfly_amd/_jit.py) against the launch-by-launch loop, bit for bit; one optimiser step; the archives; and one iteration of the
reference's own BPTT.learn with a Tanh actor (tests/golden/bptt_loop_hover_tanh.npz, tools/gen_bptt_act.py).  The networks are the ones
__graft_entry__.build() pre-builds (_jit.PREBUILD_ACT / PREBUILD_BPTT), so no test waits for a compiler."""
import ast
import os

import numpy as np
import pytest
import torch

from _golden import ENV_DYN, RACING_DYN, assert_bits_equal, consts_of, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = ["Tanh", "ELU", "LeakyReLU"]
KIND = {"ReLU": 1, "Tanh": 2, "ELU": 3, "LeakyReLU": 4}
ACTORS = [None, "MultiInputPolicy"]      # BPTT's one-head MlpPolicy actor / the reference's two-head Actor


def policy_kwargs(act, policy, sizes=([64, 64, 32], [32])):
    """the reference's policy_kwargs: `sizes` = (extractor layers, trunk layers); the defaults are the pre-built sac_hover / pi_hover shapes"""
    ext, trunk = sizes
    return dict(features_extractor_class="StateExtractor", features_extractor_kwargs={"net_arch": {"state": {"layer": list(ext)}}},
                net_arch=dict(pi=list(trunk), qf=list(trunk)) if policy else dict(pi=list(trunk), vf=list(trunk)), activation_fn=act)


def hover(N, max_episode_steps=7, seed=5, **kw):
    from visfly_amd.envs import HoverEnv
    return HoverEnv(num_agent_per_scene=N, seed=seed, dynamics_kwargs=dict(ENV_DYN), device=DEV, tensor_output=True, requires_grad=True,
                    max_episode_steps=max_episode_steps, **kw)


def racing(N, max_episode_steps=7, seed=5):
    from visfly_amd.envs import RacingEnv
    return RacingEnv(num_agent_per_scene=N, seed=seed, dynamics_kwargs=dict(RACING_DYN), device=DEV, tensor_output=True, requires_grad=True,
                     max_episode_steps=max_episode_steps)


def make(env, act, policy, **kw):
    from visfly_amd.bptt import BPTT
    kw.setdefault("policy_kwargs", policy_kwargs(act, policy))
    algo = BPTT(env, policy=policy, learning_rate=1e-3, **kw)
    assert (algo.policy.act, algo.policy.ext_act) == (KIND[act], 1) and algo.reference_actor == (policy is not None)
    assert {ly.relu for ly in algo.policy.layers if ly.dst.startswith(("pi:", "vf:"))} == {KIND[act]}
    return algo


# ---- the per-step path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [([64, 64, 32], [32]), ([48], [40, 24])], ids=["chain", "tile"])
@pytest.mark.parametrize("policy", ACTORS, ids=["one_head", "two_heads"])
@pytest.mark.parametrize("act", ACTS)
def test_policy_forward_and_gradients_vs_torch(act, policy, sizes):
    """forward, observation gradient and parameter gradients of the actor BPTT builds against a float64 torch replica of the same weights
    (MlpPolicy.to_torch: torch.nn's own Tanh / ELU / LeakyReLU), 33 rows: two 16-row tiles and one row of a third.  `chain`: a generated
    register-chained class with the activation; `tile`: widths no chain class covers -- the block-tile / per-layer kernels.  The one-head
    actor runs under torch.autograd (PolicyFunction, what use_autograd=True schedules), the two-head actor through forward / backward as
    the reverse sweep calls them.  Tolerances: those of test_bptt_gpu.py::test_policy_function_input_and_param_grads_vs_torch."""
    from visfly_amd.bptt import PolicyFunction
    N = 33
    env = hover(N)
    algo = make(env, act, policy, policy_kwargs=policy_kwargs(act, policy, sizes), horizon=4)
    pol = algo.policy
    assert bool(pol.chain_jit) == (sizes[1] == [32])
    ref = pol.to_torch().double()
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (env.reset()["state"].detach() + 0.3 * torch.randn((N, 13), device=DEV, generator=g)).contiguous()
    w0, w1 = torch.randn((N, 4), device=DEV, generator=g), torch.randn((N, pol.head_dims[1]), device=DEV, generator=g)
    pol.grad.zero_()
    if policy is None:
        xg = x.clone().requires_grad_(True)
        anchor = torch.zeros(1, device=DEV, requires_grad=True)
        mean = PolicyFunction.apply(pol, ["state"], anchor, xg)
        (mean * w0).sum().backward()
        heads, d_x = [mean.detach()], xg.grad
    else:
        mu, ls = pol.forward({"state": x}, slot=0)
        heads = [mu.clone(), ls.clone()]
        d_x = pol.backward(w0.contiguous(), w1.contiguous(), None, accumulate=True, need_input_grad=True, slot=0)["state"]
    xr = x.cpu().double().requires_grad_(True)
    out = ref({"state": xr})
    loss = (out[0] * w0.cpu().double()).sum() + ((out[1] * w1.cpu().double()).sum() if policy else 0.0)
    loss.backward()
    close = lambda a, b: torch.allclose(a.cpu().double(), b, rtol=1e-3, atol=1e-5 * float(b.abs().max()) + 1e-6)
    for got, want, what in zip(heads, out, ("first head", "second head")):
        print(f"{act} {what}: max abs err {float((got.cpu().double() - want.detach()).abs().max()):.2e} of {float(want.abs().max()):.2e}")
        assert close(got, want.detach()), what
    print(f"{act} d obs: max abs err {float((d_x.cpu().double() - xr.grad).abs().max()):.2e} of {float(xr.grad.abs().max()):.2e}")
    assert close(d_x, xr.grad)
    gref = ref.flat_grad().double()
    err, scale = float((pol.grad.cpu().double() - gref).abs().max()), float(gref.abs().max())
    print(f"{act} parameter gradient: max abs err {err:.2e} of {scale:.2e}")
    assert scale > 0 and err <= 2e-4 * scale
    env.close()


@pytest.mark.parametrize("kind", ["hover", "racing"])
@pytest.mark.parametrize("act", ACTS)
def test_reverse_sweep_equals_autograd_path(act, kind):
    """the launch-by-launch reverse sweep (one activation slot per step, deferred weight gradient) against the torch.autograd-scheduled
    path over the same kernels, as test_bptt_gpu.py::test_reverse_sweep_equals_autograd_path does for ReLU and at its tolerance: hover
    (bodyrate) and racing (thrust), 37 agents, H = 6, episodes of 4 steps so that ends fall inside the horizon.  (The persistent launches
    are switched off here: they are held to this sweep bit for bit below.)"""
    grads, losses = [], []
    for use_autograd in (True, False):
        env = hover(37, max_episode_steps=4) if kind == "hover" else racing(37, max_episode_steps=4)
        algo = make(env, act, None, horizon=6, seed=1)
        algo.use_autograd = use_autograd
        algo.fused_rollout = algo.fused_reverse = False
        loss = algo._grad_autograd() if use_autograd else algo._grad_reverse_sweep()
        grads.append(algo.policy.grad.clone())
        losses.append(float(loss))
        assert bool(env._tape_done[:6].any()), "no episode ended inside the horizon"
        env.close()
    g0, g1 = grads
    assert abs(losses[0] - losses[1]) <= 1e-6 * max(1.0, abs(losses[0]))
    scale = g0.abs().max().item()
    print(f"{act} {kind}: max abs diff {(g0 - g1).abs().max().item():.2e} of {scale:.2e}")
    assert scale > 0 and (g0 - g1).abs().max().item() <= 2e-5 * scale, ((g0 - g1).abs().max().item(), scale)


# ---- the persistent launches --------------------------------------------------------------------------------------------------
def _plugin(act, policy, cfg):
    """(shape, cache key, path) of the pre-built BPTT plugin of the test networks"""
    from visfly_amd import _jit
    name = ("sac_hover_" if policy else "pi_hover_") + {"Tanh": "tanh", "ELU": "elu", "LeakyReLU": "leaky"}[act]
    assert (name, cfg) in _jit.PREBUILD_BPTT
    sh = _jit.prebuild_shape(name)
    return sh, (sh, ("bptt",) + cfg), _jit.path_of(sh, ("bptt",) + cfg)


@pytest.mark.parametrize("kind,act,policy,N", [("hover", a, p, n) for a in ACTS for p in ACTORS for n in (5, 1000)] +
                         [("racing", "Tanh", "MultiInputPolicy", 1000)],
                         ids=lambda v: {None: "one_head", "MultiInputPolicy": "two_heads"}.get(v, str(v)))
def test_persistent_launches_equal_the_loop(kind, act, policy, N):
    """vf_bptt_rollout / vf_bptt_reverse of a generated class with the activation against the launch-by-launch sweep: observations,
    actions, rewards, done flags, the tape, every saved activation and layer gradient of every slot, the loss rows and the flat parameter
    gradient are bit-identical (the bound of test_bptt_gpu.py::test_persistent_launches_with_the_reference_actor_equal_the_loop).  5 agents:
    less than a wave; 1000: 63 tiles of 16 rows, the last one ragged.  H = 8, episodes of 5 steps.  The BPTT plugin is the pre-built one:
    its file is there before the trainer exists, the plugin cache records that file, and nothing rewrote it."""
    from visfly_amd import _jit, _lib
    H = 8
    cfg = (0, 1, 0, True) if kind == "hover" else (2, 0, 0, True)
    sh, key, path = _plugin(act, policy, cfg)
    assert os.path.exists(path), f"{path}: not pre-built (__graft_entry__.build())"
    mtime = os.path.getmtime(path)
    res = []
    for fused in (True, False):
        env = hover(N, max_episode_steps=5) if kind == "hover" else racing(N, max_episode_steps=5)
        algo = make(env, act, policy, horizon=H, seed=9)
        assert algo.policy.chain_shape == sh and algo.policy.chain_jit
        algo.fused_rollout = algo.fused_reverse = fused
        used, rev_used, rewards = [], [], []
        rr = torch.zeros((H, N), device=DEV)
        orig, orig_rev, orig_step = env.rollout_policy, env.reverse_policy, env._step_no_grad
        env.rollout_policy = lambda *a, **k: used.append(orig(*a, reward_rows=rr, **k)) or used[-1]
        env.reverse_policy = lambda *a, **k: rev_used.append(orig_rev(*a, **k)) or rev_used[-1]

        def step(*a, **k):
            o = orig_step(*a, **k)
            rewards.append(o[1].clone())
            return o
        env._step_no_grad = step
        n0 = _lib.lib().vf_chain_plugin_launches()
        loss = algo._grad_reverse_sweep()
        assert used == ([True] if fused else []) and rev_used == used, (used, rev_used)
        if fused:
            assert _lib.lib().vf_chain_plugin_launches() >= n0 + 2 and _jit._loaded.get(key) == path
        live = lambda x: x.transpose(-3, -4).reshape(*x.shape[:-4], x.shape[-3], -1, 4)[..., :N, :].clone()
        blk = algo.policy._slot_blocks[N][1]
        out = {"loss": loss.clone(), "loss_rows": algo._horizon["loss_vec"].clone(), "grad": algo.policy.grad.clone(),
               "action": algo._horizon["actions"].clone(), "reward": rr.clone() if fused else torch.stack(rewards),
               "done": env._tape_done[:H].clone(), "tape": live(env._tape[:H]), "slab": live(env._slab), "adj": live(env._adj),
               "obs": env.get_observation()["state"].clone()}
        # observations of every slot, saved activations and layer gradients; the two-head actor: both trunks and both heads (the one-head
        # actor's horizon never runs the value trunk, and its mean stays inside the launch that applies the action head)
        for name in ["obs:state", "x:state:0", "x:state:1", "feat", "pi:0", "g:x:state:0", "g:x:state:1", "g:feat", "g:pi:0"] + (
                ["vf:0", "mean", "value", "g:vf:0"] if policy else []):
            out[name] = blk[name][:H].clone()
        res.append(out)
        env.close()
    assert os.path.getmtime(path) == mtime
    assert bool(res[0]["done"].any()), "no episode ended inside the horizon"
    assert float(res[0]["grad"].abs().max()) > 0 and float(res[0]["reward"].abs().max()) > 0
    for k in res[0]:
        a, b = res[0][k], res[1][k]
        same = torch.equal(a, b) if a.dtype == torch.bool else torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert same, f"{kind} {act} {policy}: {k} differs (max abs {float((a.float() - b.float()).abs().max()):.3e})"


@pytest.mark.parametrize("policy", ACTORS, ids=["one_head", "two_heads"])
def test_one_optimiser_step_moves_every_layer(policy):
    """BPTT.learn for one horizon with a Tanh actor: every layer the horizon back-propagates through gets new weights and biases (the
    one-head actor's value trunk is not part of a BPTT horizon: no gradient, Adam leaves it alone); everything stays finite"""
    env = hover(64, max_episode_steps=32)
    algo = make(env, "Tanh", policy, horizon=8, seed=4)
    pol = algo.policy
    p0 = pol.flat.clone()
    algo.learn(8 * 64)
    assert algo._opt_step == 1 and torch.isfinite(pol.flat).all() and torch.isfinite(pol.grad).all() and np.isfinite(algo.logs["train/actor_loss"])
    for ly in pol.layers:
        moved = [not torch.equal(p0[o:o + n], pol.flat[o:o + n]) for o, n in ((ly.w_off, ly.K * ly.No), (ly.b_off, ly.No))]
        critic_side = policy is None and (ly.dst == "value" or ly.dst.startswith("vf:"))
        assert moved == [not critic_side] * 2, (ly.src, ly.dst, moved)
    env.close()


# ---- archives -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ACTORS, ids=["one_head", "two_heads"])
def test_checkpoint_names_the_activation_and_refuses_another(policy, tmp_path):
    """save with a Tanh actor: the archive's spec names both activations; load / set_parameters into a Tanh trainer reproduce
    predict(deterministic=True) bit for bit; a ReLU trainer refuses the archive (ValueError) and keeps its own weights; a ReLU archive
    names relu and is refused by a Tanh trainer"""
    from visfly_amd import checkpoint
    from visfly_amd.bptt import BPTT
    mk = lambda act, seed: make(hover(64, max_episode_steps=32), act, policy, horizon=4, seed=seed)
    algo = mk("Tanh", 2)
    algo.learn(4 * 64 * 2)
    path = str(tmp_path / "tanh_actor")
    algo.save(path)
    spec_of = lambda p: (torch.load(p + ".pth", map_location="cpu")["spec"] if policy else checkpoint.read_archive(p)[2]["policy_spec"])
    spec = spec_of(path)
    assert (spec["activation"], spec["extractor_activation"]) == ("tanh", "relu")
    obs = algo.env.get_observation()
    a0, _ = algo.predict(obs, deterministic=True)
    other = mk("Tanh", 11)
    assert not torch.equal(other.policy.flat, algo.policy.flat)
    other.set_parameters(path)
    assert torch.equal(other.policy.flat, algo.policy.flat) and torch.equal(other.predict(obs, deterministic=True)[0], a0)
    loaded = BPTT.load(path if policy else path + ".zip", hover(64, max_episode_steps=32))     # the archive's own activation
    assert (loaded.policy.act, loaded.policy.ext_act) == (2, 1) and torch.equal(loaded.predict(obs, deterministic=True)[0], a0)
    relu = mk("ReLU", 11)
    before = relu.policy.flat.clone()
    with pytest.raises(ValueError, match="activations"):
        relu.set_parameters(path)
    assert torch.equal(relu.policy.flat, before)
    with pytest.raises(ValueError, match="activations"):
        BPTT.load(path if policy else path + ".zip", hover(64, max_episode_steps=32), policy=policy, policy_kwargs=policy_kwargs("ReLU", policy))
    rpath = str(tmp_path / "relu_actor")
    relu.save(rpath)
    spec = spec_of(rpath)
    assert (spec["activation"], spec["extractor_activation"]) == ("relu", "relu")
    with pytest.raises(ValueError, match="activations"):
        other.set_parameters(rpath)
    relu2 = mk("ReLU", 12).set_parameters(rpath)
    assert torch.equal(relu2.policy.flat, relu.policy.flat)


def test_shac_still_refuses_an_activation():
    from visfly_amd.shac import SHAC
    for pk in (dict(activation_fn="Tanh"), dict(features_extractor_kwargs=dict(activation_fn="elu"))):
        with pytest.raises(NotImplementedError, match="SHAC"):
            SHAC(hover(16), policy_kwargs=pk)


# ---- the reference's own loop with a Tanh actor ----------------------------------------------------------------------------------
# tests/golden/bptt_loop_hover_tanh.npz: tools/gen_bptt_act.py -- oracle/gen_shac.py::gen_bptt_loop with policy_kwargs["activation_fn"] =
# th.nn.Tanh (MTDPolicy hands it to the Actor's trunks; the StateExtractor keeps ReLU), everything else as tests/golden/bptt_loop_hover.npz.
# Bounds: those of test_bptt_gpu.py::test_bptt_learn_iteration_matches_the_reference_loop_with_its_own_actor.
def test_bptt_learn_iteration_matches_the_reference_loop_with_a_tanh_actor():
    from test_shac_gpu import blocks_close
    from visfly_amd.bptt import BPTT
    from visfly_amd.envs import HoverEnv
    fx = load("bptt_loop_hover_tanh")
    N = fx["fs_init"].shape[0]
    env = HoverEnv(num_agent_per_scene=N, seed=int(fx["seed"]), dynamics_kwargs=ast.literal_eval(str(fx["dyn_kw"])), device=DEV,
                   tensor_output=True, requires_grad=True, max_episode_steps=int(fx["max_episode_steps"]),
                   random_kwargs=ast.literal_eval(str(fx["spawn"])), spawn="replay", replay_trig="cr", constants=consts_of(fx))
    env.reset()
    assert_bits_equal(env.full_state.cpu().numpy(), fx["fs_init"], "spawn states of the replayed stream")
    algo = BPTT(env, policy="MultiInputPolicy", policy_kwargs=dict(policy_kwargs("Tanh", "MultiInputPolicy", ([128, 64], [64, 64])),
                                                                   share_features_extractor=False),
                horizon=int(fx["H"]), gamma=float(fx["gamma"]), learning_rate=float(fx["lr"]), seed=int(fx["seed"]))
    a = algo.policy
    assert algo.reference_actor and (a.act, a.ext_act) == (2, 1) and a.n_params == fx["actor_params0"].size == a.n_total
    assert [(ly.K, ly.No) for ly in a.layers] == [(13, 128), (128, 64), (64, 64), (64, 64), (64, 4), (64, 64), (64, 64), (64, 4)]
    a.flat[:a.n_params].copy_(torch.from_numpy(fx["actor_params0"]))
    a.mark_updated()
    algo._eps_override = torch.from_numpy(fx["eps"]).to(DEV)
    loss = algo._grad_reverse_sweep()
    n = lambda t: t.cpu().numpy()
    done = n(env._tape_done[:int(fx["H"])]).astype(np.uint8)
    assert np.array_equal(done, fx["done"]) and fx["done"].sum() > 0
    for got, want, what in ((algo._last_rollout["action"], fx["action"], "actions"), (algo._last_rollout["reward"], fx["reward"], "rewards")):
        err = np.abs(n(got) - want).max()
        print(f"BPTT loop, Tanh actor, {what}: max abs err {err:.2e}")
        assert err <= 1e-6, what
    print(f"actor loss {float(loss):.7f} vs {float(fx['actor_loss']):.7f}")
    assert abs(float(loss) - float(fx["actor_loss"])) <= 2e-6, (float(loss), float(fx["actor_loss"]))
    scale = np.abs(fx["actor_grad"]).max()
    print(f"actor gradient: max abs err {np.abs(n(a.grad) - fx['actor_grad']).max():.3e} of {scale:.3e}")
    rel = blocks_close(n(a.grad), fx["actor_grad"], a, 2e-5, 1e-3, "actor gradient of BPTT.learn, Tanh actor")
    print(f"gradient rel err {rel:.2e}")
    a.grad.copy_(torch.from_numpy(fx["actor_grad"]))      # clip_grad_norm_(0.5) + Adam + env.detach() from the reference's own gradient
    algo._apply(loss)
    assert np.abs(n(a.flat[:a.n_params]) - fx["actor_params1"]).max() <= 2e-7
    assert env._tape_t == 0
    env.close()
