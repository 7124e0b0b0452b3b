"""StateGateExtractor on the GPU: the extractor against the fixture read off the reference's module (tests/golden/gate_extractor.npz), the
policies PPO and BPTT build for it against a float64 torch replica, the persistent launches of the racing kinds with the gate column as
branch 1 against the launch-by-launch loop (bit for bit), one learn step per trainer, which index the column holds, and the archives.
The networks are {state: [64, 32], gate: [32]} with trunks [32]: the classes and plugins __graft_entry__.build() pre-builds
(_jit.PREBUILD["gate_pi"], PREBUILD_SAC["gate_sac"], PREBUILD_ROLLOUT / PREBUILD_BPTT), so no test waits for a compiler.

The gates are placed inside three of RacingEnv's four spawn boxes (0.1 m off their centres; pass radius 0.3 m, boxes of half width 0.2 m):
most agents spawned there pass their gate in the first steps of the horizon, so that the index changes inside it; RacingEnv chooses
gate 0, 1 or 3 at a spawn, depending on the box."""
import os

import numpy as np
import pytest
import torch

from _golden import ENV_DYN, RACING_DYN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXT = {"state": [64, 32], "gate": [32]}
GATES = [[2.0, 2.0, 0.9], [6.0, 2.0, 1.6], [5.0, -4.0, 1.0], [2.0, 0.0, 0.9]]
ACTORS = [None, "MultiInputPolicy"]      # BPTT's one-head MlpPolicy actor / the reference's two-head Actor
IDS = lambda v: {None: "one_head", "MultiInputPolicy": "two_heads"}.get(v, str(v))


def policy_kwargs(two_heads=False, builtin=False):
    """builtin: only the class is named -- the trainers' default network ([128, 64] per branch, trunks [64, 64]), the shape of the
    library's built-in two-branch classes"""
    if builtin:
        return dict(features_extractor_class="StateGateExtractor", activation_fn="relu")
    return dict(features_extractor_class="StateGateExtractor",
                features_extractor_kwargs=dict(net_arch={k: dict(layer=list(v)) for k, v in EXT.items()}),
                net_arch=dict(pi=[32], qf=[32]) if two_heads else dict(pi=[32], vf=[32]), activation_fn="relu")


def racing_env(kind, N, dyn, max_episode_steps=5, requires_grad=True, seed=5):
    import visfly_amd.envs as E
    return {"racing2": E.RacingEnv2, "racing": E.RacingEnv}[kind](
        num_agent_per_scene=N, seed=seed, dynamics_kwargs=dict(dyn), device=DEV, tensor_output=True, requires_grad=requires_grad,
        max_episode_steps=max_episode_steps, gates=GATES)


def bits_equal(a, b):
    return torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32))


def gate_layers(pol):
    return [ly for ly in pol.layers if ly.src == "obs:gate"]


# ---- 1. the extractor against the fixture ----------------------------------------------------------------------------------------
def test_extractor_reproduces_the_reference_features():
    """MlpPolicy with the fixture's parameters on its 64 rows (the int32 gate column fed as .float()) against the features the reference's
    StateGateExtractor computed in fp32.  Bound: 4 x the fixture's own max |fp32 - fp64| (parity)"""
    from visfly_amd import checkpoint
    from visfly_amd.ppo import MlpPolicy, policy_rows
    z = np.load(os.path.join(GOLD, "gate_extractor.npz"))
    pol = MlpPolicy({"state": 16, "gate": 1}, EXT, [32], [32], DEV, seed=1)
    assert pol.chain_jit
    sd = checkpoint.policy_state_dict(pol)
    for k in z.files:
        if k.startswith("param:"):
            for alias in ("", "pi_", "vf_"):
                sd[alias + k[6:]] = torch.from_numpy(z[k])
    checkpoint.load_policy_state_dict(pol, sd, strict=True)
    obs = policy_rows({"state": torch.from_numpy(z["obs_state"]).to(DEV), "gate": torch.from_numpy(z["obs_gate"]).to(DEV)}, ["state", "gate"])
    assert obs["gate"].dtype == torch.float32 and obs["gate"].shape == (64, 1)
    pol.forward(obs, save_activations=True, slot=0)
    got = pol._buffers(64, 0)["feat"].cpu().double().numpy()
    own = np.abs(z["features32"].astype(np.float64) - z["features64"]).max()
    err = np.abs(got - z["features32"].astype(np.float64)).max()
    print(f"features: |MlpPolicy - reference fp32| {err:.3e}, the fixture's own |fp32 - fp64| {own:.3e} (bound {4 * own:.3e})")
    assert own > 0 and err <= 4 * own, (err, own)


# ---- 2. forward and gradients against a float64 replica ---------------------------------------------------------------------------
@pytest.mark.parametrize("trainer", ["ppo", "bptt_one_head", "bptt_two_heads"])
def test_policy_forward_and_gradients_vs_torch(trainer):
    """heads, d obs["state"] and the parameter gradient of the policy each trainer builds for StateGateExtractor against a float64 torch
    replica of the same weights, 33 rows (two 16-row tiles and one row of a third) with every gate index present.  Tolerances: those of
    test_bptt_activations_gpu.py::test_policy_forward_and_gradients_vs_torch; the gate branch's first layer on its own scale; no gradient
    for "gate"."""
    from visfly_amd.bptt import BPTT, PolicyFunction
    from visfly_amd.ppo import PPO
    N = 33
    if trainer == "ppo":
        env = racing_env("racing2", N, ENV_DYN, requires_grad=False)
        algo = PPO(env, n_steps=4, batch_size=4 * N, n_epochs=1, seed=2, policy_kwargs=policy_kwargs())
    else:
        env = racing_env("racing2", N, RACING_DYN)
        two = trainer == "bptt_two_heads"
        algo = BPTT(env, policy="MultiInputPolicy" if two else None, policy_kwargs=policy_kwargs(two), horizon=4, seed=2)
    pol = algo.policy
    assert algo.obs_keys == ["state", "gate"] and pol.obs_dims == {"state": 16, "gate": 1} and pol.chain_jit
    ref = pol.to_torch().double()
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (env.get_observation()["state"].detach() + 0.3 * torch.randn((N, 16), device=DEV, generator=g)).contiguous()
    gate = (torch.arange(N, device=DEV) * 3 % 4).to(torch.float32).reshape(N, 1).contiguous()
    w0, w1 = torch.randn((N, 4), device=DEV, generator=g), torch.randn((N, pol.head_dims[1]), device=DEV, generator=g)
    pol.grad.zero_()
    m, v = pol.forward({"state": x, "gate": gate}, slot=0)
    heads = [m.clone(), v.clone()]
    d_in = pol.backward(w0.contiguous(), w1.contiguous(), None, accumulate=True, need_input_grad=True, slot=0)
    assert sorted(d_in) == ["state"], sorted(d_in)
    d_x = d_in["state"]
    xr = x.cpu().double().requires_grad_(True)
    out = ref({"state": xr, "gate": gate.cpu().double()})
    ((out[0] * w0.cpu().double()).sum() + (out[1] * w1.cpu().double()).sum()).backward()
    close = lambda a, b: torch.allclose(a.cpu().double(), b, rtol=1e-3, atol=1e-5 * float(b.abs().max()) + 1e-6)
    for got, want, what in zip(heads, out, ("first head", "second head")):
        print(f"{trainer} {what}: max abs err {float((got.cpu().double() - want.detach()).abs().max()):.2e} of {float(want.detach().abs().max()):.2e}")
        assert close(got, want.detach()), what
    print(f"{trainer} d obs['state']: max abs err {float((d_x.cpu().double() - xr.grad).abs().max()):.2e} of {float(xr.grad.abs().max()):.2e}")
    assert close(d_x, xr.grad)
    gref, got = ref.flat_grad().double(), pol.grad.cpu().double()
    err, scale = float((got - gref).abs().max()), float(gref.abs().max())
    print(f"{trainer} parameter gradient: max abs err {err:.2e} of {scale:.2e}")
    assert scale > 0 and err <= 2e-4 * scale
    (ly,) = gate_layers(pol)
    assert (ly.K, ly.No, ly.dst, ly.dc) == (1, 32, "feat", 32)
    for off, n, what in ((ly.w_off, 32, "weight"), (ly.b_off, 32, "bias")):
        e, s = float((got[off:off + n] - gref[off:off + n]).abs().max()), float(gref[off:off + n].abs().max())
        print(f"{trainer} gate branch, first layer {what}: max abs err {e:.2e} of {s:.2e}")
        assert s > 0 and e <= 2e-4 * s, what
    if trainer == "bptt_one_head":      # ... and under torch.autograd (what use_autograd=True schedules): None for the index column
        xg, gg = x.clone().requires_grad_(True), gate.clone().requires_grad_(True)
        mean = PolicyFunction.apply(pol, ["state", "gate"], torch.zeros(1, device=DEV, requires_grad=True), xg, gg)
        (mean * w0).sum().backward()
        assert gg.grad is None and xg.grad is not None
    env.close()


def test_reverse_sweep_equals_autograd_path():
    """the launch-by-launch reverse sweep against the torch.autograd-scheduled path over the same kernels (the gate column enters
    PolicyFunction without a graph, obs["state"] keeps its own), as test_bptt_activations_gpu.py::test_reverse_sweep_equals_autograd_path
    and at its tolerance: RacingEnv2, 37 agents, H = 6, episodes of 4 steps"""
    from visfly_amd.bptt import BPTT
    grads, losses = [], []
    for use_autograd in (True, False):
        env = racing_env("racing2", 37, RACING_DYN, max_episode_steps=4)
        algo = BPTT(env, policy_kwargs=policy_kwargs(), horizon=6, learning_rate=1e-3, seed=1)
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
    print(f"autograd path against reverse sweep: max abs diff {(g0 - g1).abs().max().item():.2e} of {scale:.2e}")
    assert scale > 0 and (g0 - g1).abs().max().item() <= 2e-5 * scale, ((g0 - g1).abs().max().item(), scale)


# ---- 3. the persistent launches --------------------------------------------------------------------------------------------------
def _bptt_plugin(policy, cfg):
    from visfly_amd import _jit
    name = "gate_sac" if policy else "gate_pi"
    assert (name, cfg) in _jit.PREBUILD_BPTT
    sh = _jit.prebuild_shape(name)
    return sh, (sh, ("bptt",) + cfg), _jit.path_of(sh, ("bptt",) + cfg)


def _gate_conditions(gate_slots, what):
    """the comparison is not vacuous: the index changes inside the horizon for some agent, and slot 0 holds several indices"""
    g = gate_slots[..., 0]
    changed = int((g != g[0:1]).any(dim=0).sum())
    first = sorted(set(g[0].tolist()))
    print(f"{what}: gate column of {changed} of {g.shape[1]} agents changes inside the horizon; slot 0 holds the indices {first}")
    assert changed >= 1, "no agent's gate column differs between two slots"
    assert len(first) >= 2, "slot 0 holds one gate index only"
    assert set(g.reshape(-1).tolist()) <= {0.0, 1.0, 2.0, 3.0}


@pytest.mark.parametrize("kind,policy,N,net", [("racing2", p, n, "generated") for p in ACTORS for n in (5, 1000)] +
                         [("racing", "MultiInputPolicy", 1000, "generated")] +
                         [("racing2", p, 1000, "builtin") for p in ACTORS] + [("racing", "MultiInputPolicy", 1000, "builtin")], ids=IDS)
def test_bptt_persistent_launches_equal_the_loop(kind, policy, N, net):
    """vf_bptt_rollout / vf_bptt_reverse with the gate column as branch 1 (RacingEnv2: kernel-side kind 3; RacingEnv: 2; thrust) against
    the launch-by-launch sweep: actions, rewards, done flags, the tape, every slot's obs:state / obs:gate / activations / layer gradients,
    the loss rows and the flat gradient are bit-identical.  5 agents: less than a wave; 1000: 63 tiles of 16 rows, the last one ragged.
    H = 8, episodes of 5 steps.  `builtin`: the trainers' default network, i.e. what naming only the class gives -- the shape of the
    library's built-in two-branch classes, whose racing instances then serve both launches (no plugin)."""
    from visfly_amd import _jit, _lib
    from visfly_amd.bptt import BPTT
    H = 8
    builtin = net == "builtin"
    cfg = (3 if kind == "racing2" else 2, 0, 0, True)
    if not builtin:
        sh, key, path = _bptt_plugin(policy, cfg)
        assert os.path.exists(path), f"{path}: not pre-built (__graft_entry__.build())"
    res = []
    for fused in (True, False):
        env = racing_env(kind, N, RACING_DYN)
        algo = BPTT(env, policy=policy, policy_kwargs=policy_kwargs(policy is not None, builtin), horizon=H, learning_rate=1e-3, seed=9)
        assert algo.obs_keys == ["state", "gate"]
        if builtin:
            assert algo.policy.spec["extractor"] == {"state": [128, 64], "gate": [128, 64]} and _jit.is_builtin(algo.policy.chain_shape)
            assert not algo.policy.chain_jit
        else:
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
        torch.cuda.synchronize()
        assert used == ([True] if fused else []) and rev_used == used, (used, rev_used)
        if fused and not builtin:
            assert _lib.lib().vf_chain_plugin_launches() >= n0 + 2 and _jit._loaded.get(key) == path
        if builtin:
            assert _lib.lib().vf_chain_plugin_launches() == n0      # the library's own instances
        live = lambda x: x.transpose(-3, -4).reshape(*x.shape[:-4], x.shape[-3], -1, 4)[..., :N, :].clone()
        blk = algo.policy._slot_blocks[N][1]
        last = env.get_observation()
        out = {"loss": loss.clone(), "loss_rows": algo._horizon["loss_vec"].clone(), "grad": algo.policy.grad.clone(),
               "action": algo._horizon["actions"].clone(), "reward": rr.clone() if fused else torch.stack(rewards),
               "done": env._tape_done[:H].clone(), "tape": live(env._tape[:H]), "slab": live(env._slab), "adj": live(env._adj),
               "last:state": last["state"].clone(), "last:gate": last["gate"].clone()}
        # (the one-head actor's horizon never runs the value trunk, and its mean stays inside the launch that applies the action head)
        pi_side = [k for k in blk if k.split(":")[0] in ("obs", "x", "feat", "pi") or k.startswith(("g:x", "g:feat", "g:pi"))]
        vf_side = [k for k in blk if k.split(":")[0] in ("vf", "mean", "value") or k.startswith("g:vf")]
        assert {"obs:state", "obs:gate", "feat", "pi:0", "g:feat", "g:pi:0", "x:state:0", "g:x:state:0"} <= set(pi_side)
        assert {"vf:0", "mean", "value", "g:vf:0"} <= set(vf_side) and (not builtin or "g:x:gate:0" in pi_side)
        for name in pi_side + (vf_side if policy else []):
            out[name] = blk[name][:H].clone()
        res.append(out)
        env.close()
    assert bool(res[0]["done"].any()), "no episode ended inside the horizon"
    assert float(res[0]["grad"].abs().max()) > 0 and float(res[0]["reward"].abs().max()) > 0
    _gate_conditions(res[0]["obs:gate"], f"{kind} N={N}")
    for k in res[0]:
        a, b = res[0][k], res[1][k]
        assert bits_equal(a, b), f"{kind} {policy} N={N}: {k} differs (max abs {float((a.float() - b.float()).abs().max()):.3e})"


@pytest.mark.parametrize("N,net", [(5, "generated"), (1000, "generated"), (1000, "builtin")])
def test_ppo_persistent_rollout_equals_the_loop(N, net):
    """collect_rollouts on RacingEnv2 as ONE launch (vf_ppo_rollout, the roll-out plugin of the gate class) against the launch-by-launch
    loop: the buffer rows including obs["gate"], values, log-probs, the bootstrapped rewards, advantages / returns, the TimeLimit list
    with the terminal gate of every truncated row, and the values of the final observation, bit for bit.  T = 8, episodes of 5 steps."""
    from visfly_amd import _jit, _lib
    from visfly_amd.ppo import PPO
    T = 8
    sh = _jit.prebuild_shape("gate_pi")
    assert ("gate_pi", (3, 1, 0, True)) in _jit.PREBUILD_ROLLOUT and os.path.exists(_jit.path_of(sh, (3, 1, 0, True)))
    res = []
    for fused in (True, False):
        env = racing_env("racing2", N, ENV_DYN, requires_grad=False)
        ppo = PPO(env, n_steps=T, batch_size=max(N * T // 4, 8), n_epochs=1, seed=2, policy_kwargs=policy_kwargs(builtin=net == "builtin"))
        assert ppo.obs_keys == ["state", "gate"]
        if net == "builtin":      # naming only the class: the default network, served by the library's own racing instances
            assert ppo.policy.spec["extractor"] == {"state": [128, 64], "gate": [128, 64]} and _jit.is_builtin(ppo.policy.chain_shape)
        else:
            assert ppo.policy.chain_shape == sh and ppo.policy.chain_jit
        assert ppo.buf.obs["gate"].shape == (T, N, 1)
        ppo.fused_rollout = fused
        inner, results = env.collect_policy, []

        def collect(*a, **k):
            r = inner(*a, **k)
            results.append(r is not False)
            return r
        env.collect_policy = collect
        n0 = _lib.lib().vf_chain_plugin_launches()
        out = {}
        for rnd in range(2):
            ppo.collect_rollouts()
            torch.cuda.synchronize()
            assert ppo.fused_rollout is fused
            for k in ("rewards", "values", "advantages", "returns", "episode_starts", "log_probs", "actions"):
                out[f"{rnd}:{k}"] = getattr(ppo.buf, k).clone()
            for k in ppo.obs_keys:
                out[f"{rnd}:obs:{k}"] = ppo.buf.obs[k].clone()
                out[f"{rnd}:last:{k}"] = ppo._last_obs[k].clone()
            out[f"{rnd}:last_values"] = ppo.predict_values(ppo._last_obs)
            cnt = int(ppo._boot["cursor"].item())
            order = torch.argsort(ppo._boot["idx"][:cnt])
            out[f"{rnd}:boot_idx"] = ppo._boot["idx"][:cnt][order].clone()
            out[f"{rnd}:boot_rows0"] = ppo._boot["rows0"][:cnt][order].clone()
            out[f"{rnd}:boot_rows1"] = ppo._boot["rows1"][:cnt][order].clone()
            assert cnt >= N, cnt                     # T = 8 steps, episodes of 5: every agent is truncated at least once
            out[f"{rnd}:stat"] = ppo._boot["stat"].clone()
            out[f"{rnd}:starts"] = ppo._last_starts.clone()
            if rnd == 0:
                ppo.train()
        out["params"] = ppo.policy.flat.clone()
        assert results == ([True, True] if fused else []), results
        if fused and net != "builtin":
            assert _lib.lib().vf_chain_plugin_launches() > n0
        res.append(out)
        env.close()
    assert bool((res[0]["0:episode_starts"][1:] > 0).any()), "no episode ended inside the roll-out"
    _gate_conditions(res[0]["0:obs:gate"], f"PPO N={N}")
    for k in res[0]:
        assert bits_equal(res[0][k], res[1][k]), f"N={N}: {k} differs"


# ---- 4. one learn step per trainer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trainer", ["ppo", "bptt", "shac"])
def test_one_learn_step_moves_the_gate_branch(trainer):
    """one iteration of learn() at 64 agents, fused_rollout at its default: the racing persistent launch runs it, every layer of the gate
    branch gets new weights and biases, everything stays finite"""
    from visfly_amd import _lib
    from visfly_amd.bptt import BPTT
    from visfly_amd.ppo import PPO
    from visfly_amd.shac import SHAC
    N, H = 64, 8
    if trainer == "ppo":
        env = racing_env("racing2", N, ENV_DYN, max_episode_steps=32, requires_grad=False)
        algo = PPO(env, n_steps=H, batch_size=N * H // 2, n_epochs=2, seed=4, policy_kwargs=policy_kwargs())
        name, inner = "collect_policy", env.collect_policy
    else:
        env = racing_env("racing2", N, RACING_DYN, max_episode_steps=32)
        if trainer == "bptt":
            algo = BPTT(env, policy="MultiInputPolicy", policy_kwargs=policy_kwargs(True), horizon=H, learning_rate=1e-3, seed=4)
        else:
            algo = SHAC(env, policy_kwargs=policy_kwargs(True), horizon=H, gradient_steps=2, learning_rate=1e-3, seed=4)
        name, inner = "rollout_policy", env.rollout_policy
    took = []

    def wrapped(*a, **k):
        r = inner(*a, **k)
        took.append(r is not False)
        return r
    setattr(env, name, wrapped)
    nets = [algo.policy] + ([algo.critic] if trainer == "shac" else [])
    before = [p.flat.clone() for p in nets]
    n0 = _lib.lib().vf_chain_plugin_launches()
    algo.learn(H * N)
    torch.cuda.synchronize()
    assert took == [True], took
    assert _lib.lib().vf_chain_plugin_launches() > n0
    assert algo.fused_rollout is True
    for p, p0 in zip(nets, before):
        assert torch.isfinite(p.flat).all() and torch.isfinite(p.grad).all()
        layers = gate_layers(p)
        assert len(layers) == 1
        for ly in layers:
            moved = [not torch.equal(p0[o:o + n], p.flat[o:o + n]) for o, n in ((ly.w_off, ly.K * ly.No), (ly.b_off, ly.No))]
            assert moved == [True, True], (trainer, ly.src, ly.dst, moved)
    assert all(np.isfinite(v) for v in algo.logs.values() if isinstance(v, float))
    a, _ = algo.predict(env.get_observation(), deterministic=True)
    assert a.shape == (N, 4) and torch.isfinite(a).all()
    env.close()


# ---- 5. the column is the right index --------------------------------------------------------------------------------------------
# RacingEnv2's first three "state" columns are (gates[index] - p) / 10 (RacingEnv.py:254-257).  Recomputed in fp32 from the same position
# and the same index they agree to a few ulp of a value below 1 (6e-8 each): 1e-6.  With any OTHER index they move by at least the closest
# pair of GATES / 10 = 0.2 -- the check cannot pass with a wrong column.
INDEX_TOL = 1e-6


def test_bptt_slots_hold_the_index_their_state_rows_were_formed_with():
    from visfly_amd.bptt import BPTT
    N, H = 1000, 8
    env = racing_env("racing2", N, RACING_DYN)
    algo = BPTT(env, policy="MultiInputPolicy", policy_kwargs=policy_kwargs(True), horizon=H, learning_rate=1e-3, seed=9)
    took = []
    inner = env.rollout_policy

    def wrapped(*a, **k):
        took.append(inner(*a, **k))
        return took[-1]
    env.rollout_policy = wrapped
    algo._grad_reverse_sweep()
    torch.cuda.synchronize()
    assert took == [True]
    blk = algo.policy._slot_blocks[N][1]
    live = lambda x: x.transpose(-3, -4).reshape(*x.shape[:-4], x.shape[-3], -1, 4)[..., :N, :]
    tape = live(env._tape[:H])                                   # [H][granule][N][4]: row t = the state before step t
    worst, worst_wrong = 0.0, np.inf
    for t in range(H):
        raw = torch.cat([tape[t, 0, :, 1:4], tape[t, 1, :, 0:4], tape[t, 2, :, 1:4], tape[t, 3, :, 1:4]], dim=1).contiguous()
        gate = blk["obs:gate"][t, :, 0]
        assert torch.equal(gate, gate.round()) and 0 <= float(gate.min()) and float(gate.max()) <= 3
        want = env._race_state(raw, gate.to(torch.int32).contiguous())
        got = blk["obs:state"][t]
        worst = max(worst, float((got[:, :3] - want[:, :3]).abs().max()))
        wrong = env._race_state(raw, ((gate.to(torch.int32) + 1) % 4).contiguous())
        worst_wrong = min(worst_wrong, float((got[:, :3] - wrong[:, :3]).abs().max(dim=1).values.min()))
    print(f"obs:state[:, :3] against _race_state(tape position, obs:gate): max abs diff {worst:.3e}; with the next index instead: >= {worst_wrong:.3e}")
    assert worst <= INDEX_TOL and worst_wrong >= 0.19
    _gate_conditions(blk["obs:gate"][:H], "BPTT N=1000")
    env.close()


def test_ppo_bootstrap_rows_carry_the_terminal_gate():
    """the TimeLimit list of a persistent roll-out: columns 3:6 minus columns 0:3 of a terminal "state" row are (gates[k + 1] - gates[k]) / 10
    whatever the position -- k must be the row's gate entry (terminal_gate: the index of the step's start)"""
    from visfly_amd.ppo import PPO
    N, T = 1000, 8
    env = racing_env("racing2", N, ENV_DYN, requires_grad=False)
    ppo = PPO(env, n_steps=T, batch_size=N * T // 4, n_epochs=1, seed=2, policy_kwargs=policy_kwargs())
    ppo.collect_rollouts()
    torch.cuda.synchronize()
    assert ppo.fused_rollout is True
    cnt = int(ppo._boot["cursor"].item())
    assert cnt >= N
    rows0, k = ppo._boot["rows0"][:cnt], ppo._boot["rows1"][:cnt, 0]
    assert torch.equal(k, k.round()) and len(set(k.tolist())) >= 2
    tg = torch.tensor(GATES, device=DEV)
    want = (tg[(k.long() + 1) % 4] - tg[k.long()]) / 10.0
    err = float((rows0[:, 3:6] - rows0[:, 0:3] - want).abs().max())
    wrong = (tg[(k.long() + 2) % 4] - tg[(k.long() + 1) % 4]) / 10.0
    print(f"terminal rows: gate-pair columns against the rows' gate entry: max abs diff {err:.3e}")
    assert err <= 3 * INDEX_TOL and float((rows0[:, 3:6] - rows0[:, 0:3] - wrong).abs().max(dim=1).values.min()) >= 0.19
    # ... and the rows of the buffer itself: slot t's gate entry pairs with slot t's state row
    s, g = ppo.buf.obs["state"].reshape(-1, 16), ppo.buf.obs["gate"].reshape(-1).long()
    err = float((s[:, 3:6] - s[:, 0:3] - (tg[(g + 1) % 4] - tg[g]) / 10.0).abs().max())
    print(f"buffer rows: the same: max abs diff {err:.3e}")
    assert err <= 3 * INDEX_TOL
    env.close()


# ---- 6. archives -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trainer", ["ppo", "bptt_one_head", "bptt_two_heads", "shac"])
def test_archives_round_trip_and_refuse_a_policy_without_the_branch(trainer, tmp_path):
    from visfly_amd import checkpoint
    from visfly_amd.bptt import BPTT
    from visfly_amd.ppo import PPO
    from visfly_amd.shac import SHAC
    N = 64
    two = trainer in ("bptt_two_heads", "shac")
    # the trainer without the branch: networks build() pre-builds as well (_jit.PREBUILD_SAC["sac_hover"] + PREBUILD_CRITIC["critic_hover"]
    # / PREBUILD["one_layer_extractor"]; RacingEnv2's 16 columns pad to the same 16 as their 13)
    if two:
        plain_pk = dict(features_extractor_class="StateExtractor", features_extractor_kwargs=dict(net_arch=dict(state=dict(layer=[64, 64, 32]))),
                        net_arch=dict(pi=[32], qf=[32]), activation_fn="relu")
    else:
        plain_pk = dict(features_extractor_class="StateExtractor", features_extractor_kwargs=dict(net_arch=dict(state=dict(layer=[64]))),
                        net_arch=dict(pi=[64], vf=[64, 64, 32]), activation_fn="relu")

    def mk(seed, pk=None, env=None):
        pk = pk or policy_kwargs(two)
        if trainer == "ppo":
            env = env or racing_env("racing2", N, ENV_DYN, max_episode_steps=32, requires_grad=False)
            return PPO(env, n_steps=4, batch_size=2 * N, n_epochs=1, seed=seed, policy_kwargs=pk)
        env = env or racing_env("racing2", N, RACING_DYN, max_episode_steps=32)
        if trainer == "shac":
            return SHAC(env, policy_kwargs=pk, horizon=4, gradient_steps=1, learning_rate=1e-3, seed=seed)
        return BPTT(env, policy="MultiInputPolicy" if two else None, policy_kwargs=pk, horizon=4, learning_rate=1e-3, seed=seed)
    algo = mk(2)
    algo.learn(4 * N)
    path = str(tmp_path / "gate_policy")
    algo.save(path)
    spec = torch.load(path + ".pth", map_location="cpu")["spec"] if two else checkpoint.read_archive(path)[2]["policy_spec"]
    assert spec["extractor"] == EXT and list(spec["extractor"]) == ["state", "gate"]
    if not two:
        sd = checkpoint.read_archive(path)[0]
        for p in ("features_extractor", "pi_features_extractor", "vf_features_extractor"):
            assert tuple(sd[p + ".gate_extractor.0.weight"].shape) == (32, 1) and tuple(sd[p + ".gate_extractor.0.bias"].shape) == (32,)
    obs = algo.env.get_observation()
    a0, _ = algo.predict(obs, deterministic=True)
    other = mk(11)
    assert not torch.equal(other.policy.flat, algo.policy.flat)
    other.set_parameters(path)
    assert torch.equal(other.policy.flat, algo.policy.flat) and torch.equal(other.predict(obs, deterministic=True)[0], a0)
    cls = type(algo)
    loaded = cls.load(path if two else path + ".zip", racing_env("racing2", N, ENV_DYN if trainer == "ppo" else RACING_DYN, max_episode_steps=32,
                                                                requires_grad=trainer != "ppo"))
    assert loaded.obs_keys == ["state", "gate"] and torch.equal(loaded.predict(obs, deterministic=True)[0], a0)
    plain = mk(11, plain_pk)
    assert plain.obs_keys == ["state"]
    before = plain.policy.flat.clone()
    from visfly_amd import _jit
    assert plain.policy.chain_shape in [_jit.prebuild_shape(n) for n in ("sac_hover", "one_layer_extractor")]
    # SB3-layout archives (PPO, the one-head actor): the shape ValueError; the two-head actors' flat archives: their size assertion
    with (pytest.raises(AssertionError, match="different network") if two else pytest.raises(ValueError, match="shape")):
        plain.set_parameters(path)
    assert torch.equal(plain.policy.flat, before), "a refused archive must leave the policy as it was"
    ppath = str(tmp_path / "plain_policy")
    plain.save(ppath)
    mine = other.policy.flat.clone()
    with (pytest.raises(AssertionError, match="different network") if two else pytest.raises(ValueError, match="shape")):
        other.set_parameters(ppath)
    assert torch.equal(other.policy.flat, mine)
    for t in (algo, other, loaded, plain):
        t.env.close()
