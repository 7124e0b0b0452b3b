"""Deterministic evaluation episodes on the GPU (visfly_amd/evaluate.py, csrc/vf_eval_rollout.hip): the latch kernel against numpy, the
launch-by-launch loop against the reference's rule restated in plain Python over the host info dicts (utils/algorithms/BPTT.py:138-156,
utils/evaluate.py:79-129), the persistent launch against the loop bit for bit for built-in and generated classes, the needs-reset rule,
the fall-backs, and the trainers' ``learn(eval_env=...)``.

All envs run max_episode_steps = 24; N = 48 is three 16-row waves (one and a half 32-row waves), N = 33 a wave with one live row and
replicas.  Every persistent-vs-loop case first asserts that its episodes END AT DIFFERENT STEPS -- some before the time limit, some at it --
so that the first-done latch and the wave exit are exercised: HoverEnv spawns in a box that reaches the floor (agents below the 0.1 m body
radius collide in their first step) under a policy whose thrust head is biased low (the others fall, the high ones do not arrive within
0.48 s); NavigationEnv spawns around the target (agents within the 0.5 m success radius succeed in their first step); on RacingEnv2, whose
spawn boxes are the reference's fixed ones at 0.8 .. 1.2 m and 1.3 .. 1.7 m, the thrust head is biased to its minimum and the control
interval is 0.025 s: 24 steps are 0.6 s, a free fall of 1.76 m less what the action delay and the motor lag take -- the low boxes' agents
(0.7 .. 1.1 m above the body radius) reach the floor, the highest ones (1.6 m) do not."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from _golden import ENV_DYN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 24
box = lambda mean, half: {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": mean, "half": half}}]}}
HOVER_FLOOR = box([1., 0., 0.6], [1., 1., 0.6])              # z in [0, 1.2]: the floor is z = 0, the body radius 0.1
NAV_NEAR = box([9., 0., 1.], [1.2, 1.2, 0.6])                # around NavigationEnv's default target [9, 0, 1], success radius 0.5
GATES = [[2.0, 2.0, 0.9], [6.0, 2.0, 1.6], [5.0, -4.0, 1.0], [2.0, 0.0, 0.9]]
RACING_DYN = dict(ENV_DYN, dt=0.003125, ctrl_dt=0.025)
THRUST_RK4 = dict(action_type="thrust", integrator="rk4", dt=0.0025, ctrl_dt=0.02, ctrl_delay=False)
GATE_PK = dict(features_extractor_class="StateGateExtractor",
               features_extractor_kwargs=dict(net_arch={"state": dict(layer=[64, 32]), "gate": dict(layer=[32])}),
               net_arch=dict(pi=[32], vf=[32]), activation_fn="relu")


def make_env(kind, N, seed=5, dyn=ENV_DYN, **kw):
    import visfly_amd.envs as E
    if kind == "hover":
        return E.HoverEnv(num_agent_per_scene=N, seed=seed, dynamics_kwargs=dict(dyn), device=DEV, tensor_output=True, max_episode_steps=T,
                          random_kwargs=kw.pop("random_kwargs", HOVER_FLOOR), **kw)
    if kind == "nav":
        return E.NavigationEnv(num_agent_per_scene=N, seed=seed, dynamics_kwargs=dict(dyn), device=DEV, tensor_output=True,
                               max_episode_steps=T, random_kwargs=NAV_NEAR, **kw)
    return E.RacingEnv2(num_agent_per_scene=N, seed=seed, dynamics_kwargs=dict(dyn), device=DEV, tensor_output=True, max_episode_steps=T,
                        gates=GATES, **kw)


def bias_thrust(pol, value):
    """the first component of the mean head (collective thrust of both action types) gets bias `value`: tanh(-3) = -0.995 is minimum thrust"""
    head = [ly for ly in pol.layers if ly.dst == "mean"][0]
    pol.bias(head)[0] = value
    pol.mark_updated()


def make_model(case, env):
    from visfly_amd.bptt import BPTT
    from visfly_amd.ppo import PPO
    from visfly_amd.shac import SHAC
    N = env.num_agent
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if case == "ppo_relu":
            m = PPO(env, n_steps=4, batch_size=4 * N, n_epochs=1, seed=2, policy_kwargs=dict(activation_fn="relu"))
        elif case == "ppo_tanh":                  # the reference policy's default activations: a generated class
            m = PPO(env, n_steps=4, batch_size=4 * N, n_epochs=1, seed=2)
        elif case == "ppo_gate":
            m = PPO(env, n_steps=4, batch_size=4 * N, n_epochs=1, seed=2, policy_kwargs=dict(GATE_PK))
        elif case == "ppo_wide":
            m = PPO(env, n_steps=4, batch_size=4 * N, n_epochs=1, seed=2, policy_kwargs=dict(activation_fn="relu", net_arch=dict(pi=[256, 256], vf=[256, 256])))
        elif case == "shac":
            m = SHAC(env, horizon=4, gradient_steps=1, learning_rate=1e-3, seed=7)
        elif case == "bptt_sac":
            m = BPTT(env, policy="MultiInputPolicy", horizon=4, learning_rate=1e-3, seed=7)
        elif case == "bptt_sac_tanh":             # BPTT's Tanh SAC-style Actor on the sac_hover sizes: a generated (4, 4) class
            m = BPTT(env, policy="MultiInputPolicy", horizon=4, learning_rate=1e-3, seed=7,
                     policy_kwargs=dict(features_extractor_class="StateExtractor",
                                        features_extractor_kwargs={"net_arch": {"state": {"layer": [64, 64, 32]}}},
                                        net_arch=dict(pi=[32], qf=[32]), activation_fn="Tanh"))
        else:
            raise KeyError(case)
    return m


def bits_equal(a, b):
    return a.shape == b.shape and (torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ---- G1 ------------------------------------------------------------------------------------------------------------------------------
def test_g1_latch_kernel():
    from visfly_amd import _lib
    L, N, S, OW = _lib.lib(), 70, 6, 13
    rng = np.random.default_rng(3)
    first = rng.integers(0, S + 3, N)               # >= S: never finishes
    first[:4] = (0, 0, S - 1, S + 1)
    done = np.arange(S)[:, None] >= first[None, :]                       # sticky
    ret = rng.standard_normal((S, N)).astype(np.float32)                # the episode outputs keep changing after the first done
    length = rng.integers(1, 100, (S, N)).astype(np.int32)
    flags = rng.integers(0, 16, (S, N)).astype(np.uint8)
    term = rng.standard_normal((S, N, OW)).astype(np.float32)
    init = dict(r=np.full(N, -7.5, np.float32), l=np.full(N, -3, np.int32), f=np.full(N, 99, np.uint8), t=np.full((N, OW), 0.25, np.float32))
    for with_terminal in (True, False):
        out = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in init.items()}
        latched = torch.zeros(N, dtype=torch.uint8, device=DEV)
        for s in range(S):
            d = [torch.from_numpy(x[s].copy()).to(DEV) for x in (done.astype(np.uint8), ret, length, flags, term)]
            _lib.check(L.vf_eval_latch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr() if with_terminal else None,
                                       latched.data_ptr(), out["r"].data_ptr(), out["l"].data_ptr(), out["f"].data_ptr(),
                                       out["t"].data_ptr() if with_terminal else None, N, OW, _lib.current_stream(torch.device(DEV))))
        torch.cuda.synchronize()
        fin, idx, f0 = first < S, np.arange(N), np.minimum(first, S - 1)
        assert fin.any() and (~fin).any() and (first == 0).sum() >= 2
        assert np.array_equal(latched.cpu().numpy(), fin.astype(np.uint8))
        assert np.array_equal(out["r"].cpu().numpy().view(np.uint32), np.where(fin, ret[f0, idx], init["r"]).view(np.uint32))
        assert np.array_equal(out["l"].cpu().numpy(), np.where(fin, length[f0, idx], init["l"]))
        assert np.array_equal(out["f"].cpu().numpy(), np.where(fin, flags[f0, idx], init["f"]))
        want_t = np.where(fin[:, None], term[f0, idx], init["t"]) if with_terminal else init["t"]
        assert np.array_equal(out["t"].cpu().numpy().view(np.uint32), want_t.view(np.uint32))
    assert L.vf_eval_latch(None, None, None, None, None, None, None, None, None, None, N, OW, None) != 0 and b"vf_eval_latch" in L.vf_last_error()
    assert L.vf_eval_action(None, None, N, None) != 0 and L.vf_eval_rollout(None, None, None, None, None, None) != 0


# ---- G2: the reference's rule in plain Python ---------------------------------------------------------------------------------------------
def reference_rule(model, env):
    """BPTT.py:138-156 / evaluate.py:79-129: reset; a = deterministic action; env.step(a, is_test=True); at an agent's first done step take
    info[i]["episode"]["r" | "l"] and info[i]["is_success"] from the HOST info dicts; until done.all() -> (r, l, success, first step)"""
    from visfly_amd import _lib
    from visfly_amd.ppo import policy_rows
    N = env.num_agent
    env.tensor_output = True
    obs = env.reset()
    r, l, s, first = np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, bool), np.full(N, -1)
    ids = list(range(N))
    for t in range(10 * T):
        mean, _ = model.policy.forward(policy_rows(obs, model.obs_keys), save_activations=False)
        a, lp = torch.empty((N, 4), device=DEV), torch.empty(N, device=DEV)
        # tanh(mean) with the device's tanhf: the head sampler's deterministic branch (what PPO.predict(deterministic=True) runs)
        _lib.check(_lib.lib().vf_head_sample(mean.data_ptr(), model.policy.log_std.data_ptr(), a.data_ptr(), lp.data_ptr(), N, 0, 0, 1,
                                             _lib.current_stream(torch.device(DEV))))
        obs, reward, done, info = env.step(a, is_test=True)
        dn = done.cpu().numpy()
        for index in reversed(list(ids)):
            if dn[index]:
                ids.remove(index)
                r[index], l[index], s[index], first[index] = info[index]["episode"]["r"], info[index]["episode"]["l"], info[index]["is_success"], t
        if dn.all():
            break
    assert not ids and t < T
    return r, l, s, first


def assert_is_reference(res, ref):
    r, l, s, first = ref
    assert np.array_equal(res.ep_return.cpu().numpy().view(np.uint32), r.view(np.uint32))
    assert np.array_equal(res.ep_length.cpu().numpy(), l) and np.array_equal(l, first + 1)
    assert np.array_equal(res.is_success.cpu().numpy(), s)
    assert res.mean_r == float(r.astype(np.float64).mean()) and res.mean_l == float(l.mean()) and res.success_rate == float(s.mean())


@pytest.mark.parametrize("kind", ["hover", "nav"])
def test_g2_loop_is_the_reference_rule(kind):
    from visfly_amd.evaluate import evaluate_policy
    model = make_model("ppo_relu", make_env(kind, 33))
    if kind == "hover":
        bias_thrust(model.policy, -1.0)
    res = evaluate_policy(model, make_env(kind, 33, seed=11), persistent=False, terminal_rows=True)
    ref = reference_rule(model, make_env(kind, 33, seed=11))
    print(f"{kind}: lengths {sorted(set(ref[1].tolist()))}, successes {int(ref[2].sum())}")
    assert res.path == "loop" and len(set(ref[1].tolist())) >= 2
    assert_is_reference(res, ref)
    # record=True: the same episodes, and the (T, N, .) stacks of the run
    rec = evaluate_policy(model, make_env(kind, 33, seed=11), record=True)
    assert rec.path == "loop" and bits_equal(rec.ep_return, res.ep_return) and torch.equal(rec.ep_length, res.ep_length)
    assert rec.state_all.shape == (T, 33, 13) and rec.action_all.shape == (T, 33, 4) and rec.reward_all.shape == (T, 33) and rec.done_all.shape == (T, 33)
    fd = rec.done_all.int().argmax(dim=0)            # sticky: the first done step
    assert torch.equal(fd.to(torch.int32) + 1, res.ep_length) and bool(rec.done_all[-1].all())
    # the terminal rows are the observation of the first done step (is_test: no re-spawn)
    assert bits_equal(res.terminal_state, rec.state_all[fd, torch.arange(33, device=DEV)])
    assert res.state_all is None


# ---- G3: the persistent launch equals the loop ------------------------------------------------------------------------------------------
G3 = {   # case: (env kind, N, model, thrust bias or None, dynamics, generated class?)
    "ppo_relu_hover_48": ("hover", 48, "ppo_relu", -1.0, ENV_DYN, False),
    "ppo_relu_hover_33": ("hover", 33, "ppo_relu", -1.0, ENV_DYN, False),
    "ppo_relu_nav_48": ("nav", 48, "ppo_relu", None, ENV_DYN, False),
    "ppo_relu_nav_33": ("nav", 33, "ppo_relu", None, ENV_DYN, False),
    "ppo_tanh_nav_48": ("nav", 48, "ppo_tanh", None, ENV_DYN, True),
    "shac_hover_48": ("hover", 48, "shac", -1.0, ENV_DYN, False),
    "bptt_sac_nav_33": ("nav", 33, "bptt_sac", None, ENV_DYN, False),
    "bptt_sac_tanh_hover_48": ("hover", 48, "bptt_sac_tanh", -1.0, ENV_DYN, True),
    "gate_pi_racing2_48": ("racing2", 48, "ppo_gate", -3.0, RACING_DYN, True),
    "ppo_relu_hover_thrust_rk4_nodelay_48": ("hover", 48, "ppo_relu", -1.0, THRUST_RK4, False),
}


@pytest.mark.parametrize("case", list(G3))
def test_g3_persistent_launch_equals_the_loop(case):
    check_persistent_launch_equals_the_loop(case, *G3[case])


def check_persistent_launch_equals_the_loop(case, kind, N, name, bias, dyn, generated):
    """the body of test_g3_persistent_launch_equals_the_loop; tests/test_delay_ring_gpu.py runs it with other delay-ring depths in `dyn`.
    -> (the model, the loop's result)"""
    from visfly_amd import _lib
    from visfly_amd.evaluate import evaluate_policy
    model = make_model(name, make_env(kind, N, dyn=dyn, **({"requires_grad": True} if name in ("shac", "bptt_sac", "bptt_sac_tanh") else {})))
    if bias is not None:
        bias_thrust(model.policy, bias)
    assert bool(getattr(model.policy, "chain_jit", False)) == generated
    loop = evaluate_policy(model, make_env(kind, N, seed=11, dyn=dyn), persistent=False, terminal_rows=True)
    lengths = loop.ep_length.cpu().numpy()
    print(f"{case}: episode lengths {dict(zip(*np.unique(lengths, return_counts=True)))}, successes {int(loop.is_success.sum())}")
    assert loop.path == "loop"
    assert len(set(lengths.tolist())) >= 2 and (lengths < T).any() and (lengths == T).any(), lengths
    n0 = _lib.lib().vf_chain_plugin_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pers = evaluate_policy(model, make_env(kind, N, seed=11, dyn=dyn), terminal_rows=True)
    assert pers.path == "persistent"
    if generated:
        assert _lib.lib().vf_chain_plugin_launches() > n0
    assert torch.equal(pers.ep_length, loop.ep_length) and torch.equal(pers.flags, loop.flags)
    assert bits_equal(pers.ep_return, loop.ep_return) and bits_equal(pers.terminal_state, loop.terminal_state)
    assert torch.equal(pers.is_success, loop.is_success)
    # without the terminal rows: the same episodes
    p2 = evaluate_policy(model, make_env(kind, N, seed=11, dyn=dyn))
    assert p2.path == "persistent" and p2.terminal_state is None and bits_equal(p2.ep_return, loop.ep_return) and torch.equal(p2.flags, loop.flags)
    return model, loop


# ---- G4: needs-reset rule -----------------------------------------------------------------------------------------------------------
def test_g4_env_needs_a_reset_and_is_the_same_after_it():
    from visfly_amd.evaluate import evaluate_policy
    N = 48
    model = make_model("ppo_relu", make_env("hover", N))
    bias_thrust(model.policy, -1.0)
    A, B = make_env("hover", N, seed=11), make_env("hover", N, seed=11)
    ra, rb = evaluate_policy(model, A), evaluate_policy(model, B, persistent=False)
    assert (ra.path, rb.path) == ("persistent", "loop") and bits_equal(ra.ep_return, rb.ep_return)
    assert len(set(ra.ep_length.cpu().tolist())) >= 2          # waves left the launch at different steps
    g = torch.Generator(device=DEV).manual_seed(1)
    acts = torch.rand((3, N, 4), device=DEV, generator=g) * 2 - 1
    for env in (A, B):
        with pytest.raises(AssertionError, match="reset"):
            env.step(acts[0])
    oa, ob = A.reset(), B.reset()
    assert bits_equal(oa["state"], ob["state"])
    for t in range(3):
        (oa, rwa, da, _), (ob, rwb, db, _) = A.step(acts[t]), B.step(acts[t])
        assert bits_equal(oa["state"], ob["state"]) and bits_equal(rwa, rwb) and torch.equal(da, db), t
    assert bits_equal(A.state_slab, B.state_slab)


# ---- G5: fall-backs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["wide_network", "imu_noise"])
def test_g5_fallbacks_take_the_loop_with_one_warning(why):
    from visfly_amd import _lib
    from visfly_amd.evaluate import evaluate_policy
    N = 33
    kw = {}
    if why == "imu_noise":
        kw["random_kwargs"] = dict(HOVER_FLOOR, noise_kwargs={"IMU": {"model": "UniformNoiseModel", "kwargs": {"mean": [0.0] * 13, "half": [0.01] * 13}}})
    model = make_model("ppo_wide" if why == "wide_network" else "ppo_relu", make_env("hover", N))
    bias_thrust(model.policy, -1.0)
    assert (model.policy._plan is None) == (why == "wide_network")
    _lib._warned.discard("evaluate_policy")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = evaluate_policy(model, make_env("hover", N, seed=11, **kw))
        again = evaluate_policy(model, make_env("hover", N, seed=11, **kw))
    assert res.path == "loop" and again.path == "loop"
    assert len([x for x in w if "persistent evaluation" in str(x.message)]) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = reference_rule(model, make_env("hover", N, seed=11, **kw))
    assert_is_reference(res, ref)
    assert bits_equal(again.ep_return, res.ep_return)


# ---- G6: trainers ---------------------------------------------------------------------------------------------------------------------
NEW_KEYS = {"rollout/ep_rew_mean", "rollout/ep_len_mean", "rollout/success_rate", "eval/ep_rew_mean", "eval/ep_len_mean", "eval/success_rate"}


@pytest.mark.parametrize("trainer", ["shac", "bptt", "ppo"])
def test_g6_learn_with_and_without_eval_env(trainer):
    from visfly_amd.bptt import BPTT
    from visfly_amd.evaluate import EpisodeWindow
    from visfly_amd.ppo import PPO
    from visfly_amd.shac import SHAC
    N, H = 48, 4

    def run(with_eval):
        env = make_env("hover", N, **({} if trainer == "ppo" else {"requires_grad": True}))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if trainer == "shac":
                algo = SHAC(env, horizon=H, gradient_steps=1, learning_rate=1e-3, seed=7, dump_step=H * N)
            elif trainer == "bptt":
                algo = BPTT(env, horizon=H, learning_rate=1e-3, seed=7, dump_step=H * N)
            else:
                algo = PPO(env, n_steps=H, batch_size=H * N, n_epochs=1, seed=2, policy_kwargs=dict(activation_fn="relu"))
        assert trainer == "ppo" or algo.dump_step == H * N
        updates = 1 if trainer == "ppo" else 3
        algo.learn(updates * H * N, **({"eval_env": make_env("hover", N, seed=11)} if with_eval else {}))
        return algo

    plain, ev = run(False), run(True)
    assert bits_equal(plain.policy.flat, ev.policy.flat)
    if trainer == "shac":
        assert bits_equal(plain.critic.flat, ev.critic.flat) and bits_equal(plain.critic_target.flat, ev.critic_target.flat)
    today = {"shac": {"train/actor_loss", "train/critic_loss", "time/fps"}, "bptt": {"train/actor_loss", "time/fps"}}
    if trainer != "ppo":
        assert set(plain.logs) == today[trainer]
        assert set(ev.logs) == today[trainer] | NEW_KEYS
        assert ev._noise_step == plain._noise_step and torch.equal(ev._gen.get_state(), plain._gen.get_state())
    else:
        assert not any(k.startswith("eval/") for k in plain.logs) and "rollout/success_rate" not in plain.logs
        assert {"rollout/success_rate", "eval/ep_rew_mean", "eval/ep_len_mean", "eval/success_rate"} <= set(ev.logs) - set(plain.logs) <= NEW_KEYS
        assert ev._sample_step == plain._sample_step
    assert all(np.isfinite(ev.logs[k]) for k in NEW_KEYS)
    # the reference's test (BPTT.py:137,174) fires once in three updates at dump_step = one update; PPO evaluates after its iteration
    results = ev._eval_schedule.results
    assert len(results) == 1 and results[0].path == "persistent"
    win = EpisodeWindow()
    for res in results:
        win.extend(res)
    assert {k: ev.logs[k] for k in win.means()} == win.means()
    assert ev.logs["eval/ep_rew_mean"] == pytest.approx(results[-1].mean_r, rel=1e-12) and ev.logs["eval/ep_len_mean"] == results[-1].mean_l
    assert ev.logs["eval/success_rate"] == results[-1].success_rate
