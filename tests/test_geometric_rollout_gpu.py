"""The persistent PPO roll-out (vf_ppo_rollout) and evaluation launch (vf_eval_rollout) for the velocity / position action types -- the
geometric SO(3) controller of envs/base/dynamics.py:414-496, evaluated once per control step inside the launch -- against the
launch-by-launch loop, bit for bit: built-in and generated classes, 16 and 32 rows per wave, Euler and RK4, with and without motor lag,
the racing kind.  What stays declined: the BPTT horizon launches and the BPTT / SHAC trainers (the reference has no gradient for these two
action types), and per-agent wind rows.

The velocity controller has a branch on the horizontal speed (auto-yaw above 0.1 m/s, dynamics.py:421-427): every velocity case asserts,
from the recorded observation rows, that both sides occur in at least 1 % of the rows each.  Agents that spawn at rest do not get there
within the 7-step episodes of these tests, whatever the policy commands (measured on an MI355X: the largest horizontal speed of any recorded
row is 0.017 m/s with the motor lag, 0.038 m/s without; a mean head biased to the full velocity command changes neither; 20-step episodes
reach 0.6 m/s).  So the velocity cases start their episodes moving: HoverEnv / NavigationEnv spawn with a horizontal velocity of up to
0.2 m/s per axis (about 0.8 of the rows above the threshold), and the racing env, whose spawn boxes are the reference's fixed ones, is
reset(state=...) to such velocities before the first roll-out (its first episode; 0.14 of the rows of both rounds)."""
import warnings

import numpy as np
import pytest
import torch

from _golden import ENV_DYN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOVER_BOX, NAV_BOX = {"mean": [1., 0., 1.5], "half": [1.0, 1.0, 0.5]}, {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}      # (HoverEnv's default box)
NAV_SPAWN = {"state_generator": {"class": "Uniform", "kwargs": [{"position": NAV_BOX}]}}
MOVING = {"mean": [0., 0., 0.], "half": [0.2, 0.2, 0.1]}
moving_spawn = lambda box: {"state_generator": {"class": "Uniform", "kwargs": [{"position": box, "velocity": MOVING}]}}


def _dynamics(action_type, dyn):
    dkw = dict(ENV_DYN, action_type=action_type)
    if dyn.startswith("rk4"):
        dkw["integrator"] = "rk4"
    if dyn.endswith("nodelay"):
        dkw["ctrl_delay"] = False
    return dkw


def _yaw_branch_fractions(state_rows):
    """fractions of the recorded "state" rows on either side of the velocity controller's ||v_xy|| > 0.1 branch (the wind is zero: the
    observed velocity is the agent's).  13-wide rows hold v in columns 7:10; RacingEnv2's 16 gate-relative columns hold v / 10 in 10:13"""
    rows = state_rows.reshape(-1, state_rows.shape[-1]).double()
    vxy = rows[:, 7:9] if rows.shape[-1] == 13 else rows[:, 10:12] * 10.0
    above = float((vxy.norm(dim=1) > 0.1).double().mean())
    return above, 1.0 - above


def _persistent_rollout_vs_loop(env_name, N, action_type, dyn, policy_kwargs=None, max_episode_steps=7, n_steps=20):
    """collect_rollouts as ONE launch leaves the rollout buffer, the TimeLimit list, the episode statistics, the episode outputs and the
    slab of the launch-by-launch loop, bit for bit -- over two consecutive rollouts with a training pass between them (Philox counters,
    delay-ring phase and spawn counters carry over).  (tests/test_ppo_gpu.py's helper, with the env's action type as an argument)"""
    import visfly_amd.envs as E
    from visfly_amd.ppo import PPO
    dkw = _dynamics(action_type, dyn)
    res = []
    for fused in (True, False):
        kw = {}
        if env_name == "NavigationEnv":       # its default spawn box is the origin, i.e. inside the floor
            kw["random_kwargs"] = NAV_SPAWN
        if action_type == "velocity" and env_name in ("HoverEnv", "NavigationEnv"):       # both sides of the yaw branch: see the module's docstring
            kw["random_kwargs"] = moving_spawn(NAV_BOX if env_name == "NavigationEnv" else HOVER_BOX)
        env = getattr(E, env_name)(num_agent_per_scene=N, seed=5, dynamics_kwargs=dict(dkw), device=DEV, max_episode_steps=max_episode_steps,
                                   tensor_output=True, **kw)
        assert int(env.envs.dynamics.constants["action_type"]) == {"velocity": 2, "position": 3}[action_type]
        ppo = PPO(env, n_steps=n_steps, batch_size=N * n_steps // (4 if N < 16000 else 20), n_epochs=1, seed=2,
                  policy_kwargs=policy_kwargs or dict(activation_fn="relu"))
        ppo.fused_rollout = fused
        if action_type == "velocity" and "random_kwargs" not in kw:
            # the racing envs take no spawn box from the caller: the first episode starts from the env's own spawn with MOVING's velocities
            env.reset()
            fs = env.full_state.clone()          # (N, 22): p, q, v, w, motor speeds, thrusts, t
            u = torch.rand((N, 3), generator=torch.Generator().manual_seed(9)) * 2 - 1
            fs[:, 7:10] = (u * torch.tensor(MOVING["half"])).to(fs.device)
            ppo._last_obs, ppo._last_starts = env.reset(state=fs), torch.ones(N, device=DEV)
        out, fractions = {}, []
        for rnd in range(2):
            ppo.collect_rollouts()
            torch.cuda.synchronize()
            assert ppo.fused_rollout is fused                 # the kernel was not refused
            for k in ("rewards", "values", "advantages", "returns", "episode_starts", "log_probs", "actions"):
                out[f"{rnd}:{k}"] = getattr(ppo.buf, k).clone()
            for k in ppo.obs_keys:
                out[f"{rnd}:obs:{k}"] = ppo.buf.obs[k].clone()
                out[f"{rnd}:last:{k}"] = ppo._last_obs[k].clone()
            cnt = int(ppo._boot["cursor"].item())
            order = torch.argsort(ppo._boot["idx"][:cnt])
            out[f"{rnd}:boot_idx"] = ppo._boot["idx"][:cnt][order].clone()
            out[f"{rnd}:boot_rows"] = ppo._boot["rows0"][:cnt][order].clone()
            assert cnt >= N * 2                               # bootstrapped truncations: every agent's episode ends at least twice
            out[f"{rnd}:stat"] = ppo._boot["stat"].clone()
            sl = env.state_slab                               # padded to whole workgroups; pad agents are nobody's state
            out[f"{rnd}:slab"] = sl.transpose(-3, -4).reshape(sl.shape[-3], -1, 4)[:, :N].clone()
            out[f"{rnd}:starts"] = ppo._last_starts.clone()
            out[f"{rnd}:ep"] = torch.stack([env._ep_return, env._ep_length.float(), env._ep_flags.float()]).clone()
            if env._OBS_W == 13:      # (RacingEnv2: the launch's terminal rows are its own 16-column buffer; the truncated ones are compared as boot_rows)
                out[f"{rnd}:terminal"] = env._terminal_obs.clone()
            if action_type == "velocity":
                above, below = _yaw_branch_fractions(ppo.buf.obs["state"])
                print(f"{env_name} {N} {action_type} {dyn} fused={fused} round {rnd}: ||v_xy|| > 0.1 in {above:.3f} of the rows, <= 0.1 in {below:.3f}")
                fractions.append(above)
            if rnd == 0:
                ppo.train()
        out["params"] = ppo.policy.flat.clone()
        if action_type == "velocity":         # of the rows of both rounds (the same number each)
            above = sum(fractions) / len(fractions)
            assert above >= 0.01 and 1.0 - above >= 0.01, fractions
        res.append(out)
        env.close()
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    assert float((res[0]["1:rewards"].abs() > 0).float().mean()) > 0.5
    assert all(bool(torch.isfinite(v).all()) for k, v in res[0].items() if v.dtype == torch.float32 and "slab" not in k)


@pytest.mark.parametrize("env_name,N,action_type,dyn", [
    ("HoverEnv", 5, "velocity", "euler"),                   # one ragged wave, replica lanes
    ("HoverEnv", 1000, "position", "euler"),                # 16 rows per wave, ragged last wave
    ("NavigationEnv", 3000, "velocity", "euler"),           # the two-observation class
    ("NavigationEnv", 16500, "position", "rk4"),            # 32 rows per wave
    ("HoverEnv", 1000, "velocity", "euler_nodelay"),        # no motor lag
    ("RacingEnv2", 3000, "velocity", "euler")])             # racing kind, 16 gate-relative columns
def test_persistent_rollout_equals_the_per_step_loop(env_name, N, action_type, dyn):
    """the built-in actor-critic classes.  `ppo.fused_rollout is fused` inside the helper is the assertion that needs the instances: without
    them vf_ppo_rollout answers VF_EUNSUPPORTED and the trainer switches to the loop for good"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _persistent_rollout_vs_loop(env_name, N, action_type, dyn)


@pytest.mark.parametrize("env_name,N,action_type", [("HoverEnv", 3000, "velocity"), ("NavigationEnv2", 3000, "position")])
def test_persistent_rollout_of_a_generated_class_equals_the_per_step_loop(env_name, N, action_type):
    """a network shape without a built-in chain class: its roll-out plugin is instantiated with the env's action type (visfly_amd/_jit.py:
    ensure_rollout; pre-built: PREBUILD_ROLLOUT) -- the same comparison, no fallback warning, and a plugin served the launch"""
    from visfly_amd import _jit, _lib
    _, ext, pi, vf = _jit.PREBUILD["one_layer_extractor"]
    pk = dict(features_extractor_class="StateExtractor", activation_fn="ReLU",
              features_extractor_kwargs=dict(net_arch={k: dict(layer=v) for k, v in ext.items()}), net_arch=dict(pi=pi, vf=vf))
    n0 = _lib.lib().vf_chain_plugin_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _persistent_rollout_vs_loop(env_name, N, action_type, "euler", policy_kwargs=pk)
    assert _lib.lib().vf_chain_plugin_launches() > n0


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
T = 24
NAV_NEAR = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [9., 0., 1.], "half": [1.2, 1.2, 0.6]}}]}}      # around the default target


def _nav(N, action_type, seed=5):
    import visfly_amd.envs as E
    return E.NavigationEnv(num_agent_per_scene=N, seed=seed, dynamics_kwargs=_dynamics(action_type, "euler"), device=DEV, tensor_output=True,
                           max_episode_steps=T, random_kwargs=NAV_NEAR)


def _bits_equal(a, b):
    return a.shape == b.shape and (torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32)))


@pytest.mark.parametrize("action_type,generated", [("velocity", False), ("position", True)])
def test_persistent_evaluation_equals_the_loop(action_type, generated):
    """the built-in [128, 64] x [64, 64] ReLU class with velocity actions, the generated Tanh class (the reference policy's default
    activations: PREBUILD_ACT["tanh_nav"], evaluation plugin pre-built) with position actions, on NavigationEnv spawned around its target:
    agents inside the success radius finish in their first step, the others at different steps up to the time limit.  N = 48: three 16-row
    waves, one and a half 32-row waves"""
    from visfly_amd import _lib
    from visfly_amd.evaluate import evaluate_policy
    from visfly_amd.ppo import PPO
    N = 48
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = PPO(_nav(N, action_type), n_steps=4, batch_size=4 * N, n_epochs=1, seed=2, policy_kwargs=None if generated else dict(activation_fn="relu"))
    assert bool(getattr(model.policy, "chain_jit", False)) == generated
    A, B = _nav(N, action_type, seed=11), _nav(N, action_type, seed=11)
    loop = evaluate_policy(model, B, persistent=False, terminal_rows=True)
    lengths = loop.ep_length.cpu().numpy()
    print(f"{action_type}: episode lengths {dict(zip(*np.unique(lengths, return_counts=True)))}, successes {int(loop.is_success.sum())}")
    assert loop.path == "loop"
    assert len(set(lengths.tolist())) >= 2 and (lengths < T).any() and (lengths == T).any(), lengths
    n0 = _lib.lib().vf_chain_plugin_launches()
    _lib._warned.discard("evaluate_policy")
    _lib._warned.discard("vf_eval_rollout")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                        # no fallback warning
        pers = evaluate_policy(model, A, terminal_rows=True)
    assert pers.path == "persistent"
    if generated:
        assert _lib.lib().vf_chain_plugin_launches() > n0
    assert torch.equal(pers.ep_length, loop.ep_length) and torch.equal(pers.flags, loop.flags)
    assert _bits_equal(pers.ep_return, loop.ep_return) and _bits_equal(pers.terminal_state, loop.terminal_state)
    assert torch.equal(pers.is_success, loop.is_success)
    assert pers.mean_r == loop.mean_r and pers.mean_l == loop.mean_l and pers.success_rate == loop.success_rate
    assert bool(torch.isfinite(pers.ep_return).all()) and bool(torch.isfinite(pers.terminal_state).all())
    # afterwards the env demands a reset on both paths
    for env in (A, B):
        with pytest.raises(AssertionError, match="reset"):
            env.step(torch.zeros((N, 4), device=DEV))


# ---- what stays declined ------------------------------------------------------------------------------------------------------------------
def _hover(N, action_type, **kw):
    from visfly_amd.envs import HoverEnv
    return HoverEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=_dynamics(action_type, "euler"), device=DEV, max_episode_steps=16,
                    tensor_output=True, **kw)


def test_the_bptt_launch_still_declines_a_velocity_env():
    """vf_bptt_rollout has no velocity instance: asked for one -- with the built-in SAC-style Actor of a trainer constructed over a bodyrate
    env, on a velocity env that records a tape -- it answers VF_EUNSUPPORTED and rollout_policy reports False"""
    from visfly_amd import _lib
    from visfly_amd.bptt import BPTT
    N, H = 64, 4
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bptt = BPTT(_hover(N, "bodyrate", requires_grad=True), policy="MultiInputPolicy", horizon=H, learning_rate=1e-3, seed=7)
    assert not getattr(bptt.policy, "chain_jit", False)
    pol = bptt.policy
    pol.reserve_slots(N, H)
    f = dict(dtype=torch.float32, device=DEV)

    def ask(env):
        env.set_requires_grad(True, horizon=H)
        env.reset()
        _lib._warned.discard("vf_bptt_rollout")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            served = env.rollout_policy(pol, bptt.obs_keys, torch.zeros((H, N, 4), **f), torch.empty((H, N, 4), **f), torch.empty((H, N), **f),
                                        torch.zeros(N, **f), torch.ones(N, **f), 0.99, 1.0 / N)
        torch.cuda.synchronize()
        return served, [str(x.message) for x in w if "vf_bptt_rollout" in str(x.message)]

    served, said = ask(_hover(N, "velocity", requires_grad=True))
    assert served is False and len(said) == 1, (served, said)          # the library was asked and declined (VF_EUNSUPPORTED -> one warning)
    assert "no persistent roll-out for this network class / env kind / dynamics configuration" in said[0]
    # the same call on a bodyrate env is served: the refusal above is the action type's
    served, said = ask(_hover(N, "bodyrate", requires_grad=True))
    assert served is True and not said


@pytest.mark.parametrize("action_type", ["velocity", "position"])
def test_bptt_and_shac_refuse_the_env_in_the_constructor(action_type):
    from visfly_amd.bptt import BPTT
    from visfly_amd.shac import SHAC
    for cls, kw in ((BPTT, dict(horizon=4)), (BPTT, dict(horizon=4, policy="MultiInputPolicy")), (SHAC, dict(horizon=4, gradient_steps=1))):
        env = _hover(64, action_type, requires_grad=True)
        with pytest.raises(NotImplementedError, match=f'{cls.__name__} over action_type="{action_type}"'):
            cls(env, **kw)
        env.close()


def test_ppo_on_a_velocity_env_with_wind_falls_back_to_the_loop():
    """per-agent wind rows (a host-side wind function) stay without a persistent instance, whatever the action type"""
    from visfly_amd.envs import HoverEnv
    from visfly_amd.ppo import PPO
    dkw = dict(_dynamics("velocity", "euler"), wind_settings=["0.3 - 0.05*x", "0.02*x*x", "0.5*y + 0.1", "0*x + 0.125", "-0.01*x", "0.25*y - 0.05"])
    env = HoverEnv(num_agent_per_scene=512, seed=3, dynamics_kwargs=dkw, device=DEV, max_episode_steps=5, tensor_output=True)
    ppo = PPO(env, n_steps=8, batch_size=2048, n_epochs=1, seed=2, policy_kwargs=dict(activation_fn="relu"))
    used = []
    inner = env.collect_policy
    env.collect_policy = lambda *a, **k: used.append(inner(*a, **k)) or used[-1]
    ppo.collect_rollouts()
    ppo.collect_rollouts()
    torch.cuda.synchronize()
    assert used and all(u is False for u in used), used
    assert ppo.fused_rollout is False
    assert torch.isfinite(ppo.buf.advantages).all() and float(ppo._ep_stats[0]) >= 512
    env.close()


def test_ppo_learn_on_a_velocity_env_stays_on_the_persistent_launch():
    import visfly_amd.envs as E
    from visfly_amd.ppo import PPO
    N = 2048
    env = E.NavigationEnv(num_agent_per_scene=N, seed=5, dynamics_kwargs=_dynamics("velocity", "euler"), device=DEV, max_episode_steps=12,
                          tensor_output=True, random_kwargs=NAV_SPAWN)
    ppo = PPO(env, n_steps=16, batch_size=N * 4, n_epochs=1, seed=2, policy_kwargs=dict(activation_fn="relu"))
    episodes, train = [], ppo.train
    # (train() folds the roll-out's episode statistics into logs["rollout/episodes"] and clears them: one entry per iteration)
    ppo.train = lambda *a, **k: (train(*a, **k), episodes.append(ppo.logs["rollout/episodes"]))[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ppo.learn(total_timesteps=2 * 16 * N)                 # two iterations
    torch.cuda.synchronize()
    assert ppo.num_timesteps == 2 * 16 * N and len(episodes) == 2
    assert ppo.fused_rollout is True
    assert bool(torch.isfinite(ppo.policy.flat).all())
    assert sum(episodes) > N, episodes                        # 32 steps of 12-step episodes: every agent ends two
    env.close()
