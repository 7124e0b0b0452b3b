"""The env adjoint under string wind functions (six ``wind_settings`` expressions, re-evaluated on the host before every step) against
the reference's torch autograd: on its tape the wind is a per-step constant, here the tape keeps the per-agent rows every recorded step
ran with and the reverse pass replays the interval with them (vf_env_step_bwd_wind / vf_dyn_step_bwd_wind).

Fixtures: tools/gen_wind_golden.py (the recorders of oracle/ with the wind strings of dyn_wind_functions).  N = 70, H = 12: a last
block with dead lanes behind the last wind row, and a step index that matters (the wind changes from step to step and, in the resets
and navigation fixtures, jumps where an agent re-spawns with a new t).  The wind moves the reference's own gradient by 98 x / 154 x the
1e-5 the adjoint is held to (tests/test_wind_adjoint.py), so an adjoint that ignores the wind, or takes another step's, fails here."""
import ast
import ctypes as C

import numpy as np
import pytest
import torch

from _golden import assert_bits_equal, consts_of, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIND = ["0.3 - 0.05*x", "0.02*x*x", "0.5*y + 0.1", "0*x + 0.125", "-0.01*x", "0.25*y - 0.05"]      # dyn_wind_functions'
WIND_DYN = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True, wind_settings=WIND)
EINVAL, EUNSUPPORTED = -1, -4


@pytest.mark.parametrize("name", ["bptt_wind_hover", "bptt_wind_hover_resets", "bptt_wind_nav_rk4"])
def test_action_gradients_match_reference_autograd_under_wind(name):
    """check_action_gradients as it stands (forward reward bits, done flags, dL/da to 1e-5 of its largest entry), and the rows the
    tape recorded are the reference's wind_velocity of every step, bit for bit"""
    from test_bptt_gpu import check_action_gradients
    env, fx = check_action_gradients(name)
    H = fx["actions"].shape[0]
    assert env._tape_wind.shape == (H, fx["actions"].shape[1], 4)
    assert_bits_equal(env._tape_wind[:H, :, :3].cpu().numpy(), fx["wind"], f"{name}: wind rows on the tape")
    # the gradient without the wind is NOT within the bound (what the fixture is for)
    if name != "bptt_wind_nav_rk4":
        assert np.abs(fx["d_actions_nowind"] - fx["d_actions"]).max() > 50 * 1e-5 * np.abs(fx["d_actions"]).max()
    env.close()


def test_requires_grad_env_step_through_torch_autograd_under_wind():
    """the body of test_requires_grad_env_step_through_torch_autograd (tests/test_bptt_gpu.py) on bptt_wind_hover: EnvStepFunction
    goes through backward_step, so a plain loss.backward() carries the wind rows"""
    from visfly_amd.envs import HoverEnv
    fx = load("bptt_wind_hover")
    H, N = fx["actions"].shape[:2]
    env = HoverEnv(num_agent_per_scene=N, seed=int(fx["seed"]), dynamics_kwargs=ast.literal_eval(str(fx["dyn_kw"])),
                   device=DEV, tensor_output=True, requires_grad=True, max_episode_steps=1000, constants=consts_of(fx))
    env.reset(state=torch.from_numpy(fx["fs_init"]))
    acts = torch.from_numpy(fx["actions"]).cuda().requires_grad_(True)
    Wr, Wo = torch.from_numpy(fx["Wr"]).cuda(), torch.from_numpy(fx["Wo"]).cuda()
    loss = 0
    for t in range(H):
        obs, r, d, _ = env.step(acts[t])
        assert r.requires_grad and obs["state"].requires_grad
        loss = loss + (Wr[t] * r).sum() + (Wo[t] * obs["state"]).sum()
    assert abs(float(loss.detach()) - float(fx["loss"])) < 1e-3 * max(1.0, abs(float(fx["loss"])))
    loss.backward()
    want = fx["d_actions"]
    assert np.abs(acts.grad.cpu().numpy() - want).max() <= 2e-3 * np.abs(want).max()
    env.detach()
    assert env._tape_t == 0
    env.close()


def test_dynamics_only_adjoint_under_wind_equals_the_env_adjoint_without_reward():
    """a bare Dynamics with wind functions next to a HoverEnv twin from the same state: Dynamics.backward_step(..., wind=rows of that
    step) == env.backward_step(d_reward=None), bit for bit in d_action and the adjoint slab; without the rows it raises"""
    from visfly_amd import Dynamics
    from visfly_amd._lib import G_VEL
    from visfly_amd.envs import HoverEnv
    N, H = 70, 6
    g = torch.Generator(device=DEV).manual_seed(4)
    env = HoverEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(WIND_DYN), device=DEV, tensor_output=True, max_episode_steps=1000,
                   spawn_prefetch=False)
    env.reset()
    fs = env.full_state.clone()
    fs[:, 7:10] = env.envs.dynamics._vec(G_VEL)       # full_state carries v + wind; seed the raw velocity
    dyn = Dynamics(num=N, device=DEV, **WIND_DYN)
    dyn.reset(pos=fs[:, 0:3], ori=fs[:, 3:7], vel=fs[:, 7:10], ori_vel=fs[:, 10:13], motor_omega=fs[:, 13:17], thrusts=fs[:, 17:21], t=fs[:, 21])
    acts = (torch.tensor([-1 / 3, 0, 0, 0], device=DEV) + (torch.rand((H, N, 4), device=DEV, generator=g) * 2 - 1) * 0.3).clamp(-1, 1)
    W = torch.randn((H, N, 13), device=DEV, generator=g)
    env.enable_tape(H)
    tapes, rows = [], []
    for t in range(H):
        tapes.append(dyn._slab.clone())
        s = dyn.step(acts[t])
        rows.append(dyn.wind_rows)
        o, _, d, _ = env.step(acts[t], is_test=True)
        assert torch.equal(s, o["state"]) and not d.any()
        assert torch.equal(rows[t], env._tape_wind[t]) and rows[t] is not dyn._wind_rows
    assert not torch.equal(rows[0], rows[-1]) and float(rows[-1][:, :3].abs().max()) > 0.1
    with pytest.raises(ValueError, match="rows that step ran with"):
        dyn.backward_step(tapes[-1], acts[-1], W[-1], torch.zeros_like(dyn._slab))
    adj = torch.zeros_like(dyn._slab)
    G = min(adj.shape[1], env._adj.shape[1])
    nonzero = 0.0
    for t in reversed(range(H)):
        da_env = env.backward_step(t, d_obs=W[t], d_reward=None)
        da_dyn = dyn.backward_step(tapes[t], acts[t], W[t], adj, wind=rows[t])
        assert torch.equal(da_env.view(torch.int32), da_dyn.view(torch.int32)), f"step {t}"
        assert torch.equal(adj[:, :G].view(torch.int32), env._adj[:, :G].view(torch.int32)), f"adjoint slab after step {t}"
        nonzero = max(nonzero, float(da_dyn.abs().max()))
    assert nonzero > 0.0 and float(adj.abs().max()) > 0.0
    env.close()


def _bwd_args(env, t, d_obs, d_reward, adj, d_action):
    from visfly_amd import _lib
    a = _lib.EnvBwdArgs()
    a.tape_slab, a.action = env._tape[t].data_ptr(), env._tape_actions[t].data_ptr()
    a.d_obs, a.d_reward = d_obs.data_ptr(), d_reward.data_ptr()
    a.done, a.adj_slab, a.d_action = env._tape_done[t].data_ptr(), adj.data_ptr(), d_action.data_ptr()
    return a


def test_entry_points_without_rows_are_the_old_calls_and_the_old_calls_still_refuse_wind():
    """no regression by construction: on an env without wind functions vf_env_step_bwd_wind(..., NULL) and vf_env_step_bwd leave the
    same bits and the tape has no wind buffer; on a wind env the old entry point still answers VF_EUNSUPPORTED (it cannot know the
    step's rows), so does the new one without rows, and misaligned rows are VF_EINVAL before any device work"""
    from visfly_amd import _lib
    from visfly_amd.envs import HoverEnv
    from _golden import ENV_DYN
    L, st = _lib.lib(), _lib.current_stream(torch.device(DEV))
    N, H = 70, 4
    g = torch.Generator(device=DEV).manual_seed(9)
    acts = (torch.tensor([-1 / 3, 0, 0, 0], device=DEV) + (torch.rand((H, N, 4), device=DEV, generator=g) * 2 - 1) * 0.3).clamp(-1, 1)
    d_obs, d_rew = torch.randn((N, 13), device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    for windy in (False, True):
        env = HoverEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(WIND_DYN if windy else ENV_DYN), device=DEV, tensor_output=True,
                       max_episode_steps=3)
        env.reset()
        env.enable_tape(H)
        assert (env._tape_wind is not None) == windy
        for t in range(H):
            env.step(acts[t])
        assert env._tape_done.any()                      # episode ends inside the horizon
        t = H - 2
        adj0 = torch.randn(env._adj.shape, device=DEV, generator=g)
        outs = []
        for entry in ("old", "new"):
            adj, da = adj0.clone(), torch.full((N, 4), float("nan"), device=DEV)
            a = _bwd_args(env, t, d_obs, d_rew, adj, da)
            rc = L.vf_env_step_bwd(env._h, C.byref(a), st) if entry == "old" else L.vf_env_step_bwd_wind(env._h, C.byref(a), None, st)
            assert rc == (EUNSUPPORTED if windy else 0), (entry, windy, rc)
            outs.append((adj, da))
        if not windy:
            assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
            assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)) and torch.isfinite(outs[0][1]).all()
        else:
            assert torch.equal(outs[0][0], adj0) and torch.isnan(outs[1][1]).all()         # refused: nothing was launched
        rows = torch.zeros((N + 1, 4), device=DEV)
        a = _bwd_args(env, t, d_obs, d_rew, adj0.clone(), torch.empty((N, 4), device=DEV))
        assert L.vf_env_step_bwd_wind(env._h, C.byref(a), _lib.ptr(rows.view(-1)[1:]), st) == EINVAL
        dyn = env.envs.dynamics
        assert L.vf_dyn_step_bwd_wind(dyn._h, _lib.ptr(env._tape[t]), _lib.ptr(acts[t]), None, _lib.ptr(adj0.clone()), _lib.ptr(torch.empty((N, 4), device=DEV)),
                                      _lib.ptr(rows.view(-1)[1:]), st) == EINVAL
        # lifecycle: clear_tape keeps the buffer like the other tape buffers, a second enable_tape re-sizes it, requires_grad(False) drops it
        env.clear_tape()
        assert (env._tape_wind is not None) == windy and env._tape_t == 0
        env.enable_tape(2 * H)
        assert (env._tape_wind.shape[0] == 2 * H) if windy else env._tape_wind is None
        env.set_requires_grad(False)
        assert env._tape is None and env._tape_wind is None
        env.close()


def test_bptt_learn_iteration_matches_the_reference_loop_under_wind():
    """the assertions and tolerances of test_bptt_learn_iteration_matches_the_reference_loop_with_its_own_actor (tests/test_bptt_gpu.py)
    on bptt_loop_hover_wind: 71 episode ends in 8 steps, each re-spawn drawing a new t and with it a new wind"""
    from test_bptt_gpu import _make_loop
    from test_shac_gpu import blocks_close
    fx = load("bptt_loop_hover_wind")
    env, algo = _make_loop(fx)
    assert env.envs.dynamics._wind_fn is not None
    algo._eps_override = torch.from_numpy(fx["eps"]).to(DEV)
    loss = algo._grad_reverse_sweep()
    n = lambda t: t.cpu().numpy()
    r = algo._last_rollout
    assert np.array_equal(n(r["done"]).astype(np.uint8), fx["done"]) and fx["done"].sum() > 0
    for got, want, what in ((r["action"], fx["action"], "actions"), (r["reward"], fx["reward"], "rewards")):
        err = np.abs(n(got) - want).max()
        print(f"BPTT loop under wind, {what}: max abs err {err:.2e}")
        assert err <= 1e-6, what
    assert abs(float(loss) - float(fx["actor_loss"])) <= 2e-6, (float(loss), float(fx["actor_loss"]))
    a = algo.policy
    rel = blocks_close(n(a.grad), fx["actor_grad"], a, 2e-5, 1e-3, "actor gradient of BPTT.learn under wind")
    print(f"actor loss {float(loss):.7f} vs {float(fx['actor_loss']):.7f}; gradient rel err {rel:.2e}")
    a.grad.copy_(torch.from_numpy(fx["actor_grad"]))
    algo._apply(loss)
    assert np.abs(n(a.flat[:a.n_params]) - fx["actor_params1"]).max() <= 2e-7
    assert env._tape_t == 0                               # env.detach()
    env.close()


def test_shac_actor_half_matches_the_reference_loop_under_wind():
    """the actor half of test_one_iteration_matches_the_reference_loop (tests/test_shac_gpu.py) on shac_hover_wind: horizon buffer
    1e-6, loss 2e-6, gradient 2e-5 (blocks 1e-3), parameters after the step 2e-7"""
    from test_shac_gpu import blocks_close, make
    fx = load("shac_hover_wind")
    env, algo = make(fx)
    assert env.envs.dynamics._wind_fn is not None
    algo._eps_override = torch.from_numpy(fx["eps"]).to(DEV)
    loss = algo._grad_reverse_sweep()
    b = algo._buf
    n = lambda t: t.cpu().numpy()
    assert np.array_equal(n(b["done"]), fx["buf_done"]) and np.array_equal(n(b["ep_done"]), fx["buf_episode_done"])
    for got, want, what in ((b["obs"]["state"], fx["buf_obs"], "observations"), (b["action"], fx["buf_action"], "actions"),
                            (b["reward"], fx["buf_reward"], "rewards"), (b["next_value"], fx["buf_next_value"], "next values")):
        err = np.abs(n(got) - want).max()
        print(f"horizon buffer under wind, {what}: max abs err {err:.2e}")
        assert err <= 1e-6, what
    assert abs(float(loss) - float(fx["actor_loss"])) <= 2e-6, (float(loss), float(fx["actor_loss"]))
    a = algo.policy
    rel = blocks_close(n(a.grad), fx["actor_grad"], a, 2e-5, 1e-3, "actor gradient under wind")
    print(f"actor loss {float(loss):.7f} vs {float(fx['actor_loss']):.7f}; gradient rel err {rel:.2e}")
    a.grad.copy_(torch.from_numpy(fx["actor_grad"]))
    algo._apply(loss)
    assert np.abs(n(a.flat[:a.n_params]) - fx["actor_params1"]).max() <= 2e-7
    env.close()


@pytest.mark.parametrize("trainer", ["BPTT", "SHAC"])
def test_trainers_learn_on_a_wind_env(trainer):
    """two iterations of learn() on a 256-agent wind env (launch by launch): parameters finite and changed, the tape rewound"""
    from visfly_amd.bptt import BPTT
    from visfly_amd.envs import HoverEnv
    from visfly_amd.shac import SHAC
    N, H = 256, 8
    env = HoverEnv(num_agent_per_scene=N, seed=5, dynamics_kwargs=dict(WIND_DYN), device=DEV, tensor_output=True, requires_grad=True,
                   max_episode_steps=12)
    algo = (BPTT(env, horizon=H, learning_rate=1e-3, seed=1) if trainer == "BPTT"
            else SHAC(env, horizon=H, gradient_steps=2, learning_rate=1e-3, seed=1))
    p0 = algo.policy.flat.clone()
    algo.learn(2 * H * N)
    assert torch.isfinite(algo.policy.flat).all() and not torch.equal(p0, algo.policy.flat)
    assert env._tape_t == 0 and env._tape_wind is not None
    assert float(env.envs.dynamics.wind_velocity.abs().max()) > 0.1
    env.close()
