"""The navigation adjoint with an obstacle table against the reference's own autograd: tests/golden/bptt_nav_obstacles.npz
(tools/gen_obstacle_golden.py: NavigationEnv, N = 64, H = 12, bodyrate, Euler; the reference's update_collision handed the closest point of
tests/_obstacle_ref.py, so that collision_vector = collision_point.detach() - position is formed and differentiated by the reference
itself).  Bounds: those tests/test_bptt_gpu.py holds its navigation fixtures to -- its REL_TOL of the global scale, and max(1e-5,
4 noise_rel) of the agent's own scale on the judged agents, noise_rel from this fixture's own double-precision run."""
import ast

import numpy as np
import pytest
import torch

from _golden import assert_bits_equal, consts_of, load
from test_bptt_gpu import REL_TOL

pytestmark = pytest.mark.gpu
NAME = "bptt_nav_obstacles"


def _env(fx, table, **kw):
    from visfly_amd.envs import NavigationEnv
    H, N = fx["actions"].shape[:2]
    env = NavigationEnv(num_agent_per_scene=N, seed=int(fx["seed"]), dynamics_kwargs=ast.literal_eval(str(fx["dyn_kw"])), device="cuda:0",
                        tensor_output=True, max_episode_steps=int(fx["max_episode_steps"]), constants=consts_of(fx),
                        target=fx["target"].tolist(), is_collision_reset=bool(fx["is_collision_reset"]),
                        scene_kwargs=dict(obstacles=table), **kw)
    env.reset(state=torch.from_numpy(fx["fs_init"]))
    return env


def _check(got, fx, what):
    want = fx["d_actions"]
    scale, err = np.abs(want).max(), np.abs(got - want).max()
    tol = max(1e-5, 4.0 * float(fx["noise_rel"]))
    own, own_err = np.abs(want).max((0, 2)), np.abs(got - want).max((0, 2))
    held = fx["judged"].astype(bool)
    worst = int(np.argmax(np.where(held, own_err / np.maximum(own, 1e-30), 0)))
    print(f"{what}: max|dL/da| {scale:.3e} err {err:.3e} rel {err / scale:.2e} (bound {REL_TOL:.0e}); per agent bound {tol:.2e} on {int(held.sum())} "
          f"agents, worst {worst}: rel {own_err[worst] / own[worst]:.2e}")
    assert held.any()
    assert np.all(own_err[held] <= tol * own[held]), (worst, own_err[worst], own[worst], tol)
    assert err <= REL_TOL * scale, (err, scale)


def test_fixture_takes_the_obstacle_branches():
    """obstacle winners on both sides of relu(1 - dis) and of the approach relu, in every step; >= 90 % of the agents on the same sides in
    the double-precision run (the generator's own condition), the table as the env parses it"""
    fx = load(NAME)
    names = [str(x) for x in fx["obst_count_names"]]
    assert names == ["winners", "near", "far", "approaching", "receding"]
    assert (fx["obst_counts"].sum(axis=0) > 0).all(), fx["obst_counts"].sum(axis=0)
    assert (fx["obst_counts"][:, 0] > 0).all()
    assert fx["same64"].mean() >= 0.9 and fx["judged"].sum() > 0
    assert len(ast.literal_eval(str(fx["obstacles"]))) == fx["obstacle_rows"].shape[0] == 3
    assert fx["actions"].shape == (12, 64, 4) and str(fx["kind"]) == "nav"


def test_action_gradients_match_reference_autograd_with_obstacles():
    """manual tape + backward_step: rewards, done flags and post-step states bit for bit, then dL/da within the bounds; the same roll-out
    without the table misses the global bound by far (the obstacle terms carry gradient)"""
    fx = load(NAME)
    table = ast.literal_eval(str(fx["obstacles"]))
    H, N = fx["actions"].shape[:2]
    acts = torch.from_numpy(fx["actions"]).cuda()
    grads = {}
    for key, tab in (("table", table), ("bare", [])):
        env = _env(fx, tab)
        env.enable_tape(H)
        for t in range(H):
            obs, r, d, _ = env.step(acts[t], is_test=True)
            if key == "table":
                assert_bits_equal(r.cpu().numpy(), fx["reward"][t], f"forward reward @ {t}")
                assert np.array_equal(d.cpu().numpy().astype(np.uint8), fx["done"][t])
                assert_bits_equal(env.full_state.cpu().numpy(), fx["state"][t], f"post-step state @ {t}")
            assert not (fx["ev_step"] == t).any()
        got = np.zeros_like(fx["d_actions"])
        for t in reversed(range(H)):
            got[t] = env.backward_step(t, d_obs=torch.from_numpy(fx["Wo"][t]), d_reward=torch.from_numpy(fx["Wr"][t])).cpu().numpy()
        grads[key] = got
    _check(grads["table"], fx, "backward_step")
    moved = np.abs(grads["bare"] - fx["d_actions"]).max() / (REL_TOL * np.abs(fx["d_actions"]).max())
    print(f"without the table dL/da is off by {moved:.0f} x the global bound")
    assert moved >= 50


def test_requires_grad_env_with_obstacles_through_torch_autograd():
    """requires_grad=True: step() returns graph-attached obs / reward, loss.backward() runs the OBST adjoint launches; same bounds"""
    fx = load(NAME)
    table = ast.literal_eval(str(fx["obstacles"]))
    H, N = fx["actions"].shape[:2]
    env = _env(fx, table, requires_grad=True)
    acts = torch.from_numpy(fx["actions"]).cuda().requires_grad_(True)
    Wr, Wo = torch.from_numpy(fx["Wr"]).cuda(), torch.from_numpy(fx["Wo"]).cuda()
    loss = 0
    for t in range(H):
        obs, r, d, _ = env.step(acts[t], is_test=True)
        assert r.requires_grad and obs["state"].requires_grad
        assert_bits_equal(r.detach().cpu().numpy(), fx["reward"][t], f"forward reward @ {t}")
        assert np.array_equal(d.cpu().numpy().astype(np.uint8), fx["done"][t])
        loss = loss + (Wr[t] * r).sum() + (Wo[t] * obs["state"]).sum()
    assert abs(float(loss.detach()) - float(fx["loss"])) < 1e-3 * max(1.0, abs(float(fx["loss"])))
    loss.backward()
    _check(acts.grad.cpu().numpy(), fx, "autograd")
