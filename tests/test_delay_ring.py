"""The action delay ring at depths other than the default 3 (delay_steps = int(comm_delay / ctrl_dt)): the depth mapping of
visfly_amd.constants, and conditions on the INPUTS of the GPU tests (tests/test_delay_ring_gpu.py) -- each gradient fixture generated at
depth 1, 4 or 5 (oracle/gen_golden.py::BPTT_CASES, bptt_*_delay*) is recounted in numpy from its actions, done flags and depth: actions
leave the ring and reach live agents, the reference's gradient is non-zero on enough steps, every agent ends an episode inside the
horizon, and the gradient is exactly zero where the recount says the action never left the ring.  No GPU."""
import numpy as np
import pytest

from _golden import consts_of, load
from test_bptt_fixture_coverage import applied_thrust_actions
from visfly_amd.constants import derive_constants

# fixture -> (depth, max_episode_steps, horizon)
GRAD_FIXTURES = {"bptt_hover_delay1": (1, 5, 12), "bptt_hover_rk4_delay4": (4, 9, 20), "bptt_hover_thrust_delay5": (5, 9, 20)}
DYN_FIXTURES = {"dyn_thrust_delay1": 1, "dyn_bodyrate_rk4_delay4": 4, "dyn_bodyrate_delay5": 5}


def applied_to_live(actions, done, D):
    """(H, N) bool: step t applies a NON-ZERO action (the one given D steps earlier, unless a re-spawn zeroed the ring in between) to an
    agent that does not end its episode in that step.  The replay is test_bptt_fixture_coverage.applied_thrust_actions, general in D."""
    done = np.asarray(done).astype(bool)
    a = applied_thrust_actions({"actions": np.asarray(actions, np.float32), "done": done, "c_delay_steps": D})
    return (a != 0).any(-1) & ~done


def never_leaves_the_ring(done, D):
    """(H, N) bool: the action given in step t is still in the ring when the agent's episode ends (the re-spawn zeroes the slots) or
    when the horizon does.  It is applied in step t + D; e = the agent's first done step at or after t, or the last step of the horizon."""
    done = np.asarray(done).astype(bool)
    H, N = done.shape
    end = np.full(N, H - 1)
    out = np.zeros((H, N), bool)
    for t in reversed(range(H)):
        end = np.where(done[t], t, end)
        out[t] = t + D > end
    return out


@pytest.mark.parametrize("comm_delay,depth", [(0.02, 1), (0.04, 2), (0.08, 4), (0.09, 4), (0.1, 5), (0.12, 6), (1.28, 64), (1.3, 65)])
def test_depth_mapping(comm_delay, depth):
    c = derive_constants(action_type="bodyrate", dt=0.0025, ctrl_dt=0.02, comm_delay=comm_delay)
    assert c["delay_steps"].dtype == np.int32 and int(c["delay_steps"]) == depth


DYN_KW = {"dyn_thrust_delay1": dict(action_type="thrust", comm_delay=0.02),
          "dyn_bodyrate_rk4_delay4": dict(action_type="bodyrate", comm_delay=0.09, integrator="rk4"),
          "dyn_bodyrate_delay5": dict(action_type="bodyrate", comm_delay=0.1)}


@pytest.mark.parametrize("name", sorted(DYN_FIXTURES))
def test_dynamics_fixture_is_at_its_depth(name):
    """... and the host-side constants of that configuration are the reference's, bit for bit (as tests/test_constants.py)"""
    fx = load(name)
    assert int(fx["c_delay_steps"]) == DYN_FIXTURES[name]
    assert fx["actions_q"].shape[0] == 256 > DYN_FIXTURES[name]
    want = consts_of(fx)
    got = derive_constants(dt=0.0025, ctrl_dt=0.02, ctrl_delay=True, **DYN_KW[name])
    assert set(want) <= set(got)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


def test_recount_helpers_on_a_hand_made_case():
    """D = 2, one agent, episode end in step 3: actions of steps 0, 1 are applied in 2, 3; those of 2, 3 are zeroed by the re-spawn;
    4 is applied in 6; 5, 6 are still in the ring when the horizon ends"""
    a = np.arange(1, 8, dtype=np.float32).reshape(7, 1, 1) * np.ones((7, 1, 4), np.float32)
    done = np.zeros((7, 1), bool)
    done[3] = True
    assert applied_to_live(a, done, 2)[:, 0].tolist() == [False, False, True, False, False, False, True]      # (step 3 applies a_1, but ends)
    assert never_leaves_the_ring(done, 2)[:, 0].tolist() == [False, False, True, True, False, True, True]
    assert never_leaves_the_ring(done, 0).sum() == 0


@pytest.mark.parametrize("name", sorted(GRAD_FIXTURES))
def test_gradient_fixture_is_not_vacuous(name):
    fx = load(name)
    D, T, H = GRAD_FIXTURES[name]
    c = consts_of(fx)
    done = fx["done"].astype(bool)
    g = fx["d_actions"]
    N = done.shape[1]
    assert int(c["delay_steps"]) == D and int(fx["max_episode_steps"]) == T and fx["actions"].shape == (H, N, 4) and N == 64
    assert T > D, "episodes no longer than the ring: no action would ever be applied"
    hit = applied_to_live(fx["actions"], done, D)
    step_has_grad = np.abs(g).max((1, 2)) > 0
    print(f"{name}: depth {D}; non-zero action on a live agent in {int(hit.sum())} of {hit.size} (step, agent) pairs; reference gradient "
          f"non-zero on {int(step_has_grad.sum())} of {H} steps; {int(done.sum())} episode ends")
    assert 4 * int(hit.sum()) >= hit.size
    assert 4 * int(step_has_grad.sum()) >= H
    assert done.any(0).all(), "every agent must end an episode inside the horizon"
    assert len(fx["ev_step"]) == int(done.sum())
    stuck = never_leaves_the_ring(done, D)
    assert stuck.any() and (~stuck).any()
    assert np.all(g[stuck] == 0), f"{name}: {int((g[stuck] != 0).sum())} gradient entries of actions that never left the ring are non-zero"
    # ... and the other way round, per (step, agent): an action that is applied has a gradient (the reward of the step that applies it,
    # taken on the post-step state, depends on it)
    assert (np.abs(g).max(2) > 0)[~stuck].all()
