"""The sub-step loop on register pairs (visfly_amd/csrc/vf_pair_algebra.hpp: packed Hamilton products, row-paired B / J / Jinv) against the
CPU oracle, bit for bit, where the rewrite could differ from the scalar form if it were not exact: -0.0 and exact 0 in q, v and w (the
pure-vector operands keep their zero; (-a) b for -(a b) and x + (-y) for x - y must give the same signed zeros), agents tilted past 90
degrees, and actions over the whole range.  N = 65: one full wave plus one lane."""
import numpy as np
import pytest
import torch

from _golden import assert_bits_equal

pytestmark = pytest.mark.gpu

N, STEPS = 65, 24
S3 = 0.8660254037844386
# unit quaternions (w, x, y, z) with exact and negative zeros; tilts of 0, 90, 120, 150 and 180 degrees
QUATS = np.array([[1, 0, 0, 0], [1, -0., -0., -0.], [0, 1, 0, 0], [-0., 0, 1, 0], [0, 0, -0., 1], [.5, S3, 0, 0], [.5, .5, .5, .5],
                  [.5, -.5, .5, -.5], [np.sqrt(.5), 0, np.sqrt(.5), -0.], [0.25881904510252074, -0., 0.9659258262890683, 0],
                  [-.5, S3, -0., 0]], np.float32)
VELS = np.array([[0, 0, 0], [-0., -0., -0.], [0, -0., 2], [3, 0, -0.], [-1.5, 2.5, -0.75]], np.float32)
OMGS = np.array([[0, 0, 0], [-0., -0., -0.], [0, 5, -0.], [-6, 0, 0], [-0., 0, 4], [2, -3, 1], [0, -0., 0]], np.float32)


def _spawn_states(env):
    """the env's own spawn (rotor speeds, thrusts, positions) with q, v, w replaced by the patterns above (coprime cycle lengths)"""
    env.reset()
    fs = env.full_state.cpu().numpy().copy()
    i = np.arange(N)
    fs[:, 3:7], fs[:, 7:10], fs[:, 10:13] = QUATS[i % len(QUATS)], VELS[i % len(VELS)], OMGS[i % len(OMGS)]
    env.reset(state=torch.from_numpy(fs))
    got = env.full_state.cpu().numpy()
    # the reset takes the rows as they are; full_state reports v + wind, so a -0.0 velocity reads back as +0.0: q and w to the bit, v by value
    assert_bits_equal(got[:, 3:7], fs[:, 3:7], "reset(state=...) keeps q to the bit (signed zeros included)")
    assert_bits_equal(got[:, 10:13], fs[:, 10:13], "reset(state=...) keeps w to the bit (signed zeros included)")
    assert np.array_equal(got[:, 7:10], fs[:, 7:10])
    assert np.signbit(got[1, 4:7]).all() and np.signbit(got[1, 10:13]).all() and not np.signbit(got[0, 3:13]).any()
    return fs


@pytest.mark.parametrize("ctrl_delay", [True, False], ids=["delay", "nodelay"])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("action_type", ["bodyrate", "thrust"])
def test_hover_signed_zeros_tilts_wide_actions_bit_identical_to_oracle(action_type, integrator, ctrl_delay):
    import oracle
    from visfly_amd.envs import HoverEnv
    dkw = dict(action_type=action_type, integrator=integrator, dt=0.0025, ctrl_dt=0.02, ctrl_delay=ctrl_delay)
    env = HoverEnv(num_agent_per_scene=N, seed=5, dynamics_kwargs=dkw, device="cuda:0", max_episode_steps=256, tensor_output=True)
    fs = _spawn_states(env)
    ref = oracle.OracleEnv(env.envs.dynamics.constants, N, "hover", 256)
    ref.reset_full_state(fs)
    g = torch.Generator().manual_seed(17)
    for k in range(STEPS):
        a = torch.rand((N, 4), generator=g) * 2 - 1
        if k % 6 == 0:
            a[::3] = a[::3].sign()                  # the corners of the action box
        o, r, d, _ = env.step(a.cuda(), is_test=True)
        ro, rr, rd = ref.step(a.numpy())
        assert_bits_equal(o["state"].cpu().numpy(), ro, f"state @ {k}")
        assert_bits_equal(r.cpu().numpy(), rr, f"reward @ {k}")
        assert np.array_equal(d.cpu().numpy().astype(np.uint8), rd), f"done @ {k}"
    assert_bits_equal(env.extend_state.cpu().numpy(), ref.dyn.extend_state, f"extend_state after {STEPS} steps")
    env.close()


def test_navigation_rk4_drag_random_bit_identical_to_oracle_until_first_episode_end():
    import oracle
    from visfly_amd.envs import NavigationEnv
    T = 16
    dkw = dict(action_type="bodyrate", integrator="rk4", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True, drag_random=0.1)
    spawn = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}}]}}
    env = NavigationEnv(num_agent_per_scene=N, seed=7, dynamics_kwargs=dkw, random_kwargs=spawn, device="cuda:0", max_episode_steps=T,
                        tensor_output=True)
    fs = _spawn_states(env)
    dyn = env.envs.dynamics
    kl, kq = dyn.drag_coefficients
    ref = oracle.OracleEnv(dyn.constants, N, "nav", T, target=[9., 0., 1.])
    ref.dyn.klin = np.ascontiguousarray(kl.cpu().numpy().T)
    ref.dyn.kquad = np.ascontiguousarray(kq.cpu().numpy().T)
    ref.reset_full_state(fs)
    g = torch.Generator().manual_seed(19)
    alive, compared = np.ones(N, bool), 0
    for k in range(STEPS):
        a = torch.rand((N, 4), generator=g) * 2 - 1
        o, r, d, _ = env.step(a.cuda())
        ro, rr, rd = ref.step(a.numpy())
        assert np.array_equal(d.cpu().numpy().astype(np.uint8)[alive], rd[alive]), f"done @ {k}"
        assert_bits_equal(r.cpu().numpy()[alive], rr[alive], f"reward @ {k}")
        alive &= ~(rd > 0)                            # an ended agent is re-spawned by the device: compared up to its first episode end
        assert_bits_equal(o["state"].cpu().numpy()[alive], ro[alive], f"state @ {k}")
        compared += int(alive.sum())
    assert not alive.any() and compared >= N * 4, (int(alive.sum()), compared)
    env.close()
