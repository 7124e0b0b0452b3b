"""The early write-through stores of the env step's straight-line instance (k_env_step<STRAIGHT>, visfly_amd/csrc/vf_env.hip: POS, QUAT
and VEL stored write-through right behind the interval, the other five state granules plain at the end; an ending lane waits for its
early stores and stores its new episode over them) against the general kernel, which keeps every store plain and at its end, and
against the CPU oracle -- bit for bit.

Which kernel runs is decided as in tests/test_env_straight_line_gpu.py: the first env steps with step() (auto-reset, prefetched re-spawn,
no done list: the straight-line instance above 32 768 padded agents), the second asks for the compacted done list, which only the general
kernel serves.  Both step launch by launch, and the WHOLE slab (without the prefetched copies) is read back and compared after EVERY step:
a store that lands in the wrong order, too early or not at all shows in the slab one step before it can show in an observation.

N = 32 768 + 64 and 32 768 + 65: the smallest padded counts that reach k_env_step instead of the two-wave split kernel, with a full and
with a partial last tile.  max_episode_steps = 5 / 1: every agent stores its re-spawned state over its early stores every fifth step /
every step (the latter draws in place: no prefetched copy matches).  Delay-ring depths 1 and 3: the push hits the slot it has just
read at depth 1.  ctrl_dt = 0.01 (four sub-steps per interval instead of the eight of every BASELINE configuration, ring depth 6).

The project has no hook that names the kernel a launch took and the C ABI is not widened for one; that the straight-line instance ran is
what the template arguments in a kernel trace show (profiles/env_publish_early.txt, section 5)."""
import numpy as np
import pytest
import torch

from _golden import assert_bits_equal

pytestmark = pytest.mark.gpu

BIG = 32768                      # launch_env_step: up to here the two-wave split kernel
NS = (BIG + 64, BIG + 65)
STEPS = 24
COMM_DELAY = {1: 0.02, 3: 0.06}  # delay_steps = int(comm_delay / ctrl_dt) at ctrl_dt = 0.02


def _env(cls, n, integrator="euler", ctrl_delay=True, max_episode_steps=5, seed=11, ctrl_dt=0.02, **dyn):
    dkw = dict(action_type="bodyrate", integrator=integrator, dt=0.0025, ctrl_dt=ctrl_dt, ctrl_delay=ctrl_delay, **dyn)
    return cls(num_agent_per_scene=n, seed=seed, dynamics_kwargs=dkw, device="cuda:0", max_episode_steps=max_episode_steps, tensor_output=True)


def _actions(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((STEPS, n, 4), generator=g) * 2 - 1).cuda()      # the whole range: agents leave the box, collide, end


def _episode_outputs(env):
    return {k: getattr(env, k).cpu().numpy().copy() for k in ("_ep_return", "_ep_length", "_ep_flags", "_terminal_obs")}


def _cls(name):
    from visfly_amd import envs
    return getattr(envs, name)


def _run_pair(cls, n, depth=None, interval_steps=8, **kw):
    """env A: step() (the straight-line instance); env B: step() with the done list (the general kernel).  Returns the episodes ended"""
    a = _actions(n)
    A, B = _env(cls, n, **kw), _env(cls, n, **kw)
    for env in (A, B):
        if depth is not None:
            assert env.envs.dynamics._comm_delay_steps == depth
        assert int(env.envs.dynamics.constants["interval_steps"]) == interval_steps
    B.enable_done_list()
    A.reset()
    B.reset()
    assert_bits_equal(A.state_slab.cpu().numpy(), B.state_slab.cpu().numpy(), "slab after reset")
    ended = 0
    for k in range(STEPS):
        oa, ra, da, _ = A.step(a[k])
        ob, rb, db, _ = B.step(a[k])
        da = da.cpu().numpy()
        assert_bits_equal(oa["state"].cpu().numpy(), ob["state"].cpu().numpy(), f"obs @ {k}")
        assert_bits_equal(ra.cpu().numpy(), rb.cpu().numpy(), f"reward @ {k}")
        assert np.array_equal(da, db.cpu().numpy()), f"done @ {k}"
        assert_bits_equal(A.state_slab.cpu().numpy(), B.state_slab.cpu().numpy(), f"slab after step {k}")
        ended += int(da.sum())
    ea, eb = _episode_outputs(A), _episode_outputs(B)
    was_done = ea["_ep_length"] > 0                    # the episode outputs are written where an agent ended
    for key in ea:
        x, y = ea[key][was_done], eb[key][was_done]
        if x.dtype == np.float32:
            assert_bits_equal(x, y, key)
        else:
            assert np.array_equal(x, y), key
    A.close()
    B.close()
    return ended


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("ctrl_delay", [True, False], ids=["lag", "nolag"])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("kind", ["HoverEnv", "NavigationEnv"])
def test_early_stores_equal_general_kernel_every_instance(kind, integrator, ctrl_delay, depth):
    for n in NS:
        ended = _run_pair(_cls(kind), n, depth=depth, integrator=integrator, ctrl_delay=ctrl_delay, comm_delay=COMM_DELAY[depth])
        assert ended >= 4 * n                          # max_episode_steps = 5: everybody re-spawned at steps 5, 10, 15, 20


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("kind,integrator", [("HoverEnv", "euler"), ("NavigationEnv", "rk4")])
def test_every_agent_stores_over_its_early_stores_every_step(kind, integrator, depth):
    for n in NS:
        assert _run_pair(_cls(kind), n, depth=depth, integrator=integrator, max_episode_steps=1, comm_delay=COMM_DELAY[depth]) == STEPS * n


@pytest.mark.parametrize("kind,integrator", [("HoverEnv", "euler"), ("NavigationEnv", "rk4")])
def test_four_substeps_per_interval(kind, integrator):
    for n in NS:
        assert _run_pair(_cls(kind), n, depth=6, interval_steps=4, integrator=integrator, ctrl_dt=0.01) >= 4 * n


D, T = 1e-40, 2.0 ** -100          # a denormal, a tiny normal
R5 = np.sqrt(.5)
QUATS = np.array([[1, 0, 0, 0], [1, -0., T, -T], [T, 1, 0, -0.], [T, -T, 1, 0], [1, T, -T, T], [0, T, -0., 1], [.5, .5, .5, .5],
                  [R5, T, R5, -0.], [1, -0., D, -D], [D, 1, 0, -D], [R5, D, R5, T]], np.float32)
VELS = np.array([[0, 0, 0], [-0., T, -T], [T, -T, T], [T, 0, 2], [-1.5, 2.5, -0.75], [-0., D, -D], [D, 0, 2]], np.float32)
OMGS = np.array([[0, 0, 0], [T, -T, -0.], [0, 5, -0.], [2, -3, 1], [-0., 0, T], [D, -D, -0.]], np.float32)


def test_hover_bit_identical_to_oracle_from_signed_zero_and_denormal_states():
    import oracle
    n = BIG + 65
    env = _env(_cls("HoverEnv"), n, max_episode_steps=256, seed=5)
    env.reset()
    fs = env.full_state.cpu().numpy().copy()
    i = np.arange(n)
    fs[:, 3:7], fs[:, 7:10], fs[:, 10:13] = QUATS[i % len(QUATS)], VELS[i % len(VELS)], OMGS[i % len(OMGS)]
    # mid-height of the bounding box (z 0 .. 8): the inverted attitudes dive ~3.5 m in 24 steps, the upright ones climb ~2.3 m (CPU oracle)
    fs[:, 0], fs[:, 1], fs[:, 2] = (i % 7 - 3) * 0.5, (i % 5 - 2) * 0.5, 5.0 + (i % 3) * 0.25
    env.reset(state=torch.from_numpy(fs))
    ref = oracle.OracleEnv(env.envs.dynamics.constants, n, "hover", 256)
    ref.reset_full_state(fs)
    a = _actions(n, seed=23)
    a[:2, :, 1:] = 0                                   # no commanded body rate at first: the tiny components of q live a few sub-steps longer
    a[:, :, 0] = a[:, :, 0] * 0.3 - 0.5                # collective thrust at and below hover (-1/3): nobody reaches the floor or the ceiling
    for k in range(STEPS):
        o, r, d, _ = env.step(a[k])                    # auto-reset on: the straight-line instance
        ro, rr, rd = ref.step(a[k].cpu().numpy())
        assert not d.any().item() and not rd.any(), f"nobody may end an episode @ {k}: {int(d.sum())} did, {int(rd.sum())} in the oracle"
        assert_bits_equal(o["state"].cpu().numpy(), ro, f"state @ {k}")
        assert_bits_equal(r.cpu().numpy(), rr, f"reward @ {k}")
        assert_bits_equal(env.extend_state.cpu().numpy(), ref.dyn.extend_state, f"extend_state after step {k}")   # read from the slab
    env.close()
