"""The straight-line instance of the env step (k_env_step<STRAIGHT>, visfly_amd/csrc/vf_env.hip: the launch-uniform options decided on
the host, the loop's matrices from the packed constant block, the square roots outside the loop as pairs, the hover kind's collision test
without its root) against the general kernel and against the CPU oracle, bit for bit.

Which kernel runs: pick_env_kernel takes the straight-line instance for the hover / navigation kinds under the body-rate controller with
auto-reset, the prefetched re-spawn, raw rows, no drag granules, no wind rows and no done list -- and only above 32 768 padded agents:
up to there launch_env_step takes the two-wave split kernel.  So every property is checked at N = 32 768 + n, n = 1, 64, 65, 200 (partial
waves; odd n: the rows 1, 2 of a (3, N, 13) ring are not 16-byte aligned), where the new code runs, and the plain N = 1, 64, 65, 200 run
as well (the split kernel on both sides).  The general kernel is reached without any switch: the second env asks for the compacted done
list, which only the general kernel serves, and steps launch by launch (step_n does not pass the list on); the first env goes through
step_n with K = 3.

1. straight line vs general: obs, reward, done of 24 steps, the episode outputs and the whole slab (without the prefetched copies: which
   launch refilled them last is not state); max_episode_steps = 5 with actions over the whole range, so that every agent ends and re-spawns
   from its prefetched copy several times, and max_episode_steps = 1, where the first ending finds no prefetched copy and draws in place.
2. HoverEnv on the straight-line instance against the CPU oracle to the bit, start states with +-0, denormal and tiny components as in
   tests/test_pair_division_gpu.py (nobody ends an episode: the oracle does not follow device re-spawns).
3. drag_random > 0 and HoverEnv2 rows keep the general kernel and still run: step_n equals launch-by-launch stepping with the done list.
4. tools/sqrt_pair_probe.hip: sqrt_p2 against sqrtf of the same translation unit on every probe input, 0 mismatches."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from _golden import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 32768                      # launch_env_step: up to here the two-wave split kernel
STEPS, K = 24, 3


def _env(cls, n, integrator="euler", ctrl_delay=True, max_episode_steps=5, seed=11, **dyn):
    dkw = dict(action_type="bodyrate", integrator=integrator, dt=0.0025, ctrl_dt=0.02, ctrl_delay=ctrl_delay, **dyn)
    return cls(num_agent_per_scene=n, seed=seed, dynamics_kwargs=dkw, device="cuda:0", max_episode_steps=max_episode_steps, tensor_output=True)


def _actions(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((STEPS, n, 4), generator=g) * 2 - 1).cuda()


def _episode_outputs(env):
    return {k: getattr(env, k).cpu().numpy().copy() for k in ("_ep_return", "_ep_length", "_ep_flags", "_terminal_obs")}


def _run_pair(cls, n, **kw):
    """env A: step_n with K = 3 (the straight-line instance where it applies); env B: the done list, launch by launch (general kernel)"""
    a = _actions(n)
    A, B = _env(cls, n, **kw), _env(cls, n, **kw)
    B.enable_done_list()
    A.reset()
    B.reset()
    ended = 0
    for k0 in range(0, STEPS, K):
        obs, rew, done = A.step_n(a[k0:k0 + K])
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        for j in range(K):
            o, r, d, _ = B.step(a[k0 + j])
            assert_bits_equal(obs[j], o["state"].cpu().numpy(), f"obs @ {k0 + j}")
            assert_bits_equal(rew[j], r.cpu().numpy(), f"reward @ {k0 + j}")
            assert np.array_equal(done[j], d.cpu().numpy()), f"done @ {k0 + j}"
            assert sorted(B.done_indices().cpu().tolist()) == np.flatnonzero(done[j]).tolist(), f"done list @ {k0 + j}"
            ended += int(done[j].sum())
    ea, eb = _episode_outputs(A), _episode_outputs(B)
    was_done = ea["_ep_length"] > 0                    # the episode outputs are written where an agent ended
    for key in ea:
        x, y = ea[key][was_done], eb[key][was_done]
        if x.dtype == np.float32:
            assert_bits_equal(x, y, key)
        else:
            assert np.array_equal(x, y), key
    assert_bits_equal(A.state_slab.cpu().numpy(), B.state_slab.cpu().numpy(), f"slab after {STEPS} steps")
    A.close()
    B.close()
    return ended


def _cls(name):
    from visfly_amd import envs
    return getattr(envs, name)


@pytest.mark.parametrize("ctrl_delay", [True, False], ids=["lag", "nolag"])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("kind", ["HoverEnv", "NavigationEnv"])
def test_straight_line_equals_general_kernel_every_instance(kind, integrator, ctrl_delay):
    n = BIG + 65
    ended = _run_pair(_cls(kind), n, integrator=integrator, ctrl_delay=ctrl_delay)
    assert ended >= 4 * n                              # max_episode_steps = 5: everybody re-spawned at steps 5, 10, 15, 20


@pytest.mark.parametrize("n", [1, 64, 65, 200, BIG + 1, BIG + 64, BIG + 200])
@pytest.mark.parametrize("kind,integrator", [("HoverEnv", "euler"), ("NavigationEnv", "rk4")])
def test_straight_line_equals_general_kernel_partial_waves_and_unaligned_rows(kind, integrator, n):
    assert _run_pair(_cls(kind), n, integrator=integrator) >= 4 * n


@pytest.mark.parametrize("kind", ["HoverEnv", "NavigationEnv"])
def test_straight_line_in_place_draw_when_no_prefetched_copy_matches(kind):
    n = BIG + 65
    assert _run_pair(_cls(kind), n, max_episode_steps=1) == STEPS * n


def test_drag_granules_and_hover2_rows_keep_the_general_kernel():
    n = BIG + 65
    assert _run_pair(_cls("HoverEnv"), n, drag_random=0.2) >= 4 * n
    assert _run_pair(_cls("HoverEnv2"), n) >= 4 * n


D, T = 1e-40, 2.0 ** -100          # a denormal, a tiny normal
R5 = np.sqrt(.5)
QUATS = np.array([[1, 0, 0, 0], [1, -0., T, -T], [T, 1, 0, -0.], [T, -T, 1, 0], [1, T, -T, T], [0, T, -0., 1], [.5, .5, .5, .5],
                  [R5, T, R5, -0.], [1, -0., D, -D], [D, 1, 0, -D], [R5, D, R5, T]], np.float32)
VELS = np.array([[0, 0, 0], [-0., T, -T], [T, -T, T], [T, 0, 2], [-1.5, 2.5, -0.75], [-0., D, -D], [D, 0, 2]], np.float32)
OMGS = np.array([[0, 0, 0], [T, -T, -0.], [0, 5, -0.], [2, -3, 1], [-0., 0, T], [D, -D, -0.]], np.float32)


@pytest.mark.parametrize("ctrl_delay", [True, False], ids=["lag", "nolag"])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_straight_line_hover_bit_identical_to_oracle(integrator, ctrl_delay):
    import oracle
    n = BIG + 65
    env = _env(_cls("HoverEnv"), n, integrator=integrator, ctrl_delay=ctrl_delay, max_episode_steps=256, seed=5)
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
    assert_bits_equal(env.extend_state.cpu().numpy(), ref.dyn.extend_state, f"extend_state after {STEPS} steps")
    env.close()


def test_sqrt_p2_equals_sqrtf_on_every_probe_input(tmp_path):
    from visfly_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "sqrt_pair_probe")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + _build.PER_SOURCE_FLAGS["vf_env.hip"]
    subprocess.check_call([hipcc] + flags + ["-I", _build.CSRC, os.path.join(ROOT, "tools", "sqrt_pair_probe.hip"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(run.stdout)
    line = [l for l in run.stdout.splitlines() if l.startswith("mismatches ")]
    assert line, run.stdout
    k, m = int(line[0].split()[1]), int(line[0].split()[3])
    assert m >= 4 * (4 * 2041 + 2 ** 22), line[0]      # the 2 041 edge values in each of the four places, 2^22 random quadruples
    assert k == 0 and run.returncode == 0, run.stdout
