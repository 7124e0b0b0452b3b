"""div_p (visfly_amd/csrc/vf_pair_algebra.hpp): the IEEE division whose six plain operations run on a register pair.
1. tools/div_pair_probe.hip, a stand-alone program: div_p against `/` of the same translation unit, bit for bit, over every ordered pair of
   a set of specials / denormal extremes / all exponents x four mantissas (the two halves from different elements, so that one half takes a
   scaling path while the other does not) plus 2^22 random bit patterns; both forms of div_p and the interleaved div_p2 / div_p1 that the
   sub-step loop uses.  No mismatch is allowed.
2. HoverEnv against the CPU oracle to the bit from start states that put exact +-0, denormals (1e-40) and tiny normals (2^-100) into the
   numerators of the sub-step loop's divisions: components of q (q / |q|), and v, w of the same kinds so that the rotated force has zero
   and denormal components (ra / m).  N = 65: one full wave plus one lane."""
import os
import subprocess

import numpy as np
import pytest
import torch

from _golden import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_div_p_equals_the_division_operator_on_every_probe_input(tmp_path):
    import shutil
    from visfly_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "div_pair_probe")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + _build.PER_SOURCE_FLAGS["vf_env.hip"]
    subprocess.check_call([hipcc] + flags + ["-I", _build.CSRC, os.path.join(ROOT, "tools", "div_pair_probe.hip"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(run.stdout)
    line = [l for l in run.stdout.splitlines() if l.startswith("mismatches ")]
    assert line, run.stdout
    k, m = int(line[0].split()[1]), int(line[0].split()[3])
    # every ordered pair of the set and the random patterns; per input 2 + 2 quotients of div_p's two forms, 4 of div_p2, 3 of div_p1
    assert m >= 11 * (2041 ** 2 + 2 ** 22), line[0]
    assert k == 0 and run.returncode == 0, run.stdout


N, STEPS = 65, 24
D, T = 1e-40, 2.0 ** -100          # a denormal, a tiny normal
R5 = np.sqrt(.5)
QUATS = np.array([[1, 0, 0, 0], [1, -0., T, -T], [T, 1, 0, -0.], [T, -T, 1, 0], [1, T, -T, T], [0, T, -0., 1], [.5, .5, .5, .5],
                  [R5, T, R5, -0.], [1, -0., D, -D], [D, 1, 0, -D], [R5, D, R5, T]], np.float32)
VELS = np.array([[0, 0, 0], [-0., T, -T], [T, -T, T], [T, 0, 2], [-1.5, 2.5, -0.75], [-0., D, -D], [D, 0, 2]], np.float32)
OMGS = np.array([[0, 0, 0], [T, -T, -0.], [0, 5, -0.], [2, -3, 1], [-0., 0, T], [D, -D, -0.]], np.float32)
# (the commit before div_p reproduces the oracle from every one of these rows, the denormal ones included: profiles/env_pair_division.txt)


def _spawn_states(env):
    """the env's own spawn (rotor speeds, thrusts, positions) with q, v, w replaced by the patterns above (cycle lengths 11, 7, 6)"""
    env.reset()
    fs = env.full_state.cpu().numpy().copy()
    i = np.arange(N)
    fs[:, 3:7], fs[:, 7:10], fs[:, 10:13] = QUATS[i % len(QUATS)], VELS[i % len(VELS)], OMGS[i % len(OMGS)]
    assert (np.abs(fs[8, 3:7]) == np.float32(D)).sum() == 2 and fs[8, 5] != 0, "the denormals survive the host arrays"
    env.reset(state=torch.from_numpy(fs))
    got = env.full_state.cpu().numpy()
    assert_bits_equal(got[:, 3:7], fs[:, 3:7], "reset(state=...) keeps q to the bit (zeros, denormals and tiny normals included)")
    assert_bits_equal(got[:, 10:13], fs[:, 10:13], "reset(state=...) keeps w to the bit")
    assert np.array_equal(got[:, 7:10], fs[:, 7:10])          # full_state reports v + wind: by value
    return fs


def _assert_rows_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    rows = np.flatnonzero((bits(a) != bits(b)).reshape(len(a), -1).any(1))
    if len(rows):
        pat = [(int(i), int(i % len(QUATS)), int(i % len(VELS)), int(i % len(OMGS))) for i in rows[:8]]
        assert_bits_equal(a, b, f"{what}; agents (index, q row, v row, w row) {pat}")


@pytest.mark.parametrize("ctrl_delay", [True, False], ids=["delay", "nodelay"])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_hover_zero_denormal_and_tiny_numerators_bit_identical_to_oracle(integrator, ctrl_delay):
    import oracle
    from visfly_amd.envs import HoverEnv
    dkw = dict(action_type="bodyrate", integrator=integrator, dt=0.0025, ctrl_dt=0.02, ctrl_delay=ctrl_delay)
    env = HoverEnv(num_agent_per_scene=N, seed=5, dynamics_kwargs=dkw, device="cuda:0", max_episode_steps=256, tensor_output=True)
    fs = _spawn_states(env)
    ref = oracle.OracleEnv(env.envs.dynamics.constants, N, "hover", 256)
    ref.reset_full_state(fs)
    g = torch.Generator().manual_seed(23)
    for k in range(STEPS):
        a = torch.rand((N, 4), generator=g) * 2 - 1
        if k < 2:
            a[:, 1:] = 0                                # no commanded body rate at first: the tiny components of q live a few sub-steps longer
        o, r, d, _ = env.step(a.cuda(), is_test=True)
        ro, rr, rd = ref.step(a.numpy())
        _assert_rows_equal(o["state"].cpu().numpy(), ro, f"state @ {k}")
        _assert_rows_equal(r.cpu().numpy(), rr, f"reward @ {k}")
        assert np.array_equal(d.cpu().numpy().astype(np.uint8), rd), f"done @ {k}"
    _assert_rows_equal(env.extend_state.cpu().numpy(), ref.dyn.extend_state, f"extend_state after {STEPS} steps")
    env.close()
