"""The host restatement of the device random streams (oracle/vf_oracle.c: vfo_philox4x32_10, vfo_spawn, vfo_spawn_drag,
vfo_noise_uniforms) against definitions that do not share its text: Random123's published known answers, Philox in numpy uint64
arithmetic, and the fp64 value of every formula computed from the Philox words in this file (tests/_streams.py).  No GPU;
tests/test_device_streams_gpu.py then holds the device to the restatement bit for bit."""
import numpy as np
import pytest

import oracle
from _streams import UNION, box_with, noise_uniforms_fp64, philox_np, quat_zyx_fp64, spawn_fp64, spawn_words
from visfly_amd.envs.randomization import spawn_boxes

# Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]
SEEDS = [3, 2 ** 40 + 7, -1]
N = 4096


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    assert oracle.philox4x32_10([ctr], key)[0].tolist() == out
    assert philox_np([ctr], key)[0].tolist() == out


def test_philox_c_equals_numpy_uint64_restatement():
    g = np.random.default_rng(0)
    ctr = g.integers(0, 2 ** 32, (2 ** 16, 4), dtype=np.uint64)
    key = g.integers(0, 2 ** 32, (2 ** 16, 2), dtype=np.uint64)
    got = oracle.philox4x32_10(ctr.astype(np.uint32), key.astype(np.uint32))
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.uint64), philox_np(ctr, key))
    assert np.array_equal(oracle.philox4x32_10(ctr.astype(np.uint32), key[0].astype(np.uint32)).astype(np.uint64), philox_np(ctr, key[0]))


@pytest.mark.parametrize("agent0", [None, 2 ** 32 - N])
@pytest.mark.parametrize("seed", SEEDS)
def test_spawn_box_values_against_fp64(seed, agent0):
    """position, velocity and angular velocity = mean + (2u - 1) half of the picked box, u from the Philox words in this file: within 2 ulp
    of |mean| + |half| per component (one rounding of the product, one of the sum: <= 1 ulp of that scale) and inside the closed box"""
    boxes = spawn_boxes(UNION)
    agent = np.arange(N)
    episode = 1 + (agent % 5)
    state, t = oracle.spawn(seed, agent, episode, boxes, indexed=False, agent0=agent0)
    ref = spawn_fp64(seed, agent + (agent0 or 0), episode, boxes)
    for name, col in (("pos", 0), ("vel", 7), ("omg", 10)):
        got = state[:, col:col + 3].astype(np.float64)
        mean, half = ref[name + "_mean"], ref[name + "_half"]
        err = np.abs(got - ref[name])
        assert (err <= 2 * _ulp(np.abs(mean) + np.abs(half))).all(), (name, err.max())
        lo, hi = (mean - half).astype(np.float32), (mean + half).astype(np.float32)
        assert ((state[:, col:col + 3] >= lo) & (state[:, col:col + 3] <= hi)).all(), name
    assert not t.any()


def test_spawn_is_keyed_by_agent_episode_and_seed_words():
    """every key word moves the draw: the low and the high seed word, the agent id (agent0 + row, modulo nothing below 2^32), the episode"""
    boxes = spawn_boxes(UNION)
    agent = np.arange(64)
    base = oracle.spawn(2 ** 40 + 7, agent, 1, boxes, True)[0]
    for other in (oracle.spawn(2 ** 40 + 8, agent, 1, boxes, True)[0], oracle.spawn(2 ** 41 + 7, agent, 1, boxes, True)[0],
                  oracle.spawn(2 ** 40 + 7, agent, 2, boxes, True)[0], oracle.spawn(2 ** 40 + 7, agent, 1, boxes, True, agent0=64)[0]):
        assert (other[:, 0] != base[:, 0]).mean() > 0.9
    assert np.array_equal(oracle.spawn(2 ** 40 + 7, agent[:32], 1, boxes, True, agent0=32)[0], base[32:])
    assert np.array_equal(oracle.spawn(-1, agent, 1, boxes, True)[0], oracle.spawn(2 ** 64 - 1, agent, 1, boxes, True)[0])


@pytest.mark.parametrize("seed", SEEDS)
def test_spawn_quaternion_against_fp64_zyx(seed):
    """Euler angles uniform in [-pi, pi]^3 (ori_half = [pi, pi, pi]), formed in fp32 exactly as the spawner forms them; the quaternion
    against the fp64 zyx formula on those angles: max abs error <= 4e-7, | |q| - 1 | <= 4e-7 (measured on the CPU: 2.1e-7 and 2.1e-7 here, 2.1e-7 and
    2.3e-7 over 2^22 samples; any swapped axis or sign is an O(1) error)"""
    pi = float(np.float32(np.pi))
    boxes = spawn_boxes(box_with([np.pi] * 3))
    agent = np.arange(2 ** 16)
    state, _ = oracle.spawn(seed, agent, 3, boxes, indexed=True)
    ref = spawn_fp64(seed, agent, 3, boxes)
    u = ref["u"][:, 3:6].astype(np.float32)
    eul = (np.float32(2) * u - np.float32(1)) * np.float32(pi) + np.float32(0)
    assert eul.dtype == np.float32 and eul.min() < -3.1 and eul.max() > 3.1
    q = state[:, 3:7].astype(np.float64)
    err = np.abs(q - quat_zyx_fp64(eul)).max()
    nerr = np.abs(np.linalg.norm(q, axis=1) - 1.0).max()
    print(f"seed {seed}: max|q - fp64| = {err:.3e}, max||q| - 1| = {nerr:.3e}")
    assert err <= 4e-7 and nerr <= 4e-7, (err, nerr)


def test_spawn_quaternion_uses_the_boxes_mean_and_order():
    """the UNION boxes (orientation half [pi, 1, 3], non-zero means, three different ranges per axis: a swapped roll / yaw cannot hide)"""
    boxes = spawn_boxes(UNION)
    agent = np.arange(N)
    state, _ = oracle.spawn(5, agent, 1, boxes, indexed=False)
    ref = spawn_fp64(5, agent, 1, boxes)
    u = ref["u"][:, 3:6].astype(np.float32)
    eul = (np.float32(2) * u - np.float32(1)) * ref["eul_half"].astype(np.float32) + ref["eul_mean"].astype(np.float32)
    assert np.abs(state[:, 3:7] - quat_zyx_fp64(eul)).max() <= 4e-7


def test_sincos_spawn_against_fp64():
    """the spawner's sin / cos pair for |x| <= 500 (a half-angle is far below that): within 2 ulp of [0.5, 1) = 2 * 2^-24 = 1.2e-7 of fp64
    (measured 9.3e-8: ~1 ulp of the polynomial plus the rounding of the reduced argument)"""
    g = np.random.default_rng(1)
    x = np.concatenate([g.uniform(-r, r, 2 ** 18) for r in (0.8, 4.0, 50.0, 500.0)] + [np.arange(-8, 9) * np.pi / 4]).astype(np.float32)
    sn, cs = oracle.sincos_spawn(x)
    es, ec = np.abs(sn - np.sin(x.astype(np.float64))).max(), np.abs(cs - np.cos(x.astype(np.float64))).max()
    print(f"sincos_spawn: max|sin - fp64| = {es:.3e}, max|cos - fp64| = {ec:.3e}")
    assert es <= 2 * 2.0 ** -24 and ec <= 2 * 2.0 ** -24


def _inside(pos, boxes):
    """(n, len(boxes)) bool: the position lies in the closed position range of box j"""
    lo = np.array([np.subtract(b["position"]["mean"], b["position"]["half"]) for b in boxes]).astype(np.float32)
    hi = np.array([np.add(b["position"]["mean"], b["position"]["half"]) for b in boxes]).astype(np.float32)
    return ((pos[:, None, :] >= lo[None]) & (pos[:, None, :] <= hi[None])).all(2)


def test_spawn_box_pick():
    """boxes whose position ranges do not overlap: every row lies in the box that pick % n names and in no other (pick assembled here from
    the top bytes of block 0), and every box occurs.  n = 3 (256 = 1 mod 3: every one of the four bytes counts), n = 4 (RacingEnv's union:
    the low bits of byte 0) and n = 2"""
    from visfly_amd.envs.tasks import _RACING_SPAWN
    agent = np.arange(N)
    three, four = spawn_boxes(UNION), spawn_boxes(_RACING_SPAWN)
    for boxes in (three, four, three[:2]):
        for seed in SEEDS:
            state, _ = oracle.spawn(seed, agent, 2, boxes, indexed=True)
            pick = spawn_fp64(seed, agent, 2, boxes)["pick"]
            inside = _inside(state[:, 0:3], boxes)
            assert (inside.sum(1) == 1).all() and np.array_equal(inside.argmax(1), pick)
            assert set(pick.tolist()) == set(range(len(boxes)))
    one = oracle.spawn(3, agent, 2, three[1:2], indexed=True)[0]       # a single box is never picked from
    assert _inside(one[:, 0:3], three)[:, 1].all()


def test_spawn_t():
    """indexed: t = (u01(tbits) * 3.14f) * 2.0f in fp32, in [0, 6.28]; full reset: exactly 0.  (The doubling is exact, so u * (3.14f * 2.0f) and
    u * 6.28f are the same bits: the operand order cannot change a value here, the constant and the rounding to fp32 can)"""
    boxes = spawn_boxes(UNION)
    agent = np.arange(2 ** 16)
    for seed in SEEDS:
        _, t = oracle.spawn(seed, agent, 7, boxes, indexed=True)
        tb = spawn_fp64(seed, agent, 7, boxes)["tbits"]
        assert tb.max() < 2 ** 24 and tb.max() > 0.99 * 2 ** 24
        u = (tb.astype(np.float64) / 2.0 ** 24).astype(np.float32)
        want = (u * np.float32(3.14)) * np.float32(2.0)
        assert want.dtype == np.float32 and np.array_equal(t.view(np.uint32), want.view(np.uint32))
        assert t.min() >= 0 and t.max() <= np.float32(6.28) and t.max() > 6.2
        assert np.abs(t.astype(np.float64) - tb.astype(np.float64) / 2.0 ** 24 * 6.28).max() <= 2 * 2.0 ** -22      # 2 ulp of [4, 8)
        _, t0 = oracle.spawn(seed, agent, 7, boxes, indexed=False)
        assert np.array_equal(t0.view(np.uint32), np.zeros(len(agent), np.uint32))


@pytest.mark.parametrize("r", [0.1, 0.6])
def test_spawn_drag_against_fp64(r):
    """k = k_mean (clamp((u - .5) 2r, -.5, .5) + 1) with u from blocks 4 and 5: within 2 ulp of the fp64 value; r = 0.6 clamps on both sides"""
    k_lin, k_quad = np.array([0.3, 0.35, 0.4], np.float32), np.array([0.02, 0.025, 0.05], np.float32)
    agent = np.arange(N)
    for seed in SEEDS:
        kl, kq = oracle.spawn_drag(seed, agent, 4, r, k_lin, k_quad, agent0=7)
        w = spawn_words(seed, agent + 7, 4, (4, 5))
        u = (w & np.uint64(0xFFFFFF)).astype(np.float64) / 2.0 ** 24
        r32 = float(np.float32(r))
        for got, mean, uu in ((kl, k_lin, u[:, 0:3]), (kq, k_quad, u[:, 4:7])):
            f = np.clip((uu - 0.5) * 2 * r32, -0.5, 0.5) + 1.0
            ref = mean.astype(np.float64) * f
            assert (np.abs(got - ref) <= 2 * _ulp(ref)).all(), np.abs(got - ref).max()
            if r > 0.5:
                assert (f == 0.5).any() and (f == 1.5).any() and ((f > 0.5) & (f < 1.5)).any()
                assert np.array_equal(got[f == 0.5], (mean * np.float32(0.5) + np.zeros_like(got))[f == 0.5])
                assert np.array_equal(got[f == 1.5], (mean * np.float32(1.5) + np.zeros_like(got))[f == 1.5])
            else:
                assert f.min() >= 1 - r32 and f.max() <= 1 + r32 and f.min() < 0.91 and f.max() > 1.09


def test_noise_uniforms():
    """the Box-Muller input: every value is exact in fp32, so the restatement equals the fp64 definition; u1, u3 in (0, 1], u2, u4 in [0, 1);
    the step crosses the 32-bit word; the two tags and the two seed words key different blocks"""
    seed = 2 ** 33 + 5
    rows = np.arange(12345, 12345 + 2 ** 16)
    for tag in (oracle.TAG_PPO_NOISE, oracle.TAG_ROW_NOISE):
        for step in (2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1):
            u = oracle.noise_uniforms(rows, step, tag, seed)
            assert u.dtype == np.float32 and np.array_equal(u.astype(np.float64), noise_uniforms_fp64(rows, step, tag, seed))
            assert u[:, [0, 2]].min() > 0 and u[:, [0, 2]].max() <= 1 and u[:, [1, 3]].min() >= 0 and u[:, [1, 3]].max() < 1
    a = oracle.noise_uniforms(rows, 2 ** 32, oracle.TAG_ROW_NOISE, seed)
    for b in (oracle.noise_uniforms(rows, 0, oracle.TAG_ROW_NOISE, seed), oracle.noise_uniforms(rows, 2 ** 32, oracle.TAG_PPO_NOISE, seed),
              oracle.noise_uniforms(rows, 2 ** 32, oracle.TAG_ROW_NOISE, 5), oracle.noise_uniforms(rows, 2 ** 32, oracle.TAG_ROW_NOISE, 2 ** 33 + 4)):
        assert (a[:, 0] != b[:, 0]).mean() > 0.99
    assert (oracle.TAG_PPO_NOISE, oracle.TAG_ROW_NOISE) == (0xac7, 0xb977)
    # the block whose first word is 0xffffff..: u1 = 1, the radius of its pair is 0 (tests/test_device_streams_gpu.py runs it on the device)
    assert oracle.noise_uniforms([165461], 0, oracle.TAG_ROW_NOISE, seed)[0, 0] == 1.0
