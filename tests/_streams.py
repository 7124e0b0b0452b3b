"""helpers shared by tests/test_device_streams.py (CPU) and tests/test_device_streams_gpu.py: the spawn boxes both use, and definitions of
the device random streams that are INDEPENDENT of oracle/vf_oracle.c -- Philox4x32-10 in numpy uint64 arithmetic, the spawn / drag / noise
values in fp64 from the Philox words"""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _box(pos, ori_mean, vel, omg):
    return {"class": "Uniform", "kwargs": {"position": {"mean": pos[0], "half": pos[1]},
                                           "orientation": {"mean": ori_mean, "half": [math.pi, 1.0, 3.0]},
                                           "velocity": {"mean": vel[0], "half": vel[1]},
                                           "angular_velocity": {"mean": omg[0], "half": omg[1]}}}


# three boxes whose x ranges do not overlap ([-2.75, -1.25], [0.5, 1.5], [3, 5]): the position names the box that was picked
UNION = {"state_generator": {"class": "Union", "kwargs": [{"randomizers_kwargs": [
    _box(([-2., 0.5, 1.5], [0.75, 1., 0.5]), [0.1, -0.2, 0.3], ([1., 0., 0.], [1., 0.5, 0.5]), ([0., 0., 0.], [0.3, 0.2, 0.1])),
    _box(([1., -1., 2.], [0.5, 2., 1.]), [0., 0., 0.], ([0., 0.5, -0.25], [0.25, 1., 0.125]), ([0.1, -0.1, 0.2], [1., 1., 2.])),
    _box(([4., 0., 3.], [1., 0.25, 1.5]), [-0.5, 0.25, 1.], ([-1., -1., 0.5], [2., 0.1, 0.7]), ([0., 0.3, 0.], [0.05, 0.6, 0.9])),
]}]}}


def box_with(ori_half, ori_mean=(0., 0., 0.)):
    """one Uniform box with the given orientation range (everything else like box 0 of UNION)"""
    kw = dict(UNION["state_generator"]["kwargs"][0]["randomizers_kwargs"][0]["kwargs"])
    kw["orientation"] = {"mean": list(ori_mean), "half": list(ori_half)}
    return {"state_generator": {"class": "Uniform", "kwargs": [kw]}}


def philox_np(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy uint64 arithmetic:
    ctr (n,4), key (n,2) | (2,) -> (n,4) uint64 words < 2^32"""
    c = np.asarray(ctr, np.uint64).reshape(-1, 4)
    k = np.broadcast_to(np.asarray(key, np.uint64), (len(c), 2))
    x, y, z, w = (c[:, i].copy() for i in range(4))
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x, np.uint64(0xCD9E8D57) * z
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([x, y, z, w], 1)


def seed_key(seed):
    s = int(seed) & (2 ** 64 - 1)
    return [s & 0xFFFFFFFF, s >> 32]


def spawn_words(seed, ids, episode, blocks):
    """the words of the blocks {id, episode, block, 0x5eed} under key `seed`, concatenated: (n, 4 len(blocks)) uint64"""
    ids = np.asarray(ids, np.uint64) & M32
    ep = np.broadcast_to(np.asarray(episode, np.uint64), ids.shape)
    out = []
    for b in blocks:
        ctr = np.stack([ids, ep, np.full_like(ids, b), np.full_like(ids, 0x5eed)], 1)
        out.append(philox_np(ctr, seed_key(seed)))
    return np.concatenate(out, 1)


def spawn_fp64(seed, ids, episode, boxes):
    """-> dict: u (n,12) fp64 uniforms, pick (n,) box index, tbits (n,), pos / eul / vel / omg (n,3) fp64 = mean + (2u - 1) half of the
    picked box (means and halves rounded to fp32 first, as the env stores them)"""
    r = spawn_words(seed, ids, episode, (0, 1, 2))
    u = (r & np.uint64(0xFFFFFF)).astype(np.float64) / 2.0 ** 24
    top = r >> np.uint64(24)
    pick = top[:, 0] | (top[:, 1] << np.uint64(8)) | (top[:, 2] << np.uint64(16)) | (top[:, 3] << np.uint64(24))
    tbits = top[:, 4] | (top[:, 5] << np.uint64(8)) | (top[:, 6] << np.uint64(16))
    b = (pick % np.uint64(len(boxes))).astype(np.int64) if len(boxes) > 1 else np.zeros(len(r), np.int64)
    out = {"u": u, "pick": b, "tbits": tbits}
    for j, (name, f) in enumerate((("pos", "position"), ("eul", "orientation"), ("vel", "velocity"), ("omg", "angular_velocity"))):
        mean = np.array([bx[f]["mean"] for bx in boxes], np.float32).astype(np.float64)[b]
        half = np.array([bx[f]["half"] for bx in boxes], np.float32).astype(np.float64)[b]
        out[name] = mean + (2.0 * u[:, 3 * j:3 * j + 3] - 1.0) * half
        out[name + "_mean"], out[name + "_half"] = mean, half
    return out


def quat_zyx_fp64(eul):
    """Quaternion.from_euler(roll, pitch, yaw), zyx, in fp64: (n,3) -> (n,4) wxyz"""
    e = np.asarray(eul, np.float64) * 0.5
    (sr, sp, sy), (cr, cp, cy) = np.sin(e).T, np.cos(e).T
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)


def noise_uniforms_fp64(row, step, tag, seed):
    """Box-Muller input of the block {row, step lo, step hi, tag}: u1, u3 = ((w >> 8) + 1) 2^-24, u2, u4 = (w >> 8) 2^-24 (all exact in fp32)"""
    row = np.asarray(row, np.uint64).reshape(-1)
    step = np.broadcast_to(np.asarray(step, np.uint64), row.shape)
    ctr = np.stack([row & M32, step & M32, step >> np.uint64(32), np.full_like(row, tag)], 1)
    w = (philox_np(ctr, seed_key(seed)) >> np.uint64(8)).astype(np.float64)
    w[:, 0] += 1.0
    w[:, 2] += 1.0
    return w / 2.0 ** 24


def normals_fp64(u32):
    """fp64 Box-Muller on fp32 uniforms (n,4), the angle rounded the way the device forms it (one fp32 multiply by fp32(2 pi)):
    -> reference (n,4) = [ra cos a2, ra sin a2, rb cos a4, rb sin a4], radius (n,4) = [ra, ra, rb, rb]"""
    u = np.asarray(u32, np.float32)
    two_pi = np.float32(6.2831855)
    a2, a4 = (two_pi * u[:, 1]).astype(np.float64), (two_pi * u[:, 3]).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0].astype(np.float64))), np.sqrt(-2.0 * np.log(u[:, 2].astype(np.float64)))
    return (np.stack([ra * np.cos(a2), ra * np.sin(a2), rb * np.cos(a4), rb * np.sin(a4)], 1), np.stack([ra, ra, rb, rb], 1))
