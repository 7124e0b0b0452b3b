"""Host reference of the closest-scene-point rule (include/visfly_amd.h "Analytic obstacles"; csrc/vf_env_device.hpp: scene_collision) in
numpy float32: every operation an explicit np.float32 one, in the stated order, no FMA.  np.sqrt and / are correctly rounded, as the
kernels' sqrtf and division are.  ``scene_query`` is what the device must reproduce bit for bit; ``scene_query64`` is the same geometry in
float64, the yardstick of the float32 rule's own error (tests/test_obstacles.py).
"""
import numpy as np

from visfly_amd.envs.obstacles import parse_obstacles

ROOM_LO, ROOM_HI = (-30.0, -30.0, 0.0), (30.0, 30.0, 8.0)          # droneEnv.py:129
f32 = np.float32


def _room(p, lo, hi, dt):
    """the bounding-box branch of update_collision (droneEnv.py:345-360): the closest of the six faces, the first on a tie"""
    lo, hi = np.asarray(lo, dtype=dt), np.asarray(hi, dtype=dt)
    d6 = np.concatenate([p - lo, hi - p], axis=1)
    face = np.argmin(d6, axis=1)                                      # first minimum wins
    cp = p.copy()
    rows = np.arange(len(p))
    cp[rows, face % 3] = np.where(face < 3, lo[face % 3], hi[face % 3])
    return cp


def _norm_plain(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def _sphere(p, o, dt):
    c, r = np.asarray(o["center"], dtype=dt), dt(o["radius"])
    dx = p - c
    d = _norm_plain(dx)
    g = np.maximum(d - r, dt(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = r / d                                                     # formed once
        out = c + dx * s[:, None]
    cp = np.where((d <= r)[:, None], p, out)
    return g, cp


def _box(p, o, dt):
    lo, hi = np.asarray(o["lo"], dtype=dt), np.asarray(o["hi"], dtype=dt)
    q = np.minimum(np.maximum(p, lo), hi)
    e = p - q
    return _norm_plain(e), q


def _pillar(p, o, dt):
    cx, cy, r = dt(o["center"][0]), dt(o["center"][1]), dt(o["radius"])
    zlo, zhi = dt(o["z"][0]), dt(o["z"][1])
    dx, dy = p[:, 0] - cx, p[:, 1] - cy
    dxy = np.sqrt(dx * dx + dy * dy)
    er = np.maximum(dxy - r, dt(0))
    zc = np.minimum(np.maximum(p[:, 2], zlo), zhi)
    ez = p[:, 2] - zc
    g = np.sqrt(er * er + ez * ez)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(dxy > r, r / dxy, dt(1))
    cp = np.stack([cx + dx * s, cy + dy * s, zc], axis=1)
    return g, cp


_PRIM = {"sphere": _sphere, "box": _box, "pillar": _pillar}


def candidate(p, obstacle, dt=f32):
    """(g, cp) of one obstacle for positions p (N,3)"""
    p = np.ascontiguousarray(p, dtype=dt)
    g, cp = _PRIM[obstacle["type"]](p, obstacle, dt)
    assert g.dtype == dt and cp.dtype == dt
    return g, cp


def _query(p, obstacles, lo, hi, dt):
    p = np.ascontiguousarray(p, dtype=dt).reshape(-1, 3)
    cp = _room(p, lo, hi, dt)
    best = _norm_plain(cp - p)
    win = np.zeros(len(p), dtype=np.int64)
    for k, o in enumerate(obstacles):
        g, q = candidate(p, o, dt)
        take = g < best                                               # strict: ties go to the earlier candidate
        best = np.where(take, g, best)
        cp = np.where(take[:, None], q, cp)
        win = np.where(take, k + 1, win)
    assert cp.dtype == dt and best.dtype == dt
    return cp, best, win


def scene_query(p, obstacles, lo=ROOM_LO, hi=ROOM_HI):
    """p (N,3) -> (cp (N,3) float32, g (N,) float32, winner (N,): 0 = the room box, 1 + k = obstacle k).  obstacles: the dicts of
    visfly_amd/envs/obstacles.py (validated and rounded to float32 here, as the env does)"""
    return _query(p, parse_obstacles(obstacles), lo, hi, f32)


def scene_query64(p, obstacles, lo=ROOM_LO, hi=ROOM_HI):
    """the same formulas in float64 (on the float32 table values)"""
    return _query(p, parse_obstacles(obstacles), lo, hi, np.float64)


def sample_solid(obstacle, n, rng):
    """n random points of the solid (float64)"""
    u = rng.uniform(size=(n, 3))
    if obstacle["type"] == "box":
        lo, hi = np.asarray(obstacle["lo"], dtype=np.float64), np.asarray(obstacle["hi"], dtype=np.float64)
        return lo + u * (hi - lo)
    if obstacle["type"] == "sphere":
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return np.asarray(obstacle["center"], dtype=np.float64) + v * (obstacle["radius"] * u[:, :1] ** (1 / 3))
    ang, rad = 2 * np.pi * u[:, 0], obstacle["radius"] * np.sqrt(u[:, 1])
    z = obstacle["z"][0] + u[:, 2] * (obstacle["z"][1] - obstacle["z"][0])
    return np.stack([obstacle["center"][0] + rad * np.cos(ang), obstacle["center"][1] + rad * np.sin(ang), z], axis=1)


def inside(obstacle, x, tol):
    """is x (n,3), float64, in the solid grown by tol?"""
    x = np.asarray(x, dtype=np.float64)
    if obstacle["type"] == "box":
        return np.all((x >= np.asarray(obstacle["lo"]) - tol) & (x <= np.asarray(obstacle["hi"]) + tol), axis=1)
    if obstacle["type"] == "sphere":
        return np.linalg.norm(x - np.asarray(obstacle["center"]), axis=1) <= obstacle["radius"] + tol
    rad = np.hypot(x[:, 0] - obstacle["center"][0], x[:, 1] - obstacle["center"][1])
    return (rad <= obstacle["radius"] + tol) & (x[:, 2] >= obstacle["z"][0] - tol) & (x[:, 2] <= obstacle["z"][1] + tol)
