"""Analytic obstacles, host side (no GPU): the float32 closest-point rule of tests/_obstacle_ref.py against the same formulas in float64
and against the geometry itself, the tie order, the validation of scene_kwargs["obstacles"] / env.obstacles, and the C-ABI surface."""
import ctypes

import numpy as np
import pytest

import _obstacle_ref as R
from visfly_amd import _lib
from visfly_amd.envs.obstacles import obstacle_rows, obstacle_table, parse_obstacles

ROOM = 60.0                    # the room's largest extent: agreement is asked to 1e-6 of it
SPHERE = dict(type="sphere", center=[1.0, -0.5, 1.5], radius=0.6)
BOX = dict(type="box", lo=[-2.0, 0.5, 0.0], hi=[-1.0, 2.5, 3.0])
PILLAR = dict(type="pillar", center=[3.0, 1.0], radius=0.4, z=[0.0, 2.5])
PRIMS = {"sphere": SPHERE, "box": BOX, "pillar": PILLAR}


def _points(o, n, rng):
    """n float32 points around obstacle o: far, near, inside, on the surface, and -- for a pillar -- on its axis"""
    o = parse_obstacles([o])[0]
    k = n // 5
    far = rng.uniform([-30, -30, 0], [30, 30, 8], size=(k, 3))
    inner = R.sample_solid(o, k, rng)
    if o["type"] == "box":
        c, h = (np.asarray(o["lo"]) + o["hi"]) / 2, (np.asarray(o["hi"]) - o["lo"]) / 2
        near = c + rng.uniform(-2, 2, size=(k, 3)) * h
        surf = inner.copy()
        ax, side = rng.integers(0, 3, k), rng.integers(0, 2, k)
        surf[np.arange(k), ax] = np.where(side == 0, np.asarray(o["lo"])[ax], np.asarray(o["hi"])[ax])
        special = np.asarray([o["lo"], o["hi"], c]).repeat(k // 3 + 1, axis=0)[:k]
    elif o["type"] == "sphere":
        c = np.asarray(o["center"])
        near = c + rng.uniform(-2, 2, size=(k, 3)) * o["radius"]
        v = rng.normal(size=(k, 3))
        surf = c + v / np.linalg.norm(v, axis=1, keepdims=True) * o["radius"]
        special = np.tile(c, (k, 1))                                     # the centre itself: d == 0
        special[1::2, 0] += o["radius"]                                  # and exactly one radius away along x
    else:
        c = np.asarray([o["center"][0], o["center"][1], (o["z"][0] + o["z"][1]) / 2])
        near = c + rng.uniform(-2, 2, size=(k, 3)) * [o["radius"], o["radius"], (o["z"][1] - o["z"][0]) / 2]
        ang = rng.uniform(0, 2 * np.pi, k)
        surf = np.stack([c[0] + o["radius"] * np.cos(ang), c[1] + o["radius"] * np.sin(ang), rng.uniform(o["z"][0], o["z"][1], k)], axis=1)
        special = np.stack([np.full(k, c[0]), np.full(k, c[1]), rng.uniform(o["z"][0] - 2, o["z"][1] + 2, k)], axis=1)   # the axis: dxy == 0
    p = np.concatenate([far, near, inner, surf, special, rng.uniform([-30, -30, 0], [30, 30, 8], size=(n - 5 * k, 3))])
    return p.astype(np.float32)


@pytest.mark.parametrize("kind", ["sphere", "box", "pillar"])
def test_float32_rule_against_float64_and_the_geometry(kind):
    """10 000 points per primitive: the float32 (g, cp) agree with the same formulas in float64 to 1e-6 of the room size; cp lies in the
    solid; g is no larger than the distance to any of 1 000 random points of the solid; a point inside has cp == p and g == 0"""
    rng = np.random.default_rng({"sphere": 1, "box": 2, "pillar": 3}[kind])
    o = parse_obstacles([PRIMS[kind]])[0]
    p = _points(o, 10000, rng)
    assert len(p) == 10000
    if kind == "pillar":
        assert np.sum((p[:, 0] == np.float32(o["center"][0])) & (p[:, 1] == np.float32(o["center"][1]))) >= 1000
    g, cp = R.candidate(p, o)
    g64, cp64 = R.candidate(p, o, np.float64)
    tol = 1e-6 * ROOM
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(cp))
    assert np.abs(g - g64).max() <= tol and np.abs(cp - cp64).max() <= tol, (np.abs(g - g64).max(), np.abs(cp - cp64).max())
    assert R.inside(o, cp, tol).all()
    assert np.abs(np.linalg.norm(cp.astype(np.float64) - p, axis=1) - g).max() <= tol        # g is the distance to cp
    within = R.inside(o, p, 0.0) & (g == 0)
    assert within.sum() >= 2000 and np.array_equal(cp[within], p[within])
    assert (g > 0).sum() >= 2000
    solid = R.sample_solid(o, 1000, rng)
    for blk in range(0, len(p), 2000):
        d = np.linalg.norm(p[blk:blk + 2000, None, :].astype(np.float64) - solid[None], axis=2).min(axis=1)
        assert np.all(g[blk:blk + 2000] <= d + tol)


def test_scene_query_picks_the_smallest_candidate_and_agrees_with_float64():
    rng = np.random.default_rng(7)
    table = [SPHERE, BOX, PILLAR, dict(type="sphere", center=[0.0, 3.0, 6.0], radius=1.0)]
    p = np.concatenate([_points(o, 2000, rng) for o in table])
    cp, g, win = R.scene_query(p, table)
    cp64, g64, win64 = R.scene_query64(p, table)
    assert cp.dtype == np.float32 and g.dtype == np.float32
    assert set(np.unique(win)) == {0, 1, 2, 3, 4}
    assert np.abs(g - g64).max() <= 1e-6 * ROOM
    same = win == win64            # (two candidates a rounding apart may swap places; their distances still agree, above)
    assert same.mean() > 0.99 and np.abs(cp[same] - cp64[same]).max() <= 1e-6 * ROOM
    each = np.stack([np.linalg.norm(R._room(p, R.ROOM_LO, R.ROOM_HI, np.float32) - p, axis=1)] + [R.candidate(p, o)[0] for o in table])
    assert np.allclose(g, each.min(axis=0), rtol=0, atol=1e-6 * ROOM)
    assert np.array_equal(R.scene_query(p, [])[2], np.zeros(len(p), dtype=np.int64))          # no table: the room box alone


def test_ties_go_to_the_first_candidate():
    """equal distances: box before obstacle 0 before obstacle 1 (strict `<` against the best so far)"""
    a = dict(type="sphere", center=[0.0, 0.0, 4.0], radius=1.0)
    p = np.asarray([[0.0, 0.0, 4.0], [0.0, 0.0, 6.0]], dtype=np.float32)                       # inside both / 1 m from both
    cp, g, win = R.scene_query(p, [a, dict(a)])
    assert list(win) == [1, 1] and list(g) == [0.0, 1.0]
    cp, g, win = R.scene_query(p, [dict(type="box", lo=[-1, -1, 3], hi=[1, 1, 5]), a])
    assert list(win) == [1, 1]
    # the wall z = 0 and a sphere surface at the same distance 0.5 from p: the room box keeps the point
    s = dict(type="sphere", center=[0.0, 0.0, 2.0], radius=1.0)
    p = np.asarray([[0.0, 0.0, 0.5]], dtype=np.float32)
    cp, g, win = R.scene_query(p, [s])
    assert list(win) == [0] and g[0] == np.float32(0.5) and list(cp[0]) == [0.0, 0.0, 0.0]
    cp, g, win = R.scene_query(np.asarray([[0.0, 0.0, 0.75]], dtype=np.float32), [s])          # closer to the sphere: it wins
    assert list(win) == [1] and list(cp[0]) == [0.0, 0.0, 1.0]


def test_parser_normalises_and_refuses():
    got = parse_obstacles([dict(type="sphere", center=(1, 2, 3), radius=0.1), BOX, dict(type="pillar", center=np.array([1.0, 2.0]), radius=1, z=(0, 1))])
    assert got[0] == dict(type="sphere", center=[1.0, 2.0, 3.0], radius=float(np.float32(0.1)))
    assert got[1] == dict(type="box", lo=[-2.0, 0.5, 0.0], hi=[-1.0, 2.5, 3.0])
    assert got[2] == dict(type="pillar", center=[1.0, 2.0], radius=1.0, z=[0.0, 1.0])
    assert parse_obstacles(None) == [] and parse_obstacles([]) == []
    assert len(parse_obstacles([SPHERE] * 16)) == 16
    bad = [
        [SPHERE] * 17,                                                                        # more than VF_MAX_OBSTACLES
        dict(obstacles=[SPHERE]),                                                             # not a list
        ["sphere"],
        [dict(type="cone", center=[0, 0, 0], radius=1)],
        [dict(type="sphere", center=[0, 0, 0])],                                              # missing key
        [dict(type="sphere", center=[0, 0, 0], radius=1, z=[0, 1])],                          # a key of another primitive
        [dict(type="sphere", center=[0, 0], radius=1)],
        [dict(type="sphere", center=[0, 0, 0], radius=0)],
        [dict(type="sphere", center=[0, 0, 0], radius=-1)],
        [dict(type="sphere", center=[0, 0, float("nan")], radius=1)],
        [dict(type="sphere", center=[0, 0, 0], radius=float("inf"))],
        [dict(type="sphere", center=[0, 0, 0], radius="wide")],
        [dict(type="box", lo=[0, 0, 0], hi=[1, 0, 1])],                                       # lo == hi in one component
        [dict(type="box", lo=[0, 0, 0], hi=[1, 1, -1])],
        [dict(type="box", lo=[0, 0, 0], hi=[1, 1, float("inf")])],
        [dict(type="pillar", center=[0, 0, 0], radius=1, z=[0, 1])],                          # a pillar's centre is (x, y)
        [dict(type="pillar", center=[0, 0], radius=1, z=[1, 1])],
        [dict(type="pillar", center=[0, 0], radius=1, z=[2, 1])],
        [SPHERE, dict(type="pillar", center=[0, 0], radius=0, z=[0, 1])],
    ]
    for b in bad:
        with pytest.raises(ValueError):
            parse_obstacles(b)
    with pytest.raises(ValueError, match="obstacle 1"):
        parse_obstacles([SPHERE, dict(type="box", lo=[0, 0, 0], hi=[0, 1, 1])])


def test_table_rows_follow_the_struct():
    rows = obstacle_rows(parse_obstacles([SPHERE, BOX, PILLAR]))
    assert rows.dtype == np.float32 and rows.shape == (3, 8)
    assert list(rows[0]) == [_lib.OBST_SPHERE, 1.0, -0.5, 1.5, 0, 0, 0, np.float32(0.6)]
    assert list(rows[1]) == [_lib.OBST_BOX, -2.0, 0.5, 0.0, -1.0, 2.5, 3.0, 0]
    assert list(rows[2]) == [_lib.OBST_PILLAR, 3.0, 1.0, 0.0, 0, 0, 2.5, np.float32(0.4)]
    t = obstacle_table(parse_obstacles([SPHERE, BOX, PILLAR]))
    assert ctypes.sizeof(_lib.Obstacle) == 32 and len(t) == 3
    assert (t[2].type, t[2].a[0], t[2].a[1], t[2].a[2], t[2].b[2], t[2].r) == (2, 3.0, 1.0, 0.0, 2.5, np.float32(0.4))
    assert len(obstacle_table([])) == 1


def test_entry_points_exported_and_null_handles_refused():
    """the new symbols are exported with ctypes signatures (ABI stays 11); a null handle is refused before any device work"""
    import __graft_entry__ as ge
    ge.build()
    L = _lib.lib()
    for s in ("vf_env_set_obstacles", "vf_env_obstacle_count", "vf_env_query_ext"):
        assert s in _lib.SIGNATURES and hasattr(L, s)
    assert L.vf_abi_version() == _lib.ABI_VERSION == 11
    assert L.vf_env_obstacle_count(None) == -1
    assert L.vf_env_set_obstacles(None, obstacle_table([]), 0) == -1          # VF_EINVAL
    assert _lib.MAX_OBSTACLES == 16 and (_lib.OBST_SPHERE, _lib.OBST_BOX, _lib.OBST_PILLAR) == (0, 1, 2)


def test_scene_kwargs_key_is_not_reported_as_ignored():
    """scene_kwargs["obstacles"] is this library's own key: the constructor's check of unsupported scene / sensor settings says nothing
    about it, and still names the reference's keys that have no effect without a renderer"""
    import warnings
    from visfly_amd.envs.base import _reject_unsupported
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _reject_unsupported(dict(obstacles=[SPHERE]), None)
    with pytest.warns(UserWarning, match="obj_settings"):
        _reject_unsupported(dict(obstacles=[SPHERE], obj_settings={"path": "x"}), None)
