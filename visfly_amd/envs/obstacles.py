"""Analytic obstacles of an env: the host side of ``scene_kwargs=dict(obstacles=[...])`` and of ``env.obstacles``.

Three solids, at most ``_lib.MAX_OBSTACLES`` per env, shared by all its agents like the room box (include/visfly_amd.h "Analytic
obstacles"):

    dict(type="sphere", center=[x, y, z], radius=r)
    dict(type="box",    lo=[x, y, z], hi=[x, y, z])
    dict(type="pillar", center=[x, y], radius=r, z=[z_lo, z_hi])        a vertical cylinder

``parse_obstacles`` validates such a list and returns it normalised (new dicts, python floats rounded to fp32); ``obstacle_table`` packs a
normalised list into the ``vf_obstacle`` array ``vf_env_set_obstacles`` takes.  No GPU is needed for either.

``scene_kwargs=dict(scene_obstacles=[[...], [...], ...])`` / ``env.scene_obstacles`` give every scene a table of its own instead
(``parse_scene_obstacles``, ``scene_tables`` -> ``vf_env_set_scene_obstacles``); ``safe_spawn`` (``parse_safe_spawn``) has spawns re-drawn
until they keep a clearance from the agent's table.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib

_KEYS = {"sphere": {"type", "center", "radius"}, "box": {"type", "lo", "hi"}, "pillar": {"type", "center", "radius", "z"}}


def _vec(o, key, n, k):
    try:
        v = [float(np.float32(x)) for x in np.asarray(o[key], dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError) as e:
        raise ValueError(f"obstacle {k}: '{key}' must be {n} numbers") from e
    if len(v) != n:
        raise ValueError(f"obstacle {k}: '{key}' must have {n} entries, got {len(v)}")
    if not all(math.isfinite(x) for x in v):
        raise ValueError(f"obstacle {k}: '{key}' is not finite")
    return v


def _radius(o, k):
    try:
        r = float(np.float32(o["radius"]))
    except (TypeError, ValueError) as e:
        raise ValueError(f"obstacle {k}: 'radius' must be a number") from e
    if not math.isfinite(r) or r <= 0.0:
        raise ValueError(f"obstacle {k}: 'radius' must be finite and > 0")
    return r


def parse_obstacles(obstacles):
    """validate a list of obstacle dicts -> the normalised list (see the module docstring); ValueError names the entry at fault"""
    if obstacles is None:
        return []
    if isinstance(obstacles, dict) or not hasattr(obstacles, "__iter__"):
        raise ValueError("obstacles must be a list of dicts")
    obstacles = list(obstacles)
    if len(obstacles) > _lib.MAX_OBSTACLES:
        raise ValueError(f"at most {_lib.MAX_OBSTACLES} obstacles per env, got {len(obstacles)}")
    out = []
    for k, o in enumerate(obstacles):
        if not isinstance(o, dict) or o.get("type") not in _KEYS:
            raise ValueError(f"obstacle {k}: a dict with type 'sphere', 'box' or 'pillar' is expected")
        kind = o["type"]
        if set(o) != _KEYS[kind]:
            raise ValueError(f"obstacle {k}: a {kind} takes exactly the keys {sorted(_KEYS[kind])}, got {sorted(o)}")
        if kind == "sphere":
            out.append(dict(type="sphere", center=_vec(o, "center", 3, k), radius=_radius(o, k)))
        elif kind == "box":
            lo, hi = _vec(o, "lo", 3, k), _vec(o, "hi", 3, k)
            if not all(a < b for a, b in zip(lo, hi)):
                raise ValueError(f"obstacle {k}: a box needs lo < hi in every component")
            out.append(dict(type="box", lo=lo, hi=hi))
        else:
            z = _vec(o, "z", 2, k)
            if not z[0] < z[1]:
                raise ValueError(f"obstacle {k}: a pillar needs z[0] < z[1]")
            out.append(dict(type="pillar", center=_vec(o, "center", 2, k), radius=_radius(o, k), z=z))
    return out


def obstacle_rows(obstacles):
    """normalised list -> (n, 8) float32 rows [type, a0, a1, a2, b0, b1, b2, r] in vf_obstacle's field order"""
    rows = np.zeros((len(obstacles), 8), dtype=np.float32)
    for k, o in enumerate(obstacles):
        if o["type"] == "sphere":
            rows[k] = [_lib.OBST_SPHERE, *o["center"], 0, 0, 0, o["radius"]]
        elif o["type"] == "box":
            rows[k] = [_lib.OBST_BOX, *o["lo"], *o["hi"], 0]
        else:
            rows[k] = [_lib.OBST_PILLAR, o["center"][0], o["center"][1], o["z"][0], 0, 0, o["z"][1], o["radius"]]
    return rows


def obstacle_table(obstacles):
    """normalised list -> ctypes array of vf_obstacle (length >= 1, so that an empty table still has an address)"""
    rows = obstacle_rows(obstacles)
    table = (_lib.Obstacle * max(1, len(obstacles)))()
    for k, r in enumerate(rows):
        table[k].type = int(r[0])
        for d in range(3):
            table[k].a[d], table[k].b[d] = float(r[1 + d]), float(r[4 + d])
        table[k].r = float(r[7])
    return table


def parse_scene_obstacles(scene_obstacles, num_scene):
    """``scene_kwargs["scene_obstacles"]``: exactly ``num_scene`` obstacle lists, one per scene (rows ``s * num_agent_per_scene ..`` of the
    env belong to scene ``s``), each validated by ``parse_obstacles`` -> the list of normalised lists; ValueError names the scene"""
    if isinstance(scene_obstacles, dict) or not hasattr(scene_obstacles, "__iter__"):
        raise ValueError("scene_obstacles must be a list of obstacle lists, one per scene")
    scenes = list(scene_obstacles)
    if len(scenes) != num_scene:
        raise ValueError(f"scene_obstacles must have one list per scene: num_scene = {num_scene}, got {len(scenes)}")
    out = []
    for s, one in enumerate(scenes):
        try:
            out.append(parse_obstacles([] if one is None else one))
        except ValueError as e:
            raise ValueError(f"scene {s}: {e}") from e
    return out


def scene_tables(scenes):
    """normalised per-scene lists -> (vf_obstacle[n_scenes * MAX_OBSTACLES], int32[n_scenes]) as vf_env_set_scene_obstacles takes them"""
    tables = (_lib.Obstacle * (max(1, len(scenes)) * _lib.MAX_OBSTACLES))()
    counts = (C.c_int32 * max(1, len(scenes)))()
    for s, one in enumerate(scenes):
        counts[s] = len(one)
        for k, row in enumerate(obstacle_table(one)[:len(one)]):
            dst = tables[s * _lib.MAX_OBSTACLES + k]
            dst.type, dst.r = row.type, row.r
            for d in range(3):
                dst.a[d], dst.b[d] = row.a[d], row.b[d]
    return tables, counts


def parse_safe_spawn(value, uav_radius):
    """``scene_kwargs["safe_spawn"]`` / ``env.safe_spawn``: None / False / 0 -> 0.0 (off), True -> uav_radius, a number -> that clearance"""
    if value is None or value is False:
        return 0.0
    if value is True:
        return float(np.float32(uav_radius))
    try:
        c = float(np.float32(value))
    except (TypeError, ValueError) as e:
        raise ValueError("safe_spawn must be a bool or a clearance in metres") from e
    if not math.isfinite(c):
        raise ValueError("safe_spawn must be finite")
    return max(c, 0.0)
