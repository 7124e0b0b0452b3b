"""Per-scene obstacle tables and collision-free spawns, the parts that need no GPU: parsing of scene_kwargs["scene_obstacles"] /
["safe_spawn"], the three new C entry points on null handles, their ctypes signatures, the ABI version, and the host restatement
tests/_scene_ref.py that the GPU tests compare the device with -- its attempt 0 is the pinned single draw (oracle.spawn), and with the
GPU tests' tables it re-draws for some agents and exhausts its 16 tries for none (for all in the crafted trap)."""
import ctypes as C

import numpy as np
import pytest

import _scene_ref as S
import oracle
from visfly_amd import _lib
from visfly_amd.envs.obstacles import parse_obstacles, parse_safe_spawn, parse_scene_obstacles, scene_tables

BALL = dict(type="sphere", center=[1.0, 0.0, 1.5], radius=0.6)
WALL = dict(type="box", lo=[0.0, -1.0, 0.0], hi=[0.5, 1.0, 2.0])
POST = dict(type="pillar", center=[2.0, 1.0], radius=0.25, z=[0.0, 3.0])


def test_scene_lists_are_parsed_per_scene():
    got = parse_scene_obstacles([[BALL], [], [WALL, POST]], 3)
    assert got == [parse_obstacles([BALL]), [], parse_obstacles([WALL, POST])]
    assert parse_scene_obstacles([None, [BALL]], 2) == [[], parse_obstacles([BALL])]
    tables, counts = scene_tables(got)
    assert list(counts) == [1, 0, 2] and len(tables) == 3 * _lib.MAX_OBSTACLES
    assert tables[0].type == _lib.OBST_SPHERE and tables[2 * 16].type == _lib.OBST_BOX and tables[2 * 16 + 1].type == _lib.OBST_PILLAR
    assert tables[2 * 16 + 1].r == np.float32(0.25) and tables[0].a[2] == 1.5


@pytest.mark.parametrize("n", [1, 2, 4])
def test_wrong_number_of_scenes_is_refused(n):
    with pytest.raises(ValueError, match="num_scene = 3"):
        parse_scene_obstacles([[BALL]] * n, 3)


def test_not_a_list_of_lists_is_refused():
    for bad in (BALL, 3):
        with pytest.raises(ValueError, match="scene_obstacles"):
            parse_scene_obstacles(bad, 1)


def test_bad_entry_names_its_scene_and_entry():
    with pytest.raises(ValueError, match=r"scene 1: obstacle 2: 'radius'"):
        parse_scene_obstacles([[BALL], [BALL, WALL, dict(BALL, radius=-1.0)]], 2)
    with pytest.raises(ValueError, match=r"scene 0: at most 16"):
        parse_scene_obstacles([[BALL] * 17], 1)


def test_both_keys_together_are_refused():
    """raised before any device work (the same place scene_kwargs["obstacles"] is parsed)"""
    from visfly_amd.envs import HoverEnv
    with pytest.raises(ValueError, match="not both"):
        HoverEnv(num_agent_per_scene=4, num_scene=2, visual=False, device="cuda:0",
                 scene_kwargs=dict(obstacles=[BALL], scene_obstacles=[[BALL], []]))
    with pytest.raises(ValueError, match="num_scene = 2"):
        HoverEnv(num_agent_per_scene=4, num_scene=2, visual=False, device="cuda:0", scene_kwargs=dict(scene_obstacles=[[BALL]]))
    with pytest.raises(ValueError, match="safe_spawn needs spawn='device'"):
        HoverEnv(num_agent_per_scene=4, visual=False, device="cuda:0", spawn="replay", scene_kwargs=dict(obstacles=[BALL], safe_spawn=True))


def test_safe_spawn_values():
    assert parse_safe_spawn(None, 0.1) == 0.0 and parse_safe_spawn(False, 0.1) == 0.0 and parse_safe_spawn(0, 0.1) == 0.0
    assert parse_safe_spawn(True, 0.1) == float(np.float32(0.1)) and parse_safe_spawn(0.25, 0.1) == 0.25
    assert parse_safe_spawn(-1.0, 0.1) == 0.0
    for bad in ("near", float("nan"), float("inf")):
        with pytest.raises(ValueError):
            parse_safe_spawn(bad, 0.1)


def test_null_handles_are_refused_and_the_abi_is_11():
    L = _lib.lib()
    assert L.vf_abi_version() == 11 == _lib.ABI_VERSION
    tables, counts = scene_tables([parse_obstacles([BALL])])
    assert L.vf_env_set_scene_obstacles(None, tables, counts, 1, 4) == -1 and "null handle" in L.vf_last_error().decode()
    assert L.vf_env_scene_count(None) == -1
    assert L.vf_env_set_safe_spawn(None, 0.1) == -1 and "null handle" in L.vf_last_error().decode()


def test_new_symbols_are_exported_with_signatures():
    L = _lib.lib()
    sig = _lib.SIGNATURES
    assert sig["vf_env_set_scene_obstacles"] == (C.c_int, [_lib._vp, C.POINTER(_lib.Obstacle), C.POINTER(C.c_int32), C.c_int32, C.c_int32])
    assert sig["vf_env_scene_count"] == (C.c_int32, [_lib._vp]) and sig["vf_env_set_safe_spawn"] == (C.c_int, [_lib._vp, C.c_float])
    for name in ("vf_env_set_scene_obstacles", "vf_env_scene_count", "vf_env_set_safe_spawn"):
        assert getattr(L, name).argtypes == sig[name][1]
    assert _lib.SPAWN_TRIES == S.SPAWN_TRIES == 16


# ---- the host restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indexed", [False, True])
def test_attempt_zero_is_the_pinned_single_draw(indexed):
    boxes = S.boxes_of(S.SAFE_RK)
    rows = np.arange(500)
    for ep in (1, 2, 77):
        st, t = S.spawn_attempt(S.SEED, 4096 + rows, ep, boxes, 0, indexed)
        want, wt = oracle.spawn(S.SEED, rows, np.full(len(rows), ep), boxes, indexed, agent0=4096)
        assert np.array_equal(st.view(np.uint32), want.view(np.uint32)) and np.array_equal(t.view(np.uint32), wt.view(np.uint32))
    other, _ = S.spawn_attempt(S.SEED, 4096 + rows, 1, boxes, 1, indexed)
    assert not np.array_equal(other[:, :3], S.spawn_attempt(S.SEED, 4096 + rows, 1, boxes, 0, indexed)[0][:, :3])
    assert len(np.unique(other[:, 0] > -0.5)) == 2          # both boxes of the Union are picked


CASES = {"shared": ([S.SAFE_SHARED], S.N_SAFE, S.N_SAFE), "3x48": (S.SAFE_SCENES, 48, 144), "3x64": (S.SAFE_SCENES, 64, 192)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_safe_spawn_ref_is_self_consistent(case):
    """every accepted state is attempt `a` of its agent, every earlier attempt was closer than the clearance, the accepted one is not; some
    agents need at least 2 attempts (the GPU tests would pass with a no-op otherwise) and none all 16"""
    tables, aps, n = CASES[case]
    boxes, rows = S.boxes_of(S.SAFE_RK), np.arange(n)
    redrawn = 0
    for ep in range(1, 7):
        st, t, att, exhausted = S.safe_spawn_ref(S.SEED, rows, ep, boxes, tables, aps, S.UAV_RADIUS, ep > 1)
        assert not exhausted.any() and att.max() < S.SPAWN_TRIES - 1
        for a in range(att.max() + 1):
            cand, ct = S.spawn_attempt(S.SEED, rows, ep, boxes, a, ep > 1)
            _, _, dis, _ = S.scene_query_rows(cand[:, :3], rows, tables, aps)
            assert (dis[att > a] < S.UAV_RADIUS).all()
            m = att == a
            assert (dis[m] >= S.UAV_RADIUS).all()
            assert np.array_equal(st[m].view(np.uint32), cand[m].view(np.uint32)) and np.array_equal(t[m], ct[m])
        redrawn += int((att >= 1).sum())
        off, _, att0, _ = S.safe_spawn_ref(S.SEED, rows, ep, boxes, tables, aps, 0.0, ep > 1)
        assert not att0.any() and np.array_equal(off, S.spawn_attempt(S.SEED, rows, ep, boxes, 0, ep > 1)[0])
    assert redrawn >= 20, redrawn


def test_rows_of_different_scenes_meet_different_tables():
    boxes, rows = S.boxes_of(S.SAFE_RK), np.arange(144)
    _, _, a48, _ = S.safe_spawn_ref(S.SEED, rows, 1, boxes, S.SAFE_SCENES, 48, S.UAV_RADIUS, False)
    _, _, ash, _ = S.safe_spawn_ref(S.SEED, rows, 1, boxes, [S.T0], 144, S.UAV_RADIUS, False)
    assert np.array_equal(a48[:48], ash[:48]) and not np.array_equal(a48[48:], ash[48:])


def test_trap_exhausts_every_agent():
    st, _, att, exhausted = S.safe_spawn_ref(S.SEED, np.arange(S.N_SAFE), 1, S.boxes_of(S.TRAP_RK), [S.TRAP], S.N_SAFE, S.UAV_RADIUS, False)
    assert exhausted.all() and (att == S.SPAWN_TRIES - 1).all()
    want, _ = S.spawn_attempt(S.SEED, np.arange(S.N_SAFE), 1, S.boxes_of(S.TRAP_RK), 15, False)
    assert np.array_equal(st, want)
