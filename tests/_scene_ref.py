"""Host restatements for per-scene obstacle tables and collision-free spawns (include/visfly_amd.h "Per-scene tables", "Collision-free
spawns"), built from the existing pieces: tests/_obstacle_ref.py answers the query, once per scene; tests/_streams.py draws the Philox
words; the spawner's one-reduction sin / cos is oracle.sincos_spawn (pinned by tests/test_device_streams.py).

``spawn_attempt`` is attempt a of spawn_agent in numpy float32, every operation rounded on its own in the device's order (attempt 0 must
equal oracle.spawn bit for bit: tests/test_scene_tables.py).  ``safe_spawn_ref`` runs the rejection loop.  The device forms the distance
it compares with the clearance as an FMA chain in fp32; here it is the float64 norm of the float32 vector, and the loop ASSERTS that no
candidate's distance lies within 1e-6 (relative) of the clearance -- ten times the chain's own error --, so that no accept / reject
decision of the reference hinges on the norm's last bits.
"""
import numpy as np

import _obstacle_ref as R
import oracle
from _streams import spawn_words

f32 = np.float32
SPAWN_TRIES = 16
FIELDS = (("pos", "position"), ("ori", "orientation"), ("vel", "velocity"), ("omg", "angular_velocity"))


def scene_of(rows, agents_per_scene, n_scenes):
    """row of the env -> its scene (rows are laid out scene by scene)"""
    return np.minimum(np.asarray(rows, np.int64) // agents_per_scene, n_scenes - 1)


def scene_query_rows(p, rows, tables, agents_per_scene):
    """_obstacle_ref.scene_query, once per scene, for positions p (n,3) of env rows `rows` -> cp (n,3) f32, win (n,), dis (n,) f64, oob"""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    scn = scene_of(rows, agents_per_scene, len(tables))
    cp, win = np.empty_like(p), np.zeros(len(p), np.int64)
    for s in np.unique(scn):
        m = scn == s
        cp[m], _, win[m] = R.scene_query(p[m], tables[s])
    vec = (cp - p).astype(np.float64)
    oob = np.any((p < f32(R.ROOM_LO)) | (p > f32(R.ROOM_HI)), axis=1)
    return cp, win, np.sqrt((vec * vec).sum(axis=1)), oob


def spawn_attempt(seed, ids, episode, boxes, attempt, indexed):
    """attempt `attempt` of the device spawner for global agent ids `ids` starting episode `episode`: Philox blocks 8 a, 8 a + 1, 8 a + 2
    -> state (n,13) f32 [p q v w], t (n,) f32.  boxes: what visfly_amd.envs.randomization.spawn_boxes returns"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    r = spawn_words(seed, ids, episode, (8 * attempt, 8 * attempt + 1, 8 * attempt + 2))
    u = (r & np.uint64(0xFFFFFF)).astype(f32) * f32(1.0 / 16777216.0)
    top = r >> np.uint64(24)
    pick = top[:, 0] | (top[:, 1] << np.uint64(8)) | (top[:, 2] << np.uint64(16)) | (top[:, 3] << np.uint64(24))
    tbits = top[:, 4] | (top[:, 5] << np.uint64(8)) | (top[:, 6] << np.uint64(16))
    b = (pick % np.uint64(len(boxes))).astype(np.int64) if len(boxes) > 1 else np.zeros(len(ids), np.int64)
    val = {}
    for j, (name, f) in enumerate(FIELDS):
        mean = np.array([bx[f]["mean"] for bx in boxes], f32)[b]
        half = np.array([bx[f]["half"] for bx in boxes], f32)[b]
        m = f32(2.0) * u[:, 3 * j:3 * j + 3] - f32(1.0)
        val[name] = mean + m * half if name == "pos" else m * half + mean
        assert val[name].dtype == f32
    eul = val["ori"]
    sy, cy = oracle.sincos_spawn(eul[:, 2] * f32(0.5))
    sp, cp = oracle.sincos_spawn(eul[:, 1] * f32(0.5))
    sr, cr = oracle.sincos_spawn(eul[:, 0] * f32(0.5))
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)
    state = np.concatenate([val["pos"], q, val["vel"], val["omg"]], 1)
    assert state.dtype == f32
    t = (tbits & np.uint64(0xFFFFFF)).astype(f32) * f32(1.0 / 16777216.0) * f32(3.14) * f32(2.0) if indexed else np.zeros(len(ids), f32)
    return state, t.astype(f32)


def safe_spawn_ref(seed, rows, episode, boxes, tables, agents_per_scene, clearance, indexed, agent0=0):
    """the collision-free spawn of env rows `rows` (global ids agent0 + rows) for episode `episode` (scalar or per row) -> state (n,13),
    t (n,), attempt (n,): the index 0 .. 15 of the accepted attempt, exhausted (n,) bool: the 16th candidate was kept although it is
    closer than `clearance`.  tables: one obstacle list per scene (a shared table: [table] with agents_per_scene = N)"""
    rows = np.asarray(rows, np.int64).reshape(-1)
    episode = np.broadcast_to(np.asarray(episode, np.int64), rows.shape)
    n = len(rows)
    state, t = np.zeros((n, 13), f32), np.zeros(n, f32)
    attempt, exhausted = np.zeros(n, np.int64), np.zeros(n, bool)
    todo = np.arange(n)
    clearance = float(f32(clearance))
    for a in range(SPAWN_TRIES):
        if not len(todo):
            break
        st, tt = spawn_attempt(seed, agent0 + rows[todo], episode[todo], boxes, a, indexed)
        state[todo], t[todo], attempt[todo] = st, tt, a
        if not clearance > 0.0:
            break
        _, _, dis, _ = scene_query_rows(st[:, :3], rows[todo], tables, agents_per_scene)
        assert (np.abs(dis - clearance) > 1e-6 * clearance).all(), "a candidate's distance ties with the clearance: pick another seed"
        rejected = dis < clearance
        if a == SPAWN_TRIES - 1:
            exhausted[todo] = rejected
        todo = todo[rejected]
    return state, t, attempt, exhausted


# ---- the cases tests/test_scene_tables.py (CPU) and tests/test_safe_spawn_gpu.py share -----------------------------------------------------
def _rk(*pos):
    """a Union of Uniform spawn boxes with the given (mean, half) position ranges; orientation, velocity and body rates as _streams.UNION"""
    from _streams import _box
    return {"state_generator": {"class": "Union", "kwargs": [{"randomizers_kwargs": [
        _box(p, [0.1, -0.2, 0.3], ([0.5, 0., 0.], [1., 0.5, 0.5]), ([0., 0., 0.], [0.3, 0.2, 0.1])) for p in pos]}]}}


SEED = 11
N_SAFE = 192
# two spawn boxes, A around [1, 0, 1.5] (HoverEnv's) and B around [-2, 1, 1], with solids inside both
SAFE_RK = _rk(([1., 0., 1.5], [1., 1., .5]), ([-2., 1., 1.], [.5, .5, .5]))
T0 = [dict(type="sphere", center=[1.0, 0.0, 1.5], radius=0.6), dict(type="box", lo=[-2.3, 0.7, 0.5], hi=[-1.8, 1.3, 1.5])]
T1 = [dict(type="pillar", center=[1.5, 0.5], radius=0.35, z=[0.0, 3.0]), dict(type="sphere", center=[-2.0, 1.0, 1.0], radius=0.3),
      dict(type="box", lo=[0.2, -1.0, 1.0], hi=[0.8, -0.2, 2.0])]
T2 = [dict(type="box", lo=[0.0, -1.0, 1.0], hi=[2.0, 0.0, 2.0])]          # half of box A
SAFE_SHARED = T0 + T1[:1]
SAFE_SCENES = [T0, T1, T2]                                                 # (3, 64) and, for straddling waves, (3, 48) with 144 agents
# a spawn box wholly inside a box solid: every attempt is rejected, the 16th candidate is kept
TRAP_RK = _rk(([1., 0., 1.5], [.2, .2, .2]))
TRAP = [dict(type="box", lo=[0.0, -1.0, 0.5], hi=[2.0, 1.0, 2.5])]
UAV_RADIUS = 0.1


def boxes_of(random_kwargs):
    from visfly_amd.envs.randomization import spawn_boxes
    return spawn_boxes(random_kwargs)


def fma32(a, b, c):
    """fp32 fma through float64: the product of two fp32 values is exact there, the sum is rounded to 53 bits and then to 24 -- equal to the
    single rounding unless the 53-bit sum lands exactly on an fp32 tie, which inexact sums do with probability ~2^-29"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def chained_norm(v):
    """the kernels' norm3: sqrt(fma(z, z, fma(y, y, x x))) in fp32"""
    v = np.asarray(v, f32)
    return np.sqrt(fma32(v[:, 2], v[:, 2], fma32(v[:, 1], v[:, 1], v[:, 0] * v[:, 0])))
