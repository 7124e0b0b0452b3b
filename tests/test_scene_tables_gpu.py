"""Per-scene obstacle tables (scene_kwargs["scene_obstacles"] / env.scene_obstacles; vf_env_set_scene_obstacles; scene_collision<VF_TABLE_SCENES>).

(1) the device query equals tests/_obstacle_ref.py, called once per scene, bit for bit, for uniform, straddling and partial waves;
(2) the same table in every scene is the shared table; (3) a row depends on its own scene's table only; (4) the fused step equals the
split step fed the reference's point; (5) the navigation adjoint: equal tables = the shared table's gradients (which
tests/test_obstacles_bptt_gpu.py pins to the reference's autograd), distinct tables row by row; (6) the persistent entry points refuse,
the trainers step launch by launch, clearing the tables restores them."""
import ctypes as C

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

import _obstacle_ref as R
import _scene_ref as S
from visfly_amd import _lib
from visfly_amd.envs import HoverEnv, NavigationEnv, NavigationEnv2

DEV = "cuda:0"
KW = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)


def _spawn(mean, half):
    return {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": mean, "half": half}}]}}


def _mk(cls, ns, aps, scenes=None, shared=None, seed=7, steps=48, dyn=KW, **kw):
    if scenes is not None:
        kw["scene_kwargs"] = dict(scene_obstacles=scenes)
    elif shared is not None:
        kw["scene_kwargs"] = dict(obstacles=shared)
    env = cls(num_agent_per_scene=aps, num_scene=ns, seed=seed, visual=False, dynamics_kwargs=dict(dyn), device=DEV, tensor_output=True,
              max_episode_steps=steps, **kw)
    env.reset()
    return env


def _act(n, t, g):
    """the action schedule of tests/test_obstacles_gpu.py"""
    act = (th.rand((n, 4), device="cuda", generator=g) * 2 - 1) * (1.0 if t % 3 else 0.05) + th.tensor([-1 / 3, 0, 0, 0], device="cuda") * (t % 3 == 0)
    return act.clamp(-1, 1).contiguous()


def _bits(x):
    x = x.detach().contiguous()
    return x.view(th.int32) if x.dtype == th.float32 else x


def _same(a, b):
    return th.equal(_bits(a), _bits(b))


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------------
def _random_tables(ns, rng):
    """counts 16, 0, 1, 5, 3, 16, ... ; all three primitives in every table of 3 or more"""
    def prim(k):
        c = rng.uniform([-2.0, -3.0, 0.5], [4.0, 3.0, 3.0])
        if k % 3 == 0:
            return dict(type="sphere", center=c.tolist(), radius=float(rng.uniform(0.2, 0.8)))
        if k % 3 == 1:
            return dict(type="box", lo=c.tolist(), hi=(c + rng.uniform(0.3, 1.2, 3)).tolist())
        return dict(type="pillar", center=c[:2].tolist(), radius=float(rng.uniform(0.15, 0.5)), z=[0.0, float(rng.uniform(1.0, 3.0))])
    counts = [16, 0, 1, 5, 3]
    return [[prim(k + s) for k in range(counts[s % len(counts)])] for s in range(ns)]


def _surface(o, rng):
    """a point of the solid's surface (float64)"""
    if o["type"] == "sphere":
        v = rng.normal(size=3)
        return np.asarray(o["center"]) + o["radius"] * v / np.linalg.norm(v)
    if o["type"] == "box":
        lo, hi = np.asarray(o["lo"]), np.asarray(o["hi"])
        x = lo + rng.uniform(size=3) * (hi - lo)
        d = rng.integers(3)
        x[d] = (lo, hi)[rng.integers(2)][d]
        return x
    a = rng.uniform(0, 2 * np.pi)
    return np.array([o["center"][0] + o["radius"] * np.cos(a), o["center"][1] + o["radius"] * np.sin(a), rng.uniform(o["z"][0], o["z"][1])])


def _positions(tables, aps, rng):
    """per row, in turn: anywhere in the flown region, inside a solid of the row's scene, on its surface, just outside it"""
    n = len(tables) * aps
    p = rng.uniform([-3.0, -4.0, 0.1], [5.0, 4.0, 4.0], size=(n, 3))
    for i in range(n):
        tab = R.parse_obstacles(tables[i // aps])
        if not tab or i % 4 == 0:
            continue
        o = tab[rng.integers(len(tab))]
        if i % 4 == 1:
            p[i] = R.sample_solid(o, 1, rng)[0]
        else:
            x = _surface(o, rng)
            p[i] = x if i % 4 == 2 else x + 0.05 * (x - R.sample_solid(o, 1, rng)[0]) / 1.0
    p[:, 2] = np.maximum(p[:, 2], 0.05)
    return p.astype(np.float32)


@pytest.mark.parametrize("ns,aps", [(64, 1), (3, 48), (3, 64), (2, 100)])
def test_device_query_equals_host_reference_per_scene(ns, aps):
    rng = np.random.default_rng(100 * ns + aps)
    tables = _random_tables(ns, rng)
    n = ns * aps
    env = _mk(HoverEnv, ns, aps, tables)
    L = _lib.lib()
    assert L.vf_env_scene_count(env._h) == ns and L.vf_env_obstacle_count(env._h) == max(len(t) for t in tables)
    assert env.scene_obstacles == [R.parse_obstacles(t) for t in tables]
    with pytest.raises(ValueError, match="scene_obstacles"):
        env.obstacles
    winners, inside = set(), 0
    for rnd in range(3):
        p = _positions(tables, aps, rng)
        fs = env.envs.dynamics.full_state.cpu().clone()
        fs[:, :3] = th.from_numpy(p)
        env.reset(state=fs)
        cp, win, _, _ = S.scene_query_rows(p, np.arange(n), tables, aps)
        vec = cp - p
        dis = S.chained_norm(vec)
        assert _same(env.collision_point.cpu(), th.from_numpy(cp)), rnd
        assert _same(env.collision_vector.cpu(), th.from_numpy(vec)), rnd
        assert _same(env.collision_dis.cpu(), th.from_numpy(dis)), rnd
        assert th.equal(env.is_collision.cpu(), th.from_numpy(dis < np.float32(0.1))), rnd
        scn = np.arange(n) // aps
        for i in np.nonzero(win > 0)[0]:
            winners.add(R.parse_obstacles(tables[scn[i]])[win[i] - 1]["type"])
        winners |= {"room"} if (win == 0).any() else set()
        inside += int(((dis == 0) & (win > 0)).sum())
    assert winners == {"room", "sphere", "box", "pillar"}, winners
    assert inside > 0


# ---- (2), (3) ------------------------------------------------------------------------------------------------------------------------------
BALL = dict(type="sphere", center=[1.0, 0.0, 1.5], radius=0.6)            # the middle of HoverEnv's spawn box
NAV_RK = _spawn([1., 0., 1.5], [0.0, 2., 1.])
NAV_TABLE = [dict(type="box", lo=[1.3, -2.0, 0.0], hi=[1.8, -1.0, 3.0]), dict(type="pillar", center=[1.5, 2.0], radius=0.2, z=[0.0, 3.0])]
NAV_B = [dict(type="box", lo=[1.3, 0.0, 0.0], hi=[1.8, 1.0, 3.0])]
NAV_C = [dict(type="pillar", center=[1.6, -0.5], radius=0.25, z=[0.0, 3.0]), dict(type="sphere", center=[2.2, 1.0, 1.5], radius=0.5), NAV_TABLE[0]]
TASKS = {"hover": (HoverEnv, {}, [BALL], [dict(BALL, center=[1.5, 0.5, 1.2])]), "nav": (NavigationEnv, dict(random_kwargs=NAV_RK), NAV_TABLE, NAV_C)}


def _run(envs, n, steps, seed=3):
    """step every env with the same actions; -> per env the stacked (state rows, reward, done) and the counters after the last step"""
    g = th.Generator(device="cuda").manual_seed(seed)
    rec = [[] for _ in envs]
    for t in range(steps):
        act = _act(n, t, g)
        for e, r in zip(envs, rec):
            o, rew, d, _ = e.step(act)
            r.append((o["state"].clone(), rew.clone(), d.clone(), e._ep_return.clone(), e._ep_length.clone(), e._ep_flags.clone()))
    return [[th.stack([s[k] for s in r]) for k in range(6)] + [e.state.clone(), e.state_slab.clone()] for e, r in zip(envs, rec)]


@pytest.mark.parametrize("collision_reset", [True, False])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("task", ["hover", "nav"])
def test_equal_scene_tables_are_the_shared_table(task, integrator, collision_reset):
    """192 agents in 3 scenes, 120 steps (> 2 episodes of 48): states, rewards, done flags, episode outputs and the slab with its counters"""
    cls, kw, table, _ = TASKS[task]
    dyn = dict(KW, integrator=integrator)
    a = _mk(cls, 3, 64, scenes=[table] * 3, dyn=dyn, is_collision_reset=collision_reset, **kw)
    b = _mk(cls, 3, 64, shared=table, dyn=dyn, is_collision_reset=collision_reset, **kw)
    c = _mk(cls, 3, 64, dyn=dyn, is_collision_reset=collision_reset, **kw)
    assert a.scene_obstacles == b.scene_obstacles == [R.parse_obstacles(table)] * 3
    ra, rb, rc = _run([a, b, c], 192, 120)
    for x, y in zip(ra, rb):
        assert _same(x, y)
    assert int(ra[2].sum()) > 192                            # re-spawns happened ...
    assert not (_same(ra[1], rc[1]) and _same(ra[2], rc[2]) and _same(ra[5], rc[5]))   # ... and the table was seen (reward, done or the collided bit)


@pytest.mark.parametrize("task", ["hover", "nav"])
def test_rows_depend_on_their_own_scene_only(task):
    """scenes [T0, T1] of 96 agents (the wave of rows 64 .. 127 straddles them) against two shared-table envs over the same 192 rows"""
    cls, kw, t0, t1 = TASKS[task]
    both = _mk(cls, 2, 96, scenes=[t0, t1], **kw)
    e0, e1 = _mk(cls, 2, 96, shared=t0, **kw), _mk(cls, 2, 96, shared=t1, **kw)
    rb, r0, r1 = _run([both, e0, e1], 192, 120)
    for k in range(7):                                       # (the slab is tiled: compared through the state rows)
        x, y0, y1 = rb[k], r0[k], r1[k]
        rows = (lambda z, s: z[:, s]) if k < 6 else (lambda z, s: z[s])
        assert _same(rows(x, slice(0, 96)), rows(y0, slice(0, 96))), k
        assert _same(rows(x, slice(96, 192)), rows(y1, slice(96, 192))), k
    assert not _same(r0[1], r1[1])                           # the two tables are told apart
    assert int(rb[2].sum()) > 192


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------------
# NavigationEnv2 observes collision_vector also for a re-spawned agent, where the table-less env of the split step answers with the room
# box: its agents spawn where the floor is the closest surface under every table (tests/test_obstacles_gpu.py: NAV2_RK, NAV2_TABLE)
NAV2_RK = _spawn([1., 0., 0.35], [1.0, 1.0, 0.1])
NAV2_TABLE = [dict(type="box", lo=[-1.0, -2.0, 1.0], hi=[3.0, 2.0, 1.3]), dict(type="box", lo=[2.5, -3.0, 0.0], hi=[3.0, 3.0, 1.0]),
              dict(type="pillar", center=[-0.7, 0.0], radius=0.2, z=[0.0, 1.0])]
NAV2_SCENES = [NAV2_TABLE, NAV2_TABLE[:2], [NAV2_TABLE[0], dict(NAV2_TABLE[1], lo=[2.6, -3.0, 0.0], hi=[3.1, 3.0, 1.0]), dict(NAV2_TABLE[2], center=[-0.7, 0.5])]]
SPLIT = {"nav": (NavigationEnv, dict(random_kwargs=NAV_RK), [NAV_TABLE, NAV_B, NAV_C]), "nav2": (NavigationEnv2, dict(random_kwargs=NAV2_RK), NAV2_SCENES)}


@pytest.mark.parametrize("ns,aps", [(3, 48), (2, 64)])
@pytest.mark.parametrize("task", ["nav", "nav2"])
def test_fused_step_equals_split_step_per_scene(task, ns, aps):
    cls, kw, scenes = SPLIT[task]
    scenes, n = scenes[:ns], ns * aps
    a, b = _mk(cls, ns, aps, scenes=scenes, **kw), _mk(cls, ns, aps, **kw)
    g = th.Generator(device="cuda").manual_seed(3)
    seen, hits, ended = 0, 0, 0
    for t in range(120):
        act = _act(n, t, g)
        o1, r1, d1, _ = a.step(act)
        pose = b.step_begin(act)
        p = pose["position"].cpu().numpy()
        cp, win, dis, oob = S.scene_query_rows(p, np.arange(n), scenes, aps)
        o2, r2, d2, _ = b.step_finish(th.from_numpy(cp).to(DEV), th.from_numpy(oob).to(DEV))
        assert _same(r1, r2) and th.equal(d1, d2), t
        for k in o1.keys():
            assert _same(o1[k], o2[k]), (t, k)
        for name in ("_ep_return", "_ep_length", "_ep_flags", "_terminal_obs"):
            assert _same(getattr(a, name)[d1], getattr(b, name)[d1]), (t, name)
        alive = ~d1
        assert th.equal(a.is_collision[alive], b.is_collision[alive]) and _same(a.collision_dis[alive], b.collision_dis[alive]), t
        seen += int((win > 0).sum())
        hits += int(((win > 0) & (dis < 0.1)).sum())
        ended += int(d1.sum())
    assert _same(a.state, b.state)
    print(task, ns, aps, dict(obstacle_closest=seen, obstacle_hits=hits, ended=ended))
    assert seen > 0 and ended > n


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------------
def _grads(ns, aps, H=16, **tables):
    env = _mk(NavigationEnv, ns, aps, random_kwargs=NAV_RK, requires_grad=True, **tables)
    n = ns * aps
    g = th.Generator(device="cuda").manual_seed(9)
    acts = th.stack([_act(n, t, g) for t in range(H)]).requires_grad_(True)
    Wr, Wo = th.randn((H, n), device=DEV, generator=g), th.randn((H, n, 13), device=DEV, generator=g) * 0.1
    loss, rewards = 0, []
    for t in range(H):
        obs, r, d, _ = env.step(acts[t], is_test=True)
        assert r.requires_grad
        rewards.append(r.detach().clone())
        loss = loss + (Wr[t] * r).sum() + (Wo[t] * obs["state"]).sum()
    loss.backward()
    assert bool(th.isfinite(acts.grad).all())
    return acts.grad.clone(), th.stack(rewards)


def test_adjoint_follows_the_scene_tables():
    """NavigationEnv, requires_grad, 16 recorded steps, (3, 48): equal tables give the shared table's gradients bit for bit; with distinct
    tables the gradient rows of scene s are those of the shared-table env with table s"""
    shared, rs = _grads(3, 48, shared=NAV_TABLE)
    equal, re = _grads(3, 48, scenes=[NAV_TABLE] * 3)
    assert _same(rs, re) and _same(shared, equal)
    bare, _ = _grads(3, 48)
    assert not _same(shared, bare)                           # the obstacle terms carry gradient
    scenes = [NAV_TABLE, NAV_B, NAV_C]
    mixed, rm = _grads(3, 48, scenes=scenes)
    told_apart = False
    for s, tab in enumerate(scenes):
        one, r1 = _grads(3, 48, shared=tab)
        rows = slice(48 * s, 48 * s + 48)
        assert _same(rm[:, rows], r1[:, rows]) and _same(mixed[:, rows], one[:, rows]), s
        told_apart = told_apart or not _same(mixed, one)
    assert told_apart


# ---- (6) ---------------------------------------------------------------------------------------------------------------------------------
def test_persistent_entry_points_refuse_and_trainers_fall_back():
    from visfly_amd.ppo import PPO
    env = _mk(NavigationEnv, 2, 64, scenes=[NAV_TABLE, NAV_B], steps=6, seed=1, random_kwargs=NAV_RK)
    assert env._PERSISTENT is False and type(env)._PERSISTENT is True
    L, st = _lib.lib(), _lib.current_stream(th.device(DEV))
    buf = th.zeros(4096, device=DEV)
    d = buf.data_ptr()
    out = env._out(env._terminal_obs, env._ep_return, env._ep_flags)
    desc, bdesc = _lib.MlpDesc(), _lib.MlpBwdDesc()
    pa = _lib.PpoRolloutArgs()
    for name, kind in pa._fields_:
        setattr(pa, name, d if kind is C.c_void_p else 0)
    pa.T, pa.out = 1, C.addressof(out)
    ea = _lib.EvalRolloutArgs()
    for name, kind in ea._fields_:
        setattr(ea, name, d if kind is C.c_void_p else 0)
    ea.T_max, ea.out = 1, C.addressof(out)
    K = 2
    env.step_n(th.zeros((K, 128, 4), device=DEV))
    calls = {
        "vf_env_rollout_fused": lambda: L.vf_env_rollout_fused(env._h, env._rollouts[K]["ref"], st),
        "vf_ppo_rollout": lambda: L.vf_ppo_rollout(env._h, desc, d, d, pa, st),
        "vf_eval_rollout": lambda: L.vf_eval_rollout(env._h, desc, d, d, ea, st),
        "vf_bptt_rollout": lambda: L.vf_bptt_rollout(env._h, desc, d, d, d, d, d, d, d, out, d, d, 1 << 40, d, d, d, d, 0.99, 1.0, 1, None, None, None, None, None, st),
        "vf_bptt_reverse": lambda: L.vf_bptt_reverse(env._h, bdesc, d, d, d, d, d, 1 << 40, d, d, d, d, d, d, 1, None, None, st),
    }
    for name, call in calls.items():
        assert call() == _lib.EUNSUPPORTED, (name, L.vf_last_error().decode())
        assert name in L.vf_last_error().decode() and "obstacle" in L.vf_last_error().decode()
    with pytest.raises(ValueError, match="obstacles"):
        env.step_n(th.zeros((K, 128, 4), device=DEV), fused=True)
    # a refused table changes nothing; the refusal names the scene and the entry
    from visfly_amd.envs.obstacles import parse_obstacles, scene_tables
    tables, counts = scene_tables([parse_obstacles(NAV_TABLE), parse_obstacles(NAV_B)])
    tables[16].r, tables[16].type = -1.0, _lib.OBST_SPHERE
    assert L.vf_env_set_scene_obstacles(env._h, tables, counts, 2, 64) == -1 and "scene 1: entry 0" in L.vf_last_error().decode()
    assert L.vf_env_set_scene_obstacles(env._h, tables, counts, 2, 63) == -1 and L.vf_env_set_scene_obstacles(env._h, tables, counts, 3, 64) == -1
    counts[0] = 17
    assert L.vf_env_set_scene_obstacles(env._h, tables, counts, 2, 64) == -1 and "scene 0" in L.vf_last_error().decode()
    assert L.vf_env_scene_count(env._h) == 2 and L.vf_env_obstacle_count(env._h) == 2
    env._qcache = None
    cp, win, _, _ = S.scene_query_rows(env.position.cpu().numpy(), np.arange(128), [NAV_TABLE, NAV_B], 64)
    assert _same(env.collision_point.cpu(), th.from_numpy(cp))
    # PPO steps launch by launch
    model = PPO(env, n_steps=8, batch_size=1024, n_epochs=1, seed=3, learning_rate=1e-3, policy_kwargs=dict(activation_fn="relu"))
    model.learn(8 * 128)
    th.cuda.synchronize()
    assert model.fused_rollout is False and bool(th.isfinite(model.policy.flat).all())
    # the two forms replace each other; clearing restores the persistent launches
    env.obstacles = NAV_TABLE
    assert L.vf_env_scene_count(env._h) == 0 and L.vf_env_obstacle_count(env._h) == 2 and env.obstacles == R.parse_obstacles(NAV_TABLE)
    assert env.scene_obstacles == [R.parse_obstacles(NAV_TABLE)] * 2 and env._PERSISTENT is False
    env.scene_obstacles = [NAV_B, []]
    assert L.vf_env_scene_count(env._h) == 2 and L.vf_env_obstacle_count(env._h) == 1 and env._PERSISTENT is False
    env.scene_obstacles = [[], []]
    assert L.vf_env_obstacle_count(env._h) == 0 and env._PERSISTENT is True
    env.scene_obstacles = [NAV_B, []]
    env.obstacles = []
    assert L.vf_env_scene_count(env._h) == 0 and L.vf_env_obstacle_count(env._h) == 0 and env._PERSISTENT is True and env.obstacles == []
    env.scene_obstacles = [NAV_B, []]
    env.scene_obstacles = None
    assert L.vf_env_scene_count(env._h) == 0 and env._PERSISTENT is True
    env.step_begin(th.zeros((128, 4), device=DEV))
    from visfly_amd._lib import VisflyError
    with pytest.raises(VisflyError, match="step_finish"):
        env.scene_obstacles = [NAV_B, []]
    env.step_finish()
