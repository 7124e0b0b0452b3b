"""Collision-free spawns (scene_kwargs["safe_spawn"] / env.safe_spawn; vf_env_set_safe_spawn; spawn_agent_safe) against the host
restatement tests/_scene_ref.py::safe_spawn_ref, bit for bit: (7) vf_env_reset drawing on the device, shared and per-scene tables, a Union
of two spawn boxes, the crafted trap whose 16th candidate is kept; (8) the re-spawn inside the step, drawn in place or prefetched by the
helper blocks; (9) off means off."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

import _scene_ref as S
from visfly_amd import _lib
from visfly_amd.envs import HoverEnv, NavigationEnv

DEV = "cuda:0"
KW = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)
CASES = {"shared": (1, S.N_SAFE, [S.SAFE_SHARED]), "3x48": (3, 48, S.SAFE_SCENES)}


def _mk(ns, aps, tables, safe, rk=S.SAFE_RK, cls=HoverEnv, steps=48, **kw):
    sk = {}
    if tables is not None:
        sk = dict(obstacles=tables[0]) if len(tables) == 1 and ns == 1 else dict(scene_obstacles=tables)
    if safe is not None:
        sk["safe_spawn"] = safe
    return cls(num_agent_per_scene=aps, num_scene=ns, seed=S.SEED, visual=False, dynamics_kwargs=dict(KW), device=DEV, tensor_output=True,
               max_episode_steps=steps, random_kwargs=rk, scene_kwargs=sk, **kw)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_rows(env, rows, state, t, what):
    fs = env.full_state.cpu().numpy()
    assert np.array_equal(_bits(fs[rows, :13]), _bits(state)), (what, np.abs(fs[rows, :13] - state).max())
    assert np.array_equal(_bits(fs[rows, 21]), _bits(t)), what


def _act(n, t, g):
    act = (th.rand((n, 4), device="cuda", generator=g) * 2 - 1) * (1.0 if t % 3 else 0.05) + th.tensor([-1 / 3, 0, 0, 0], device="cuda") * (t % 3 == 0)
    return act.clamp(-1, 1).contiguous()


# ---- (7) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_reset_draws_the_accepted_state(case):
    ns, aps, tables = CASES[case]
    n, boxes = ns * aps, S.boxes_of(S.SAFE_RK)
    off, on = _mk(ns, aps, tables, None), _mk(ns, aps, tables, True)
    assert off.safe_spawn == 0.0 and on.safe_spawn == float(np.float32(S.UAV_RADIUS))
    redrawn = 0
    for ep in (1, 2):                                         # every full reset starts the next episode
        off.reset(), on.reset()
        st, t, att, exhausted = S.safe_spawn_ref(S.SEED, np.arange(n), ep, boxes, tables, aps, S.UAV_RADIUS, False)
        assert not exhausted.any()
        _assert_rows(on, np.arange(n), st, t, ("on", ep))
        st0, t0 = S.spawn_attempt(S.SEED, np.arange(n), ep, boxes, 0, False)
        _assert_rows(off, np.arange(n), st0, t0, ("off", ep))
        assert int(off.is_collision.sum()) >= 1 and int(on.is_collision.sum()) == 0
        assert th.equal(off.is_collision.cpu(), th.from_numpy(att > 0))          # the agents in collision are the ones that get re-drawn
        redrawn += int((att > 0).sum())
    assert redrawn >= 2
    # an indexed reset draws t as well; a host-replayed state is never re-drawn
    idx = np.arange(5, n, 7)
    on.reset_agent_by_id(th.from_numpy(idx))
    st, t, _, _ = S.safe_spawn_ref(S.SEED, idx, 3, boxes, tables, aps, S.UAV_RADIUS, True)
    _assert_rows(on, idx, st, t, "indexed")
    fs = on.full_state.cpu().clone()
    fs[:, :3] = th.tensor(tables[0][0]["center"] if "center" in tables[0][0] else [1.0, 0.0, 1.5])
    on.reset(state=fs)
    assert th.equal(on.position.cpu(), fs[:, :3]) and int(on.is_collision[:aps].sum()) == aps


def test_trap_keeps_the_sixteenth_candidate():
    """the spawn box lies wholly inside a box solid: every candidate is rejected, the call returns with attempt 15's state"""
    env = _mk(1, S.N_SAFE, [S.TRAP], True, rk=S.TRAP_RK)
    env.reset()
    st, t = S.spawn_attempt(S.SEED, np.arange(S.N_SAFE), 1, S.boxes_of(S.TRAP_RK), S.SPAWN_TRIES - 1, False)
    _assert_rows(env, np.arange(S.N_SAFE), st, t, "trap")
    assert bool(env.is_collision.all())
    env.step(th.zeros((S.N_SAFE, 4), device=DEV))             # every agent ends its episode at once and is re-drawn 16 times again
    st, t = S.spawn_attempt(S.SEED, np.arange(S.N_SAFE), 2, S.boxes_of(S.TRAP_RK), S.SPAWN_TRIES - 1, True)
    _assert_rows(env, np.arange(S.N_SAFE), st, t, "trap, in the step")


# ---- (8) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_respawns_inside_the_step(case):
    """is_collision_reset, 120 steps of 48-step episodes: every re-spawned state is the host restatement's for (agent, episode), no agent
    that re-spawned in a step has is_collision set after it; drawn in place and prefetched by the helper blocks give the same bits"""
    ns, aps, tables = CASES[case]
    n, boxes = ns * aps, S.boxes_of(S.SAFE_RK)
    envs = [_mk(ns, aps, tables, True, is_collision_reset=True, spawn_prefetch=p) for p in (True, False)]
    for e in envs:
        e.reset()
    g = th.Generator(device="cuda").manual_seed(3)
    ep = np.ones(n, np.int64)
    respawned = redrawn = 0
    for t in range(120):
        act = _act(n, t, g)
        outs = [e.step(act) for e in envs]
        done = outs[0][2].cpu().numpy()
        assert th.equal(outs[0][2], outs[1][2]) and th.equal(outs[0][1].view(th.int32), outs[1][1].view(th.int32)), t
        assert th.equal(envs[0].full_state.view(th.int32), envs[1].full_state.view(th.int32)), t
        rows = np.nonzero(done)[0]
        if len(rows):
            ep[rows] += 1
            st, tt, att, exhausted = S.safe_spawn_ref(S.SEED, rows, ep[rows], boxes, tables, aps, S.UAV_RADIUS, True)
            assert not exhausted.any()
            for e in envs:
                _assert_rows(e, rows, st, tt, t)
                assert int(e.is_collision[outs[0][2]].sum()) == 0, t
            respawned += len(rows)
            redrawn += int((att > 0).sum())
    print(case, dict(respawned=respawned, redrawn=redrawn))
    assert respawned > n and redrawn >= 10


# ---- (9) ---------------------------------------------------------------------------------------------------------------------------------
BALL = dict(type="sphere", center=[1.0, 0.0, 1.5], radius=0.6)
NAV_RK = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0.0, 2., 1.]}}]}}
NAV_TABLE = [dict(type="box", lo=[0.8, -2.0, 0.0], hi=[1.8, -1.0, 3.0]), dict(type="pillar", center=[1.1, 2.0], radius=0.3, z=[0.0, 3.0])]


def _trajectory(env, steps=120):
    n = env.num_agent
    env.reset()
    g = th.Generator(device="cuda").manual_seed(3)
    rec = []
    for t in range(steps):
        o, r, d, _ = env.step(_act(n, t, g))
        rec.append(th.cat([o["state"], r[:, None], d[:, None].float()], 1))
    return th.stack(rec).view(th.int32), env.state_slab.clone().view(th.int32)


@pytest.mark.parametrize("task", ["hover", "nav"])
def test_off_means_off(task):
    """safe_spawn unset, set to 0, or set without any table: the 120-step trajectories (192 agents, re-spawns included) are unchanged to the
    bit; set with a table they are not"""
    cls, rk, table = (HoverEnv, None, [BALL]) if task == "hover" else (NavigationEnv, NAV_RK, NAV_TABLE)
    mk = lambda tables, safe: _mk(3, 64, tables, safe, rk=rk, cls=cls, is_collision_reset=True)
    want, want_slab = _trajectory(mk([table] * 3, None))
    for safe in (0, 0.0, False):
        got, slab = _trajectory(mk([table] * 3, safe))
        assert th.equal(got, want) and th.equal(slab, want_slab), safe
    env = mk([table] * 3, True)
    env.safe_spawn = 0                                        # ... switched off again before the first reset
    got, slab = _trajectory(env)
    assert th.equal(got, want) and th.equal(slab, want_slab)
    bare, bare_slab = _trajectory(mk(None, None))
    env = mk(None, True)
    assert env.safe_spawn > 0 and _lib.lib().vf_env_obstacle_count(env._h) == 0
    got, slab = _trajectory(env)
    assert th.equal(got, bare) and th.equal(slab, bare_slab)
    on, _ = _trajectory(mk([table] * 3, True))
    assert not th.equal(on, want)
