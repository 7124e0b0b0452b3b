"""Analytic obstacles inside the fused env step (scene_kwargs["obstacles"] / env.obstacles; csrc/vf_env_device.hpp: scene_collision).

(1) the device query equals the host reference tests/_obstacle_ref.py bit for bit; (2) the fused step with a table equals the split step
of a table-less env that is handed the reference's closest point (step_begin -> _obstacle_ref -> step_finish), bit for bit over whole
episodes; (3) step_n, its graph replay, the refusals of the fused / persistent paths and the trainers' launch-by-launch fall-back;
(4) clearing the table returns the env to the behaviour of one that never had it."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

import _obstacle_ref as R
from visfly_amd import _lib
from visfly_amd.envs import HoverEnv, NavigationEnv, NavigationEnv2, RacingEnv2, TrackEnv

DEV = "cuda:0"
KW = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)


def _spawn(mean, half):
    return {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": mean, "half": half}}]}}


BALL = dict(type="sphere", center=[1.0, 0.0, 1.5], radius=0.6)          # the middle of HoverEnv's spawn box (mean [1,0,1.5], half [1,1,.5])
# NavigationEnv spawns on the plane x = 1 (y in [-2, 2], z in [.5, 2.5]) and flies to [9, 0, 1]: a box and a pillar right behind that plane
NAV_RK = _spawn([1., 0., 1.5], [0.0, 2., 1.])
NAV_TABLE = [dict(type="box", lo=[1.3, -2.0, 0.0], hi=[1.8, -1.0, 3.0]), dict(type="pillar", center=[1.5, 2.0], radius=0.2, z=[0.0, 3.0])]
# NavigationEnv2 observes collision_vector, also for an agent that re-spawned in the step -- where the table-less env of the split step
# can only answer with the room box.  Its agents therefore spawn low (z in [.25, .45]: at every spawn point the floor is the closest
# surface, for both envs) under a slab 0.55 m above them, between a wall and a pillar 0.5 m away
NAV2_RK = _spawn([1., 0., 0.35], [1.0, 1.0, 0.1])
NAV2_TABLE = [dict(type="box", lo=[-1.0, -2.0, 1.0], hi=[3.0, 2.0, 1.3]), dict(type="box", lo=[2.5, -3.0, 0.0], hi=[3.0, 3.0, 1.0]),
              dict(type="pillar", center=[-0.7, 0.0], radius=0.2, z=[0.0, 1.0])]
CASES = {"hover": (HoverEnv, {}, [BALL]), "nav": (NavigationEnv, dict(random_kwargs=NAV_RK), NAV_TABLE),
         "nav2": (NavigationEnv2, dict(random_kwargs=NAV2_RK), NAV2_TABLE)}


def _mk(cls, n, table=None, seed=7, steps=48, **kw):
    if table is not None:
        kw["scene_kwargs"] = dict(obstacles=table)
    env = cls(num_agent_per_scene=n, seed=seed, visual=False, dynamics_kwargs=dict(KW), device=DEV, tensor_output=True,
              max_episode_steps=steps, **kw)
    env.reset()
    return env


def _act(n, t, g):
    """the action schedule of tests/test_env_external_scene_gpu.py::test_split_step_equals_fused_step"""
    act = (th.rand((n, 4), device="cuda", generator=g) * 2 - 1) * (1.0 if t % 3 else 0.05) + th.tensor([-1 / 3, 0, 0, 0], device="cuda") * (t % 3 == 0)
    return act.clamp(-1, 1).contiguous()


def _ref(position, table):
    p = position.detach().cpu().numpy()
    cp, g, win = R.scene_query(p, table)
    oob = np.any((p < np.float32(R.ROOM_LO)) | (p > np.float32(R.ROOM_HI)), axis=1)
    return cp, g, win, oob


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 1000])
def test_device_query_equals_host_reference(n):
    """after reset() and after each of 8 steps env.collision_point is the reference's closest point of env.position, bit for bit -- for
    every agent, re-spawned ones included (the query runs on the current position) --, collision_vector / collision_dis / is_collision
    follow from it; one of each primitive plus two more spheres; every primitive and the room box win somewhere, some agent is inside"""
    table = [dict(type="sphere", center=[1.0, 0.0, 1.0], radius=0.5), dict(type="box", lo=[-1.5, -2.0, 0.2], hi=[-1.0, 2.0, 1.8]),
             dict(type="pillar", center=[3.0, 1.0], radius=0.3, z=[0.0, 2.0]), dict(type="sphere", center=[1.0, 2.0, 1.0], radius=0.3),
             dict(type="sphere", center=[1.0, -2.0, 1.2], radius=0.3)]
    env = _mk(HoverEnv, n, table, random_kwargs=_spawn([1., 0., 1.0], [3.0, 3.0, 0.5]))
    assert _lib.lib().vf_env_obstacle_count(env._h) == 5 and env.obstacles == R.parse_obstacles(table)
    g = th.Generator(device="cuda").manual_seed(5)
    winners, inside = set(), 0
    for t in range(9):
        if t:
            env.step(_act(n, t, g))
        cp, gd, win, _ = _ref(env.position, table)
        got = env.collision_point
        assert th.equal(got.cpu(), th.from_numpy(cp)), (t, np.abs(got.cpu().numpy() - cp).max())
        assert th.equal(env.collision_vector, got - env.position)
        dis = env.collision_dis.cpu().numpy()
        assert np.abs(dis - gd).max() <= 4e-7 * max(1.0, gd.max())          # (the FMA-chained norm against the plain one: an ulp or two)
        assert th.equal(env.is_collision, env.collision_dis < 0.1)
        winners |= set(np.unique(win).tolist())
        inside += int(((gd == 0) & (win > 0)).sum())
    assert winners == {0, 1, 2, 3, 4, 5}, winners
    assert inside > 0


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------------
def _fused_vs_split(cls, kw, table, n, steps, collision_reset):
    a = _mk(cls, n, table, is_collision_reset=collision_reset, **kw)
    b = _mk(cls, n, None, is_collision_reset=collision_reset, **kw)
    g = th.Generator(device="cuda").manual_seed(3)
    stat = dict(ended_by_obstacle=0, obstacle_hits=0, near=0, far=0, approach=0, recede=0)
    for t in range(steps):
        act = _act(n, t, g)
        o1, r1, d1, _ = a.step(act)
        pose = b.step_begin(act)
        cp, gd, win, oob = _ref(pose["position"], table)
        o2, r2, d2, _ = b.step_finish(th.from_numpy(cp).to(DEV), th.from_numpy(oob).to(DEV))
        assert th.equal(r1, r2) and th.equal(d1, d2), t
        assert set(o1.keys()) == set(o2.keys())
        for k in o1.keys():
            assert th.equal(o1[k], o2[k]), (t, k)
        for name in ("_ep_return", "_ep_length", "_ep_flags", "_terminal_obs"):          # what the info dicts of the done agents are made of
            assert th.equal(getattr(a, name)[d1], getattr(b, name)[d1]), (t, name)
        alive = ~d1
        assert th.equal(a.is_collision[alive], b.is_collision[alive]), t
        assert th.equal(a.collision_dis[alive], b.collision_dis[alive]), t
        # what happened, from the reference's answer for the pre-reset poses
        vec = cp - pose["position"].cpu().numpy()
        dis = np.sqrt((vec * vec).sum(axis=1))
        hit = (dis < 0.1) & (win > 0)
        done = d1.cpu().numpy()
        stat["obstacle_hits"] += int(hit.sum())
        stat["ended_by_obstacle"] += int((hit & done & ~oob).sum())
        ap = (vec * pose["velocity"].cpu().numpy()).sum(axis=1)
        stat["near"] += int(((win > 0) & (dis < 1)).sum())
        stat["far"] += int(((win > 0) & (dis > 1)).sum())
        stat["approach"] += int(((win > 0) & (ap > 0)).sum())
        stat["recede"] += int(((win > 0) & (ap < 0)).sum())
    assert th.equal(a.state, b.state)
    return stat


@pytest.mark.parametrize("collision_reset", [True, False])
@pytest.mark.parametrize("case", ["hover", "nav", "nav2"])
def test_fused_step_equals_split_step(case, collision_reset):
    """1 000 agents, 120 steps (> 2 episodes of 48).  Not vacuous: where a hit ends an episode (is_collision_reset, or NavigationEnv2's
    failure = is_collision) at least 20 episodes were ended by an obstacle; with is_collision_reset off on the other two envs a hit ends
    nothing, and at least 20 agent-steps in contact with an obstacle are asked instead.  Navigation: obstacle winners on both sides of
    relu(1 - dis) and of the approach relu"""
    cls, kw, table = CASES[case]
    stat = _fused_vs_split(cls, kw, table, 1000, 120, collision_reset)
    print(case, collision_reset, stat)
    if collision_reset or case == "nav2":
        assert stat["ended_by_obstacle"] >= 20, stat
    assert stat["obstacle_hits"] >= 20, stat
    if case == "nav":
        assert min(stat["near"], stat["far"], stat["approach"], stat["recede"]) > 0, stat


def test_fused_step_equals_split_step_above_32768_agents():
    """the dispatch of vf_env_step above 32 768 agents (one thread per agent at every count once a table is set)"""
    stat = _fused_vs_split(HoverEnv, {}, [BALL], 65600, 8, True)
    assert stat["ended_by_obstacle"] >= 20, stat


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------------
def test_step_n_and_its_graph_replay_equal_single_steps():
    n, K = 1000, 5
    envs = [_mk(NavigationEnv, n, NAV_TABLE, random_kwargs=NAV_RK, steps=7) for _ in range(3)]
    plain = _mk(NavigationEnv, n, None, random_kwargs=NAV_RK, steps=7)
    g = th.Generator(device="cuda").manual_seed(11)
    buf = th.empty((K, n, 4), device=DEV)
    differs = False
    for rnd in range(4):                                  # one graph per delay-ring phase (3 slots, K = 5): the fourth round replays the first
        buf.copy_(th.stack([_act(n, rnd * K + k, g) for k in range(K)]))
        want = [envs[0].step(buf[k]) for k in range(K)]
        o1, r1, d1 = (x.clone() for x in envs[1].step_n(buf))
        o2, r2, d2 = envs[2].step_n(buf, graph=True)
        for k in range(K):
            for o, r, d in ((o1, r1, d1), (o2, r2, d2)):
                assert th.equal(o[k], want[k][0]["state"]) and th.equal(r[k], want[k][1]) and th.equal(d[k], want[k][2]), (rnd, k)
        differs = differs or not th.equal(plain.step_n(buf)[1], r1)
    assert th.equal(envs[0].state, envs[1].state) and th.equal(envs[0].state, envs[2].state)
    assert differs                                        # the table was seen: a table-less env earns other rewards
    with pytest.raises(ValueError, match="obstacles"):
        envs[1].step_n(buf, fused=True)
    plain.step_n(buf, fused=True)                         # ... and only the table refuses it


def test_c_entry_points_validate_and_refuse():
    env = _mk(NavigationEnv, 64, NAV_TABLE, random_kwargs=NAV_RK)
    L = _lib.lib()
    from visfly_amd.envs.obstacles import obstacle_table, parse_obstacles
    ok = parse_obstacles([BALL])
    assert L.vf_env_set_obstacles(env._h, obstacle_table(ok * 16), 17) == -1 and L.vf_env_set_obstacles(env._h, obstacle_table(ok), -1) == -1
    for field, value in (("r", 0.0), ("r", float("nan")), ("type", 3)):
        t = obstacle_table(ok)
        setattr(t[0], field, value)
        assert L.vf_env_set_obstacles(env._h, t, 1) == -1, (field, value)
    t = obstacle_table(parse_obstacles([NAV_TABLE[0]]))
    t[0].b[1] = t[0].a[1]                                  # lo == hi in one component
    assert L.vf_env_set_obstacles(env._h, t, 1) == -1
    assert L.vf_env_obstacle_count(env._h) == 2           # a refused table changes nothing
    with pytest.raises(ValueError):
        env.obstacles = [dict(type="sphere", center=[0, 0, 0], radius=-1)]
    assert env.obstacles == parse_obstacles(NAV_TABLE)
    # the K-step kernel is refused by the library itself, whatever the Python layer says
    n, K = 64, 2
    ro = env.step_n(th.zeros((K, n, 4), device=DEV))
    rc = L.vf_env_rollout_fused(env._h, env._rollouts[K]["ref"], _lib.current_stream(th.device(DEV)))
    assert rc == _lib.EUNSUPPORTED and "obstacle" in L.vf_last_error().decode()
    # the table survives a change of the agent offset (the same device block is rewritten)
    assert L.vf_env_set_agent_offset(env._h, 128) == 0 and L.vf_env_obstacle_count(env._h) == 2
    env._qcache = None
    cp, _, win, _ = _ref(env.position, NAV_TABLE)
    assert th.equal(env.collision_point.cpu(), th.from_numpy(cp)) and (win > 0).any()
    del ro


def _nav_ppo(seed_env=1, table=NAV_TABLE):
    from visfly_amd.ppo import PPO
    env = _mk(NavigationEnv, 256, table, seed=seed_env, steps=6, random_kwargs=NAV_RK)
    return PPO(env, n_steps=8, batch_size=2048, n_epochs=1, seed=3, learning_rate=1e-3, policy_kwargs=dict(activation_fn="relu"))


def test_trainers_step_launch_by_launch_and_equal_a_hand_driven_loop():
    """an env with a table has _PERSISTENT False on the instance: rollout_policy / collect_policy / evaluate_policy_launch answer False,
    PPO.learn and evaluate_policy step launch by launch, and what they saw is what a hand-driven loop over an identical env sees"""
    from visfly_amd.evaluate import evaluate_policy
    from visfly_amd.ppo import policy_rows
    model = _nav_ppo()
    env, N = model.env, 256
    assert env._PERSISTENT is False and type(env)._PERSISTENT is True
    f = dict(dtype=th.float32, device=DEV)
    z = th.zeros((8, N, 4), **f)
    assert env.rollout_policy(model.policy, model.obs_keys, z, z.clone(), th.zeros((8, N), **f), th.zeros(N, **f), th.ones(N, **f), 0.99, 1.0 / N) is False
    assert env.collect_policy(model.policy, model.obs_keys, model.buf, None, 0, 0, None) is False
    assert env.evaluate_policy_launch(model.policy, model.obs_keys, {}, None, None, None) is False
    model.learn(8 * N)                                    # one roll-out, one update
    assert model.fused_rollout is False
    th.cuda.synchronize()
    assert bool(th.isfinite(model.policy.flat).all())
    hand, bare = _mk(NavigationEnv, N, NAV_TABLE, seed=1, steps=6, random_kwargs=NAV_RK), _mk(NavigationEnv, N, None, seed=1, steps=6, random_kwargs=NAV_RK)
    obs, differs = hand.reset(), False                  # (the trainer's constructor reset its env once more: the same episode number here)
    bare.reset()
    for t in range(8):
        assert th.equal(model.buf.obs["state"][t], obs["state"]), t
        obs, reward, done, _ = hand.step(model.buf.actions[t])
        if t + 1 < 8:
            assert th.equal(model.buf.episode_starts[t + 1] != 0, done), t
        keep = ~(done & ((hand._ep_flags & 2) != 0))      # (a truncated row also carries the TimeLimit bootstrap)
        assert th.equal(model.buf.rewards[t][keep], reward[keep]), t
        differs = differs or not th.equal(bare.step(model.buf.actions[t])[1], reward)
    assert differs
    # evaluation
    res = evaluate_policy(model, _mk(NavigationEnv, 100, NAV_TABLE, seed=11, steps=6, random_kwargs=NAV_RK), terminal_rows=True)
    assert res.path == "loop"
    ev = _mk(NavigationEnv, 100, NAV_TABLE, seed=11, steps=6, random_kwargs=NAV_RK)
    obs = ev.reset()
    r, l, open_ids = np.zeros(100, np.float32), np.zeros(100, np.int64), set(range(100))
    for t in range(6):
        mean, _ = model.policy.forward(policy_rows(obs, model.obs_keys), save_activations=False)
        a = th.empty((100, 4), device=DEV)
        _lib.check(_lib.lib().vf_eval_action(mean.data_ptr(), a.data_ptr(), 100, _lib.current_stream(th.device(DEV))))
        obs, reward, done, info = ev.step(a, is_test=True)
        for i in np.nonzero(done.cpu().numpy())[0]:
            if i in open_ids:
                open_ids.remove(i)
                r[i], l[i] = info[int(i)]["episode"]["r"], info[int(i)]["episode"]["l"]
    assert not open_ids
    assert np.array_equal(res.ep_return.cpu().numpy().view(np.uint32), r.view(np.uint32)) and np.array_equal(res.ep_length.cpu().numpy(), l)


# ---- (4) and the orthogonal options --------------------------------------------------------------------------------------------------------
def test_clearing_the_table_returns_the_parent_behaviour():
    n = 1000
    a, b = _mk(HoverEnv, n, [BALL]), _mk(HoverEnv, n, None)
    assert a._PERSISTENT is False
    a.obstacles = []
    assert a.obstacles == [] and _lib.lib().vf_env_obstacle_count(a._h) == 0 and a._PERSISTENT is True
    a.reset(), b.reset()
    g = th.Generator(device="cuda").manual_seed(3)
    for t in range(40):
        act = _act(n, t, g)
        o1, r1, d1, _ = a.step(act)
        o2, r2, d2, _ = b.step(act)
        assert th.equal(o1["state"], o2["state"]) and th.equal(r1, r2) and th.equal(d1, d2), t
        assert th.equal(a.collision_point, b.collision_point) and th.equal(a.is_collision, b.is_collision)
    assert th.equal(a.state_slab, b.state_slab)
    b.obstacles = [BALL]                                  # ... and assigning one between steps is seen by the next query and step
    assert not th.equal(b.collision_point, a.collision_point)
    assert not th.equal(b.step(act)[2], a.step(act)[2])   # agents inside the ball end their episode


@pytest.mark.parametrize("which", ["racing2", "track", "imu_wind_offset"])
def test_orthogonal_options_keep_working_with_a_table(which):
    table = [dict(type="sphere", center=[2.0, 1.0, 1.0], radius=1.0), dict(type="pillar", center=[6.0, 0.0], radius=0.5, z=[0.0, 4.0])]
    n = 300
    if which == "racing2":
        env = _mk(RacingEnv2, n, table)
    elif which == "track":
        env = _mk(TrackEnv, n, table)
    else:
        env = HoverEnv(num_agent_per_scene=n, seed=7, dynamics_kwargs=dict(KW, wind_settings=[0.5, -0.25, 0.125]), device=DEV,
                       tensor_output=True, max_episode_steps=48, agent_offset=4096, scene_kwargs=dict(obstacles=[BALL]),
                       random_kwargs=dict(_spawn([1., 0., 1.5], [1., 1., .5]), noise_kwargs={"IMU": {"model": "UniformNoiseModel", "kwargs": {"mean": [0.0] * 13, "half": [0.01] * 13}}}))
        env.reset()
        table = [BALL]
    g = th.Generator(device="cuda").manual_seed(2)
    seen = 0
    for t in range(6):
        obs, reward, done, _ = env.step(_act(n, t, g))
        cp, gd, win, _ = _ref(env.position, table)
        assert th.equal(env.collision_point.cpu(), th.from_numpy(cp)), t
        assert bool(th.isfinite(reward).all()) and bool(th.isfinite(obs["state"]).all())
        seen += int((win > 0).sum())
    assert seen > 0
