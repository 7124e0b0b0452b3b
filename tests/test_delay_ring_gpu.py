"""The action delay ring at depths other than 0 and the default 3: delay_steps = int(comm_delay / ctrl_dt) of 1, 4 and 5 (and 2, 64, 65
where named) through every path the depth shapes -- the slab layout behind the ring (drag granules at G_RING + D), the launch-uniform
slot index and its per-agent copy, the head the persistent launches advance themselves, the kRingRegs = 4 registers of the
16-agents-per-wave reverse sweep (depth 4 uses the last one, depth 5 takes the replay form), one captured graph per ring phase, the slot
loops of the reset paths, and the limit of 64 slots.

References: the fixtures generated from the reference at these depths (dyn_*_delay*, bptt_*_delay*: oracle/gen_golden.py), the CPU oracle
(its ring Q[D] is general in D; pinned to the reference at these depths by tests/test_oracle_golden.py), the launch-by-launch loop for the
multi-step and persistent launches, and -- a witness that needs neither -- the shifted-action identity: without resets, depth D fed a_t
equals depth 0 fed a_{t-D} (zeros first), bit for bit.  The conditions on the inputs are in tests/test_delay_ring.py."""
import collections

import numpy as np
import pytest
import torch

import oracle
from _golden import ENV_DYN, assert_bits_equal, consts_of, load
from test_delay_ring import GRAD_FIXTURES, applied_to_live

pytestmark = pytest.mark.gpu

COMM_DELAY = {1: 0.02, 2: 0.04, 4: 0.09, 5: 0.1, 64: 1.28, 65: 1.3}      # at ctrl_dt = 0.02 (0.09: the reference's debug scripts' value)
DEPTHS = [1, 4, 5]
NAV_SPAWN = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}}]}}
RAN = collections.Counter()


@pytest.fixture(scope="module", autouse=True)
def cases_per_depth():
    yield
    print("\ntest_delay_ring_gpu: cases run per delay-ring depth: " + ", ".join(f"depth {d}: {n}" for d, n in sorted(RAN.items())))


def dkw(depth, **kw):
    """the env fixtures' dynamics keywords at this depth (counts one case)"""
    RAN[depth] += 1
    return dict(ENV_DYN, comm_delay=COMM_DELAY[depth], **kw)


def make_dynamics(depth, N, **kw):
    from visfly_amd import Dynamics
    dyn = Dynamics(num=N, device="cuda:0", **dkw(depth, **kw))
    assert dyn._comm_delay_steps == depth == int(dyn.constants["delay_steps"])
    return dyn


def ring_of(dyn):
    """(D, 4, N) like the oracle's Q"""
    return dyn.delay_ring.permute(0, 2, 1).contiguous().cpu().numpy()


def hover_actions(rng, N, mode, wide):
    hover = np.array([-1 / 3, 0, 0, 0]) if mode == "bodyrate" else np.full(4, -0.8333)
    return np.clip(hover + rng.uniform(-1, 1, (N, 4)) * wide, -1, 1).astype(np.float32)


def shifted(acts, D):
    """a_{t-D}, zeros for t < D"""
    out = torch.zeros_like(acts)
    out[D:] = acts[:acts.shape[0] - D]
    return out


def assert_not_vacuous(actions, done, D, what):
    """a non-zero action reaches a live agent in at least a quarter of the (step, agent) pairs (the recount of tests/test_delay_ring.py)"""
    hit = applied_to_live(actions.float().cpu().numpy(), done.cpu().numpy(), D)
    print(f"{what}: depth {D}: non-zero action on a live agent in {int(hit.sum())} of {hit.size} (step, agent) pairs")
    assert 4 * int(hit.sum()) >= hit.size, (what, int(hit.sum()), hit.size)


# ---- 3. forward step against the reference and the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth", [("dyn_thrust_delay1", 1), ("dyn_bodyrate_rk4_delay4", 4), ("dyn_bodyrate_delay5", 5)])
def test_dynamics_step_equals_the_reference_fixture(name, depth):
    """the body of test_dyn_gpu.test_golden_bit_exact: state and step() return bit for bit at every checkpoint of the 256 steps"""
    from test_dyn_gpu import test_golden_bit_exact
    RAN[depth] += 1
    assert int(consts_of(load(name))["delay_steps"]) == depth
    test_golden_bit_exact(name)


@pytest.mark.parametrize("mode", ["bodyrate", "thrust"])
@pytest.mark.parametrize("N", [1, 65, 257])
@pytest.mark.parametrize("depth", DEPTHS)
def test_dynamics_step_equals_the_oracle(depth, N, mode):
    dyn = make_dynamics(depth, N, action_type=mode)
    ref = oracle.OracleDynamics(dyn.constants, N)
    rng = np.random.default_rng(100 * depth + N)
    pos = (np.array([1, 0, 1.5]) + rng.uniform(-1, 1, (N, 3))).astype(np.float32)
    vel = rng.uniform(-2, 2, (N, 3)).astype(np.float32)
    dyn.reset(pos=torch.from_numpy(pos), vel=torch.from_numpy(vel))
    ref.reset(pos=pos, vel=vel)
    for k in range(40):
        a = hover_actions(rng, N, mode, 1.0 if k % 2 else 0.1)
        s = dyn.step(torch.from_numpy(a).cuda())
        so = ref.step(a)
        assert_bits_equal(s.cpu().numpy(), so, f"depth {depth} N={N} {mode} step {k}")
        assert_bits_equal(dyn.extend_state.cpu().numpy(), ref.extend_state, f"extend_state @ {k}")
        assert_bits_equal(ring_of(dyn), ref.Q, f"delay ring @ {k}")
    assert np.abs(ref.Q).max(axis=(1, 2)).min() > 0, "every slot holds an action"


@pytest.mark.parametrize("depth", [1, 5])
def test_indexed_reset_zeroes_every_slot(depth):
    N = 300
    dyn = make_dynamics(depth, N)
    ref = oracle.OracleDynamics(dyn.constants, N)
    rng = np.random.default_rng(7)
    phases = set()
    for k in range(30):
        a = rng.uniform(-1, 1, (N, 4)).astype(np.float32)
        dyn.step(torch.from_numpy(a).cuda()); ref.step(a)
        if k % 4 == 3:
            phases.add((k + 1) % depth)
            idx = np.sort(rng.choice(N, size=17, replace=False)).astype(np.int32)
            pos = rng.uniform(0, 2, (17, 3)).astype(np.float32)
            q = rng.normal(size=(17, 4)).astype(np.float32); q /= np.linalg.norm(q, axis=1, keepdims=True)
            tr = rng.uniform(0, 1, 17).astype(np.float32)
            dyn.reset(pos=torch.from_numpy(pos), ori=torch.from_numpy(q), indices=torch.from_numpy(idx), t_rand=torch.from_numpy(tr))
            ref.reset(pos=pos, quat=q, idx=idx, t_rand=tr)
            ring = ring_of(dyn)
            assert ring.shape == (depth, 4, N) and not ring[:, :, idx].any(), "all D rows of a reset agent are zero"
            assert_bits_equal(dyn.extend_state.cpu().numpy(), ref.extend_state, f"after the reset @ {k}")
            assert_bits_equal(ring, ref.Q, f"delay ring after the reset @ {k}")
    assert len(phases) == min(depth, 5), phases
    assert_bits_equal(dyn.extend_state.cpu().numpy(), ref.extend_state, "after indexed resets")
    assert_bits_equal(ring_of(dyn), ref.Q, "delay ring")


def test_depth_64_and_the_limit():
    from visfly_amd import Dynamics
    from visfly_amd._lib import VisflyError
    N, D, steps = 65, 64, 70
    dyn, twin = make_dynamics(D, N), Dynamics(num=N, device="cuda:0", **dict(ENV_DYN, comm_delay=0.0))
    assert twin._comm_delay_steps == 0 and twin.delay_ring is None
    ref = oracle.OracleDynamics(dyn.constants, N)
    rng = np.random.default_rng(64)
    pos = (np.array([1, 0, 1.5]) + rng.uniform(-1, 1, (N, 3))).astype(np.float32)
    for d in (dyn, twin):
        d.reset(pos=torch.from_numpy(pos))
    ref.reset(pos=pos)
    acts = torch.from_numpy(np.stack([hover_actions(rng, N, "bodyrate", 0.3) for _ in range(steps)])).cuda()
    late = shifted(acts, D)
    for k in range(steps):
        s, st = dyn.step(acts[k]), twin.step(late[k])
        so = ref.step(acts[k].cpu().numpy())
        assert_bits_equal(s.cpu().numpy(), so, f"depth 64 vs the oracle @ {k}")
        assert_bits_equal(s.cpu().numpy(), st.cpu().numpy(), f"depth 64 vs depth 0 fed the actions of 64 steps earlier @ {k}")
    assert_bits_equal(dyn.extend_state.cpu().numpy(), ref.extend_state, "extend_state")
    assert_bits_equal(dyn.extend_state.cpu().numpy(), twin.extend_state.cpu().numpy(), "extend_state vs the twin")
    assert_bits_equal(ring_of(dyn), ref.Q, "all 64 slots")
    assert bool(late[D:].any()), "the first actions have left the ring"
    RAN[65] += 1
    with pytest.raises(VisflyError, match="delay_steps"):      # VF_EINVAL from check_dyn_cfg, before any launch
        Dynamics(num=N, device="cuda:0", **dict(ENV_DYN, comm_delay=COMM_DELAY[65]))


@pytest.mark.parametrize("case", ["hover", "nav", "nav_rk4_drag"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_env_step_equals_the_oracle(depth, case):
    import visfly_amd.envs as E
    N, T = 257, 40
    if case == "hover":
        env = E.HoverEnv(num_agent_per_scene=N, seed=9, dynamics_kwargs=dkw(depth), device="cuda:0", max_episode_steps=T, tensor_output=True)
        ref = oracle.OracleEnv(env.envs.dynamics.constants, N, "hover", T)
        hover = [-1 / 3, 0, 0, 0]
    else:
        extra = dict(integrator="rk4", drag_random=0.1) if case == "nav_rk4_drag" else {}
        env = E.NavigationEnv(num_agent_per_scene=N, seed=9, dynamics_kwargs=dkw(depth, **extra), random_kwargs=NAV_SPAWN, device="cuda:0",
                              max_episode_steps=T, tensor_output=True)
        ref = oracle.OracleEnv(env.envs.dynamics.constants, N, "nav", T, target=[9., 0., 1.])
        hover = [-0.3, 0, 0, 0]
    env.reset()
    dyn = env.envs.dynamics
    c = dyn.constants
    assert dyn._comm_delay_steps == depth
    if case == "nav_rk4_drag":      # the coefficients drawn on the device, read from the granules behind the ring (G_RING + D), into the oracle
        kl, kq = dyn.drag_coefficients
        for k, mean in ((kl, c["k_lin"]), (kq, c["k_quad"])):
            f = (k / torch.tensor(mean, device="cuda")).cpu()
            assert (f >= 0.9 - 1e-6).all() and (f <= 1.1 + 1e-6).all() and f.std(dim=0).min() > 0.02
            assert len(torch.unique(f[:, 0])) > N // 2, "the coefficients differ between agents"
        ref.dyn.klin = np.ascontiguousarray(kl.cpu().numpy().T)
        ref.dyn.kquad = np.ascontiguousarray(kq.cpu().numpy().T)
    else:
        assert dyn.drag_coefficients is None
    ref.reset_full_state(env.full_state.cpu().numpy())
    g = torch.Generator().manual_seed(depth)
    for k in range(30):      # < max_episode_steps: no timeout; is_test keeps an agent that collides in step on both sides
        a = ((torch.rand((N, 4), generator=g) * 2 - 1) * 0.5 + torch.tensor(hover)).clamp(-1, 1)
        o, r, d, _ = env.step(a.cuda(), is_test=True)
        ro, rr, rd = ref.step(a.numpy())
        assert_bits_equal(o["state"].cpu().numpy(), ro, f"{case} depth {depth}: observation @ {k}")
        assert_bits_equal(r.cpu().numpy(), rr, f"{case} depth {depth}: reward @ {k}")
        assert np.array_equal(d.cpu().numpy().astype(np.uint8), rd), f"{case} depth {depth}: done @ {k}"
    assert_bits_equal(ring_of(dyn), ref.dyn.Q, "delay ring")
    env.close()


@pytest.mark.parametrize("depth", [1, 5])
def test_straight_line_kernel_equals_the_general_one(depth):
    """tests/test_env_straight_line_gpu.py::_run_pair above the split kernel's agent count; episodes of 2 D + 1 steps, so that actions
    leave the ring between the re-spawns"""
    from test_env_straight_line_gpu import BIG, STEPS, _cls, _run_pair
    RAN[depth] += 1
    n, T = BIG + 65, 2 * depth + 1
    ended = _run_pair(_cls("HoverEnv"), n, max_episode_steps=T, comm_delay=COMM_DELAY[depth])
    assert ended >= (STEPS // T) * n


def test_auto_reset_inside_the_step_zeroes_every_slot():
    """re-spawn inside the step kernel at depth 5: the oracle follows with reset_agents on the GPU's spawn states; a re-spawned agent's
    five slots are zero afterwards, and the slot each of the following five steps consumes still is"""
    import visfly_amd.envs as E
    from visfly_amd import _lib
    N, D, T = 257, 5, 7
    env = E.HoverEnv(num_agent_per_scene=N, seed=9, dynamics_kwargs=dkw(D), device="cuda:0", max_episode_steps=T, tensor_output=True)
    env.reset()
    dyn = env.envs.dynamics
    ref = oracle.OracleEnv(dyn.constants, N, "hover", T)
    ref.reset_full_state(env.full_state.cpu().numpy())
    g = torch.Generator().manual_seed(3)
    since = np.full(N, 1000)                     # steps since the agent's last re-spawn
    ended = checked = 0
    for k in range(30):
        head = int(_lib.lib().vf_env_ring_phase(env._h))
        assert head == k % D
        fresh = since < D
        consumed = ring_of(dyn)[head]            # (4, N): what this step applies
        assert not consumed[:, fresh].any(), f"step {k}: a zero action for the {D} steps after a re-spawn"
        checked += int(fresh.sum())
        a = ((torch.rand((N, 4), generator=g) * 2 - 1) * 0.5 + torch.tensor([-1 / 3, 0, 0, 0])).clamp(-1, 1)
        assert bool((a != 0).all())
        o, r, d, _ = env.step(a.cuda())
        ro, rr, rd = ref.step(a.numpy())
        assert_bits_equal(r.cpu().numpy(), rr, f"reward @ {k}")
        assert np.array_equal(d.cpu().numpy().astype(np.uint8), rd), f"done @ {k}"
        idx = np.flatnonzero(rd).astype(np.int32)
        since += 1
        if len(idx):
            assert_bits_equal(env._terminal_obs.cpu().numpy()[idx], ro[idx], f"terminal rows @ {k}")
            ref.reset_agents(idx, env.full_state.cpu().numpy()[idx])
            ring = ring_of(dyn)
            assert not ring[:, :, idx].any(), f"step {k}: all {D} slots of a re-spawned agent are zero"
            since[idx] = 0
            ended += len(idx)
        assert_bits_equal(o["state"].cpu().numpy(), ref.obs_state, f"observation after the re-spawns @ {k}")
        assert_bits_equal(ring_of(dyn), ref.dyn.Q, f"delay ring @ {k}")
    assert ended >= 4 * N and checked >= 3 * D * N          # (episodes of 7 steps: re-spawns in steps 6, 13, 20, 27)
    env.close()


@pytest.mark.parametrize("what", ["dynamics", "env"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_shifted_action_identity(depth, what):
    import visfly_amd.envs as E
    from visfly_amd import Dynamics
    N, steps = 65, 20
    g = torch.Generator().manual_seed(depth)
    acts = ((torch.rand((steps, N, 4), generator=g) * 2 - 1) * 0.5 + torch.tensor([-1 / 3, 0, 0, 0])).clamp(-1, 1).cuda()
    late = shifted(acts, depth)
    if what == "dynamics":
        a, b = make_dynamics(depth, N), Dynamics(num=N, device="cuda:0", **dict(ENV_DYN, comm_delay=0.0))
        pos = torch.tensor([1, 0, 1.5]) + (torch.rand((N, 3), generator=g) * 2 - 1)
        a.reset(pos=pos), b.reset(pos=pos)
        for k in range(steps):
            assert_bits_equal(a.step(acts[k]).cpu().numpy(), b.step(late[k]).cpu().numpy(), f"depth {depth} vs depth 0 @ {k}")
        assert_bits_equal(a.extend_state.cpu().numpy(), b.extend_state.cpu().numpy(), "extend_state")
        return
    mk = lambda d: E.HoverEnv(num_agent_per_scene=N, seed=4, dynamics_kwargs=d, device="cuda:0", max_episode_steps=1000, tensor_output=True)
    a, b = mk(dkw(depth)), mk(dict(ENV_DYN, comm_delay=0.0))
    a.reset()
    b.reset(state=a.full_state.clone())
    for k in range(steps):
        (oa, ra, da, _), (ob, rb, db, _) = a.step(acts[k], is_test=True), b.step(late[k], is_test=True)
        assert_bits_equal(oa["state"].cpu().numpy(), ob["state"].cpu().numpy(), f"depth {depth} vs depth 0: observation @ {k}")
        assert_bits_equal(ra.cpu().numpy(), rb.cpu().numpy(), f"reward @ {k}")
        assert torch.equal(da, db)
    a.close(), b.close()


# ---- 4. multi-step launches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["step_n", "fused"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_step_n_equals_k_steps(depth, fused):
    from test_env_multistep_gpu import actions, make, same
    N, K, T = 512, 14, 2 * depth + 1
    RAN[depth] += 1
    mk = lambda: make("HoverEnv", N, dyn_extra=dict(comm_delay=COMM_DELAY[depth]), max_episode_steps=T)
    ref, env = mk(), mk()
    assert env.envs.dynamics._comm_delay_steps == depth
    for call in range(2):                          # K % D != 0 for D = 4, 5: the second call starts at another ring phase
        A = actions(N, K, seed=call)
        outs = [ref.step(A[k]) for k in range(K)]
        obs, reward, done = env.step_n(A, fused=fused)
        assert bool(done.any()), "the run must contain re-spawns"
        for k in range(K):
            same(obs[k], outs[k][0]["state"], f"call {call}: obs @ {k}")
            same(reward[k], outs[k][1], f"call {call}: reward @ {k}")
            same(done[k], outs[k][2], f"call {call}: done @ {k}")
        same(env.state_slab, ref.state_slab, f"call {call}: slab")
        if call == 0:
            assert_not_vacuous(A, done, depth, f"step_n(fused={fused})")
    x = actions(N, 1, seed=2)[0]
    same(env.step(x)[0]["state"], ref.step(x)[0]["state"], "step() after the two calls (ring phase, counters)")
    same(env.state_slab, ref.state_slab, "slab")
    same(env._ep_return, ref._ep_return, "episode returns")


@pytest.mark.parametrize("depth,graphs", [(1, 1), (4, 2), (5, 5)])
def test_graph_replay_holds_one_graph_per_ring_phase(depth, graphs):
    from test_env_multistep_gpu import actions, make, same
    from visfly_amd import _lib
    N, K = 512, 6
    RAN[depth] += 1
    mk = lambda: make("HoverEnv", N, dyn_extra=dict(comm_delay=COMM_DELAY[depth]), max_episode_steps=2 * depth + 1)
    ref, env = mk(), mk()
    buf = torch.empty((K, N, 4), device="cuda")
    for rnd in range(5):
        A = actions(N, K, seed=10 + rnd)
        buf.copy_(A)
        outs = [ref.step(A[k]) for k in range(K)]
        obs, reward, done = env.step_n(buf, graph=True)
        for k in range(K):
            same(obs[k], outs[k][0]["state"], f"round {rnd} obs @ {k}")
            same(reward[k], outs[k][1], f"round {rnd} reward @ {k}")
            same(done[k], outs[k][2], f"round {rnd} done @ {k}")
        same(env.state_slab, ref.state_slab, f"round {rnd} slab")
    assert len(env._rollouts[K]["graphs"]) == graphs
    assert sorted(key[2] for key in env._rollouts[K]["graphs"]) == sorted({(K * r) % depth for r in range(5)})
    if depth == 4:      # a graph launched at the wrong phase is refused and leaves the env untouched
        L = _lib.lib()
        phase = int(L.vf_env_ring_phase(env._h))
        assert phase == (5 * K) % depth
        wrong = next(g for key, g in env._rollouts[K]["graphs"].items() if key[2] != phase)
        assert L.vf_env_graph_launch(wrong, _lib.current_stream(env.device)) == -3 and b"phase" in L.vf_last_error()
        same(env.state_slab, ref.state_slab, "a refused replay leaves the env untouched")
    env.close()


# ---- 5. persistent launches against the launch-by-launch loop ---------------------------------------------------------------------------
def bptt_lengths(depth):
    """H, max_episode_steps: max_episode_steps = 2 D + 1, and H % D != 0 where the ring has more than one phase, so that the second
    horizon starts at another one; an episode ends inside each horizon (asserted from the done flags)"""
    H, T = (12 if depth == 5 else 10), 2 * depth + 1
    assert T == 2 * depth + 1 and (depth == 1 or H % depth != 0) and T <= H
    return H, T


def check_bptt_horizons(res, substep, depth, H, what):
    pers = res[0]
    for it in range(2):
        assert bool(pers[f"done{it}"].any()), f"{what}: no episode ended inside horizon {it}"
    assert_not_vacuous(torch.cat([pers["action0"], pers["action1"]]), torch.cat([pers["done0"], pers["done1"]]), depth, what)
    assert float(pers["grad0"].abs().max()) > 0 and float(pers["grad1"].abs().max()) > 0
    # the two sides of kRingRegs = 4: up to four slots the reverse sweep reads the roll-out's sub-step tape and keeps the ring's adjoint in
    # registers; from five on no tape is allocated and the interval is replayed
    if depth <= 4:
        assert substep == [(0, H), (0, H)], substep
    else:
        assert substep == [None, None], substep


@pytest.mark.parametrize("kind,depth", [("hover", 1), ("hover", 4), ("hover", 5), ("hover_thrust", 1), ("hover_thrust", 4), ("hover_thrust", 5),
                                        ("nav_rk4_drag", 4), ("nav_rk4_drag", 5)])
def test_bptt_persistent_launches_equal_the_loop(kind, depth):
    from test_bptt_gpu import check_persistent_rollout_equals_the_per_step_forward
    RAN[depth] += 1
    H, T = bptt_lengths(depth)
    res, substep = check_persistent_rollout_equals_the_per_step_forward(kind, 777, H=H, max_episode_steps=T,
                                                                        dyn=dict(comm_delay=COMM_DELAY[depth]))
    check_bptt_horizons(res, substep, depth, H, f"BPTT {kind}")


@pytest.mark.parametrize("depth", [4, 5])
def test_reference_actor_persistent_launches_equal_the_loop(depth):
    from test_bptt_gpu import check_persistent_launches_with_the_reference_actor_equal_the_loop
    RAN[depth] += 1
    H, T = bptt_lengths(depth)
    res, substep = check_persistent_launches_with_the_reference_actor_equal_the_loop("hover", 777, H=H, max_episode_steps=T,
                                                                                     dyn=dict(comm_delay=COMM_DELAY[depth]))
    check_bptt_horizons(res, substep, depth, H, "two-headed actor, hover")


@pytest.mark.parametrize("env_name,N,dyn,depth", [("HoverEnv", 1000, "euler", 1), ("HoverEnv", 1000, "euler", 4), ("HoverEnv", 1000, "euler", 5),
                                                  ("NavigationEnv", 1000, "rk4_drag", 1), ("NavigationEnv", 1000, "rk4_drag", 4),
                                                  ("NavigationEnv", 1000, "rk4_drag", 5),
                                                  ("HoverEnv", 16401, "euler", 5)])       # (32 rows per wave)
def test_ppo_persistent_rollout_equals_the_loop(env_name, N, dyn, depth):
    from test_ppo_gpu import _persistent_rollout_vs_loop
    RAN[depth] += 1
    n_steps, T = 22, 2 * depth + 1
    assert depth == 1 or n_steps % depth != 0
    res = _persistent_rollout_vs_loop(env_name, N, dyn, max_episode_steps=T, n_steps=n_steps, dyn_extra=dict(comm_delay=COMM_DELAY[depth]))
    pers = res[0]
    # done flags of step t: the episode starts of step t + 1; the two roll-outs are one trajectory (nothing steps the env in between)
    done = torch.cat([torch.cat([pers[f"{r}:episode_starts"][1:].float(), pers[f"{r}:starts"].float().reshape(1, N)]) for r in range(2)]) != 0
    assert bool(done[:n_steps].any()) and bool(done[n_steps:].any()), "an episode ends inside each roll-out"
    assert_not_vacuous(torch.cat([pers["0:actions"], pers["1:actions"]]), done, depth, f"PPO {env_name} {dyn} N={N}")


@pytest.mark.parametrize("depth", [1, 5])
def test_evaluation_persistent_launch_equals_the_loop(depth):
    from test_evaluate_gpu import check_persistent_launch_equals_the_loop, make_env
    from visfly_amd.evaluate import evaluate_policy
    dyn = dkw(depth)
    model, loop = check_persistent_launch_equals_the_loop(f"ppo_relu_hover_48_delay{depth}", "hover", 48, "ppo_relu", -1.0, dyn, False)
    rec = evaluate_policy(model, make_env("hover", 48, seed=11, dyn=dyn), record=True)
    assert torch.equal(rec.ep_length, loop.ep_length)
    assert_not_vacuous(rec.action_all, rec.done_all, depth, "evaluation, hover")


# ---- 6. adjoint ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRAD_FIXTURES))
def test_action_gradients_match_reference_autograd(name):
    """forward bit for bit, gradient within test_bptt_gpu.REL_TOL of max|dL/da| (measured: see the test's output and DESIGN.md)"""
    from test_bptt_gpu import check_action_gradients
    depth = GRAD_FIXTURES[name][0]
    RAN[depth] += 1
    env, fx = check_action_gradients(name)
    assert env.envs.dynamics._comm_delay_steps == depth and len(fx["ev_step"]) > 0


@pytest.mark.parametrize("depth", [1, 5])
def test_dynamics_only_adjoint_equals_the_env_adjoint(depth):
    """the comparison of test_bptt_gpu.test_dynamics_only_adjoint_equals_the_env_adjoint_without_reward: d_action of every step bit for
    bit; the last D steps' actions are still in the ring when the horizon ends and have exactly zero gradient"""
    from visfly_amd import Dynamics
    from visfly_amd.envs import HoverEnv
    N, H = 257, 12
    kw = dkw(depth)
    g = torch.Generator(device="cuda:0").manual_seed(4)
    env = HoverEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(kw), device="cuda:0", tensor_output=True, max_episode_steps=1000,
                   spawn_prefetch=False)
    env.reset()
    fs = env.full_state.clone()
    dyn = Dynamics(num=N, device="cuda:0", **kw)
    dyn.reset(pos=fs[:, 0:3], ori=fs[:, 3:7], vel=fs[:, 7:10], ori_vel=fs[:, 10:13], motor_omega=fs[:, 13:17], thrusts=fs[:, 17:21], t=fs[:, 21])
    acts = (torch.tensor([-1 / 3, 0, 0, 0], device="cuda:0") + (torch.rand((H, N, 4), device="cuda:0", generator=g) * 2 - 1) * 0.3).clamp(-1, 1)
    W = torch.randn((H, N, 13), device="cuda:0", generator=g)
    env.enable_tape(H)
    tapes = []
    for t in range(H):
        tapes.append(dyn._slab.clone())
        s = dyn.step(acts[t])
        o, _, d, _ = env.step(acts[t], is_test=True)
        assert torch.equal(s, o["state"]) and not d.any()
    adj = torch.zeros_like(dyn._slab)
    peak = np.zeros(H)
    for t in reversed(range(H)):
        da_env = env.backward_step(t, d_obs=W[t], d_reward=None)
        da_dyn = dyn.backward_step(tapes[t], acts[t], W[t], adj)
        assert torch.equal(da_env.view(torch.int32), da_dyn.view(torch.int32)), f"step {t}"
        peak[t] = float(da_dyn.abs().max())
    assert (peak[H - depth:] == 0).all(), peak
    assert (peak[:H - depth] > 0).all(), peak
    env.close()
