"""The device random streams against their host restatement (oracle/vf_oracle.c, pinned to independent definitions by
tests/test_device_streams.py): what spawn="device" envs draw -- spawn states, t, drag coefficients -- bit for bit for every (seed, global
agent id, episode); the Box-Muller rows of vf_noise_fill and of the PPO head against fp64 on the restated uniforms."""
import numpy as np
import pytest
import torch

import oracle
from _golden import ENV_DYN, RACING_DYN, assert_bits_equal
from _streams import UNION, normals_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAV_DYN = dict(ENV_DYN, integrator="rk4", drag_random=0.1)


def _make(name, n, seed, off, dkw=None, **kw):
    """-> env, the boxes its random_kwargs describe (what the oracle is fed), drag_random"""
    import visfly_amd.envs as E
    from visfly_amd.envs import tasks
    from visfly_amd.envs.randomization import spawn_boxes
    rk = tasks._RACING_SPAWN if name == "RacingEnv" else UNION       # RacingEnv always spawns from the reference's own four-box union
    if dkw is None:
        dkw = {"HoverEnv": ENV_DYN, "NavigationEnv": NAV_DYN, "RacingEnv": RACING_DYN}[name]
    env = getattr(E, name)(num_agent_per_scene=n, seed=seed, dynamics_kwargs=dict(dkw), random_kwargs=rk, device=DEV, tensor_output=True,
                           agent_offset=off, **kw)
    boxes = spawn_boxes(rk)
    assert env._boxes == boxes and len(boxes) >= 3
    return env, boxes, float(dkw.get("drag_random", 0))


class _Expect:
    """the state of every row as the restatement alone predicts it across resets: full_state (N,22), drag coefficients, episode counters
    (counted from 1: the first reset() starts episode 1, every re-spawn of a row the next one)"""

    def __init__(self, env, boxes, seed, off, drag):
        self.env, self.boxes, self.seed, self.off, self.drag = env, boxes, seed, off, drag
        self.c = env.envs.dynamics.constants
        n = env.num_agent
        self.ep = np.zeros(n, np.int64)
        self.fs = np.zeros((n, 22), np.float32)
        self.kl, self.kq = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)

    def respawn(self, idx, indexed):
        idx = np.asarray(idx, np.int64).reshape(-1)
        self.ep[idx] += 1
        st, t = oracle.spawn(self.seed, idx, self.ep[idx], self.boxes, indexed, agent0=self.off)
        self.fs[idx] = oracle.spawn_full_state(self.c, st, t)
        if self.drag:
            self.kl[idx], self.kq[idx] = oracle.spawn_drag(self.seed, idx, self.ep[idx], self.drag, self.c["k_lin"], self.c["k_quad"], agent0=self.off)
        return st

    def check(self, what, rows=None):
        """full_state, t and the drag coefficients of `rows` (default: all) on the device == the prediction"""
        env = self.env
        rows = slice(None) if rows is None else rows
        fs = env.full_state.cpu().numpy()
        assert_bits_equal(fs[rows, :13], self.fs[rows, :13], f"{what}: state")
        assert_bits_equal(env.t.cpu().numpy()[rows], self.fs[rows, 21], f"{what}: t")
        assert_bits_equal(fs[rows], self.fs[rows], f"{what}: full_state")
        if self.drag:
            kl, kq = (x.cpu().numpy() for x in env.envs.dynamics.drag_coefficients)
            assert_bits_equal(kl, self.kl, f"{what}: k_lin")        # every row: the rows that did not re-spawn keep theirs
            assert_bits_equal(kq, self.kq, f"{what}: k_quad")


@pytest.mark.parametrize("seed", [3, 2 ** 40 + 7, -1])
@pytest.mark.parametrize("name", ["HoverEnv", "NavigationEnv", "RacingEnv"])
def test_spawn_bit_for_bit(name, seed):
    """reset() (episode 1, t = 0), reset() again (episode 2), reset_agent_by_id on a ragged list (indexed: t drawn, those rows' episode + 1,
    the other rows untouched); seeds with a high key word and one masked to 64 bits; rows keyed by agent_offset + row up to id 2^32 - 1"""
    for n in (1, 63, 65, 1000):
        for off in (None, 0, 2 ** 32 - n):
            env, boxes, drag = _make(name, n, seed, off)
            x = _Expect(env, boxes, seed, off, drag)
            what = f"{name} seed={seed} N={n} offset={off}"
            obs = env.reset()
            st = x.respawn(np.arange(n), False)
            assert_bits_equal(obs["state"].cpu().numpy(), st, f"{what}: observation of reset()")
            x.check(f"{what}: first reset")
            assert not x.fs[:, 21].any()
            env.reset()
            x.respawn(np.arange(n), False)
            x.check(f"{what}: second reset")
            idx = np.random.default_rng(n).permutation(n)[:max(1, n // 3)]         # unsorted, with gaps
            env.reset_agent_by_id(idx.tolist())
            x.respawn(idx, True)
            x.check(f"{what}: indexed reset")
            assert x.fs[idx, 21].max() > 0 and sorted(set(x.ep.tolist())) == ([3] if n == 1 else [2, 3])
            env.close()


@pytest.mark.parametrize("path", ["step", "step_n", "fused"])
@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("name", ["HoverEnv", "NavigationEnv", "RacingEnv"])
def test_auto_reset_spawns_bit_for_bit(name, prefetch, path):
    """max_episode_steps = 3, 10 steps with zero actions: after every step the rows that reported done hold exactly the restatement's spawn
    for (agent, next episode) -- the in-place draw and the prefetched copy, launch by launch and inside the multi-step launches"""
    K = 10
    for n, off, seed in ((65, None, 3), (1000, 2 ** 32 - 1000, 2 ** 40 + 7)):
        env, boxes, drag = _make(name, n, seed, off, max_episode_steps=3, spawn_prefetch=prefetch)
        assert bool(env._ecfg.spawn_prefetch) == prefetch
        x = _Expect(env, boxes, seed, off, drag)
        what = f"{name} prefetch={prefetch} {path} N={n}"
        env.reset()
        x.respawn(np.arange(n), False)
        acts = torch.zeros((K, n, 4), device=DEV)
        ended = 0
        if path == "step":
            for k in range(K):
                o, _, d, _ = env.step(acts[k])
                idx = np.nonzero(d.cpu().numpy())[0]
                st = x.respawn(idx, True)
                assert_bits_equal(o["state"].cpu().numpy()[idx], st, f"{what}: returned rows of the re-spawned agents @ {k}")
                x.check(f"{what} @ {k}", rows=idx)
                ended += len(idx)
        else:
            obs, _, done = env.step_n(acts, fused=path == "fused")
            obs, done = obs.cpu().numpy(), done.cpu().numpy().astype(bool)
            for k in range(K):
                idx = np.nonzero(done[k])[0]
                st = x.respawn(idx, True)
                assert_bits_equal(obs[k][idx], st, f"{what}: rows of the re-spawned agents @ {k}")
                ended += len(idx)
            x.check(f"{what}: the rows that re-spawned in the last step", rows=np.nonzero(done[K - 1])[0])
        assert ended >= 3 * n and x.ep.min() >= 4, (ended, x.ep.min())
        env.close()


@pytest.mark.parametrize("r", [0.1, 0.6])
def test_drag_redraw_bit_for_bit(r):
    """NavigationEnv, RK4, drag_random 0.1 and 0.6 (the clamp to [0.5, 1.5] fires on both sides): the per-agent coefficients after reset() and
    after every auto-reset"""
    n, seed, off = 1000, 2 ** 40 + 7, 2 ** 32 - 1000
    env, boxes, drag = _make("NavigationEnv", n, seed, off, dkw=dict(NAV_DYN, drag_random=r), max_episode_steps=3)
    assert drag == r
    x = _Expect(env, boxes, seed, off, drag)
    env.reset()
    x.respawn(np.arange(n), False)
    x.check(f"drag_random={r}: reset")
    zero = torch.zeros((n, 4), device=DEV)
    for k in range(10):
        _, _, d, _ = env.step(zero)
        idx = np.nonzero(d.cpu().numpy())[0]
        x.respawn(idx, True)
        x.check(f"drag_random={r} @ {k}", rows=idx)
    assert x.ep.min() >= 4
    ml, mq = np.asarray(x.c["k_lin"], np.float32).reshape(1, 3), np.asarray(x.c["k_quad"], np.float32).reshape(1, 3)
    if r > 0.5:
        for k, m in ((x.kl, ml), (x.kq, mq)):
            assert (k == m * np.float32(0.5)).any() and (k == m * np.float32(1.5)).any()
    else:
        f = np.concatenate([x.kl.astype(np.float64) / ml, x.kq.astype(np.float64) / mq])
        assert f.min() >= 0.9 - 1e-6 and f.max() <= 1.1 + 1e-6 and f.min() < 0.91 and f.max() > 1.09
    env.close()


def test_env_run_never_reads_a_draw_back():
    """NavigationEnv, 777 agents, RK4 + drag randomisation, max_episode_steps = 6, 40 steps of random actions: the oracle env takes its initial
    state, every re-spawn and every drag redraw from the restatement alone; reward, done and the observation of EVERY row, re-spawned rows
    included, are bit-identical at every step, extend_state at the end"""
    N, T, seed = 777, 6, 23
    env, boxes, drag = _make("NavigationEnv", N, seed, None, max_episode_steps=T)
    x = _Expect(env, boxes, seed, None, drag)
    c = env.envs.dynamics.constants
    ref = oracle.OracleEnv(c, N, "nav", T, target=[9., 0., 1.])
    st = x.respawn(np.arange(N), False)
    ref.dyn.klin, ref.dyn.kquad = np.ascontiguousarray(x.kl.T), np.ascontiguousarray(x.kq.T)
    ref.reset_full_state(x.fs)
    assert_bits_equal(env.reset()["state"].cpu().numpy(), st, "reset")
    g = torch.Generator().manual_seed(5)
    ended = 0
    for k in range(40):
        a = ((torch.rand((N, 4), generator=g) * 2 - 1) * 0.6 + torch.tensor([-0.3, 0, 0, 0])).clamp(-1, 1)
        o, r, d, _ = env.step(a.to(DEV))
        ro, rr, rd = ref.step(a.numpy())
        assert_bits_equal(r.cpu().numpy(), rr, f"reward @ {k}")
        assert np.array_equal(d.cpu().numpy().astype(np.uint8), rd), f"done @ {k}"
        idx = np.nonzero(rd)[0]
        if len(idx):
            ended += len(idx)
            ro[idx] = x.respawn(idx, True)
            ref.dyn.klin[:, idx], ref.dyn.kquad[:, idx] = x.kl[idx].T, x.kq[idx].T
            ref.reset_agents(idx, x.fs[idx])
        assert_bits_equal(o["state"].cpu().numpy(), ro, f"observation of every row @ {k}")
    assert ended >= 5 * N, ended
    assert_bits_equal(env.extend_state.cpu().numpy(), ref.dyn.extend_state, "extend_state after 40 steps")
    env.close()


# ---- the per-row normal streams ------------------------------------------------------------------------------------------------
SEED, ROW0, STEP0 = 2 ** 33 + 5, 12345, 2 ** 32 - 2            # the steps cross the 32-bit word of the counter
ULP = 2.0 ** -24
_noise = {}


def _fill(T, n, row0, seed, step0):
    from visfly_amd import _lib
    eps = torch.full((T, n, 4), float("nan"), device=DEV)
    _lib.check(_lib.lib().vf_noise_fill(eps.data_ptr(), T, n, row0, seed, step0, _lib.current_stream(eps.device)))
    torch.cuda.synchronize()
    return eps


def _noise_rows():
    """(device rows (4, 2^18, 4), restated uniforms of the same blocks), computed once"""
    if not _noise:
        T, n = 4, 2 ** 18
        rows = np.arange(ROW0, ROW0 + n)
        _noise["eps"] = _fill(T, n, ROW0, SEED, STEP0)
        _noise["u"] = np.stack([oracle.noise_uniforms(rows, STEP0 + t, oracle.TAG_ROW_NOISE, SEED) for t in range(T)])
    return _noise["eps"], _noise["u"]


def test_noise_rows_against_fp64_box_muller():
    """2^22 normals of vf_noise_fill against sqrt(-2 ln u1) (cos | sin)(fp32(fp32(2 pi) u2)) in fp64 on the restated uniforms:
    |e - ref| <= 8 * 2^-24 * sqrt(-2 ln u1).  The device maths library documents the OpenCL-profile limits log 3 ulp, sin / cos 4 ulp, and
    the multiply and sqrt are correctly rounded (1/2 ulp each): 3 ulp of ln u1 become 1.5 ulp of the radius through the square root, + 1/2
    (the multiply by -2 is exact) + 1/2 (sqrt) = 2.5, + 4 (sin / cos, at most 1 in magnitude) + 1/2 (the product) = 6.5 ulp of the radius.
    Measured on an MI355X: max|e - ref| = 5.49e-7 = 3.17 ulp of the radius over the 2^22 samples; two radii come from u1 <= 2^-20 (the largest
    radius is 5.42)."""
    eps, u = _noise_rows()
    got = eps.cpu().numpy().astype(np.float64).reshape(-1, 4)
    u = u.reshape(-1, 4)
    ref, radius = normals_fp64(u)
    assert np.isfinite(got).all()
    tail = int((u[:, [0, 2]] <= 2.0 ** -20).sum())
    err = np.abs(got - ref)
    ulps = err / (ULP * np.maximum(radius, 1e-300))
    print(f"noise rows: max|e - fp64| = {err.max():.3e} = {ulps.max():.3f} ulp of the radius over {got.size} samples; "
          f"{tail} radii from u1 <= 2^-20 (largest radius {radius.max():.3f})")
    assert tail >= 1, "the sample was meant to reach the tail"
    assert (err <= 8 * ULP * radius).all(), (err.max(), ulps.max())


def test_noise_row_with_u1_equal_one_is_exactly_zero():
    """block {165461, 0, 0, 0xb977} under this seed has a first word of 0xffffff..: u1 = 1, ln u1 = 0, both normals of the pair are 0"""
    assert oracle.noise_uniforms([165461], 0, oracle.TAG_ROW_NOISE, SEED)[0, 0] == 1.0
    e = _fill(1, 1, 165461, SEED, 0).cpu().numpy().reshape(4)
    assert e[0] == 0.0 and e[1] == 0.0 and e[2] != 0.0 and np.isfinite(e).all()


def test_noise_windows_equal_the_whole():
    """row0 + i keys the row, step0 + t the step: windows of the population and of the steps are the same bits"""
    eps, _ = _noise_rows()
    for r, n in ((63, 130), (2 ** 18 - 1, 1), (1000, 4097)):
        assert torch.equal(_fill(4, n, ROW0 + r, SEED, STEP0), eps[:, r:r + n]), (r, n)
    assert torch.equal(_fill(2, 5000, ROW0, SEED, STEP0 + 1)[:, :], eps[1:3, :5000])


def test_ppo_head_stream_against_fp64():
    """vf_head_sample_at with mean = 0, log_std = 0: action = tanh(eps), eps the Box-Muller pair of block {row0 + i, step, 0xac7}:
    |action - tanh(ref)| <= (1 - a^2) * 8 * 2^-24 * radius + 4 * 2^-24 (the bound of the noise rows through tanh's derivative, + tanhf's own
    error).  The same rows under the noise rows' tag 0xb977 miss that bound on > 95 % of the rows: the two streams are distinct.
    Measured on an MI355X: max|action - tanh(ref)| = 1.18e-7 = 1.98 * 2^-24."""
    from visfly_amd import _lib
    M, row0, step = 4096, 192, 2 ** 32 - 1
    mean, ls = torch.zeros(M, 4, device=DEV), torch.zeros(4, device=DEV)
    act, lp = torch.full((M, 4), float("nan"), device=DEV), torch.empty(M, device=DEV)
    _lib.check(_lib.lib().vf_head_sample_at(mean.data_ptr(), ls.data_ptr(), act.data_ptr(), lp.data_ptr(), M, row0, SEED, step, 0,
                                            _lib.current_stream(act.device)))
    torch.cuda.synchronize()
    got = act.cpu().numpy().astype(np.float64)
    rows = np.arange(row0, row0 + M)

    def miss(tag):
        ref, radius = normals_fp64(oracle.noise_uniforms(rows, step, tag, SEED))
        a = np.tanh(ref)
        err = np.abs(got - a)
        return err, err > (1 - a * a) * 8 * ULP * radius + 4 * ULP

    err, bad = miss(oracle.TAG_PPO_NOISE)
    print(f"ppo head: max|action - tanh(fp64 eps)| = {err.max():.3e} = {err.max() / ULP:.3f} * 2^-24")
    assert not bad.any(), err.max()
    _, other = miss(oracle.TAG_ROW_NOISE)
    assert other.any(axis=1).mean() > 0.95
