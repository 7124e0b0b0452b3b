"""Global agent ids (agent_offset): a contiguous shard of a population draws -- spawns, drag randomisation, exploration noise -- what
the matching rows of ONE env over the whole population draw with the same seed.  N = 512 split as 256 + 256 and as 192 + 320 (not
wave-aligned on purpose)."""
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 512
SPLITS = [(256, 256), (192, 320)]
NAV_SPAWN = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}}]}}


def _env(name, n, off, prefetch=None, seed=5, max_episode_steps=9, **kw):
    import visfly_amd.envs as E
    from _golden import ENV_DYN
    if name == "NavigationEnv":     # RK4 + per-agent drag re-drawn at every (re)spawn
        kw.setdefault("random_kwargs", NAV_SPAWN)
        dkw = dict(ENV_DYN, integrator="rk4", drag_random=0.5)
    else:
        dkw = dict(ENV_DYN)
    return getattr(E, name)(num_agent_per_scene=n, seed=seed, dynamics_kwargs=dkw, device=DEV, max_episode_steps=max_episode_steps,
                            tensor_output=True, spawn_prefetch=prefetch, agent_offset=off, **kw)


def _shards(split):
    out, a = [], 0
    for c in split:
        out.append((a, a + c))
        a += c
    assert a == N
    return out


def _obs_equal(full, part, a, b, what):
    if isinstance(full, dict):
        assert sorted(full.keys()) == sorted(part.keys())
        for k in full.keys():
            assert torch.equal(part[k], full[k][..., a:b, :] if full[k].dim() > 1 else full[k][a:b]), f"{what}: obs[{k}] rows [{a}, {b})"
    else:
        assert torch.equal(part, full[..., a:b, :]), f"{what}: obs rows [{a}, {b})"


def _actions(K, seed=11):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand((K, N, 4), device=DEV, generator=g) * 2 - 1


RESET_IDS = [5, 100, 191, 192, 255, 256, 300, 511]     # global agents of the mid-run indexed reset


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("name", ["HoverEnv", "NavigationEnv"])
def test_env_step_rows_of_a_shard_equal_the_whole_population(name, prefetch):
    """obs / reward / done / episode outputs of every step() over 64 steps with ~7 re-spawns per agent and an indexed reset in the middle"""
    K = 64
    acts = _actions(K)
    for split in SPLITS:
        full = _env(name, N, 0, prefetch)
        parts = [(a, b, _env(name, b - a, a, prefetch)) for a, b in _shards(split)]
        o_full = full.reset()
        for a, b, e in parts:
            assert e.agent_offset == a
            _obs_equal(o_full, e.reset(), a, b, f"{split} reset")
        n_done = 0
        for k in range(K):
            if k == 20:
                o_full = full.reset_agent_by_id(agent_indices=RESET_IDS)
                for a, b, e in parts:
                    _obs_equal(o_full, e.reset_agent_by_id(agent_indices=[i - a for i in RESET_IDS if a <= i < b]), a, b, f"{split} indexed reset")
            of, rf, df, info_f = full.step(acts[k])
            n_done += int(df.sum())
            for a, b, e in parts:
                o, r, d, info = e.step(acts[k, a:b].contiguous())
                what = f"{name} prefetch={prefetch} split={split} step {k}"
                _obs_equal(of, o, a, b, what)
                assert torch.equal(r, rf[a:b]) and torch.equal(d, df[a:b]), what
                m = d.bool()
                assert torch.equal(e._ep_return[m], full._ep_return[a:b][m]) and torch.equal(e._ep_length[m], full._ep_length[a:b][m]), what
                assert torch.equal(e._ep_flags[m], full._ep_flags[a:b][m]) and torch.equal(e._terminal_obs[m], full._terminal_obs[a:b][m]), what
                if k in (8, 40):          # the info dicts themselves, where episodes just ended
                    for i in torch.nonzero(m).flatten().tolist()[:8]:
                        x, y = info[i], info_f[a + i]
                        assert x["episode"]["r"] == y["episode"]["r"] and x["episode"]["l"] == y["episode"]["l"]
                        assert x["TimeLimit.truncated"] == y["TimeLimit.truncated"] and x["is_success"] == y["is_success"]
                        assert torch.equal(torch.as_tensor(x["terminal_observation"]["state"]), torch.as_tensor(y["terminal_observation"]["state"]))
        assert n_done >= 5 * N, "every agent was meant to re-spawn several times"
        for e in [full] + [p[2] for p in parts]:
            e.close()


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("name", ["HoverEnv", "NavigationEnv"])
def test_env_fused_multi_step_rows_of_a_shard_equal_the_whole_population(name, prefetch):
    """the same through step_n(fused=True): the 64 steps inside one launch"""
    K = 64
    acts = _actions(K, seed=12)
    full = _env(name, N, 0, prefetch)
    full.reset()
    of, rf, df = [x.clone() if not isinstance(x, dict) else {k: v.clone() for k, v in x.items()} for x in full.step_n(acts, fused=True)]
    assert int(df.sum()) >= 5 * N
    for split in SPLITS:
        for a, b in _shards(split):
            e = _env(name, b - a, a, prefetch)
            e.reset()
            o, r, d = e.step_n(acts[:, a:b].contiguous(), fused=True)
            _obs_equal(of, o, a, b, f"{name} fused split={split}")
            assert torch.equal(r, rf[:, a:b]) and torch.equal(d, df[:, a:b])
            e.close()
    full.close()


def test_offset_moves_the_stream_and_none_equals_zero():
    """not vacuous: row 0 of an env at offset 256 spawns where row 256 of the offset-0 env spawns, not where its row 0 does; the legacy
    path (None) and offset 0 are the same bits"""
    full, legacy, shifted = _env("HoverEnv", N, 0), _env("HoverEnv", N, None), _env("HoverEnv", 256, 256)
    assert legacy.agent_offset is None and full.agent_offset == 0 and shifted.agent_offset == 256
    from visfly_amd import _lib
    assert _lib.lib().vf_env_agent_offset(legacy._h) == 0 and _lib.lib().vf_env_agent_offset(shifted._h) == 256
    s0, sl, ss = full.reset()["state"], legacy.reset()["state"], shifted.reset()["state"]
    assert torch.equal(s0, sl)
    assert torch.equal(ss[0], s0[256]) and not torch.equal(ss[0], s0[0])
    acts = _actions(24, seed=13)
    for k in range(24):
        a, b = full.step(acts[k]), legacy.step(acts[k])
        assert torch.equal(a[0]["state"], b[0]["state"]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for e in (full, legacy, shifted):
        e.close()


def test_offsets_that_do_not_fit_are_refused():
    import visfly_amd.envs as E
    from visfly_amd import _lib
    with pytest.raises(ValueError):
        _env("HoverEnv", 64, -1)
    with pytest.raises(ValueError):
        _env("HoverEnv", 64, 2 ** 32 - 63)
    with pytest.raises(ValueError):
        E.HoverEnv(num_agent_per_scene=64, device=DEV, spawn="replay", agent_offset=0)
    with pytest.raises(ValueError):
        _env("HoverEnv", 64, 1.5)
    top = _env("HoverEnv", 64, 2 ** 32 - 64)         # the last ids the 32-bit counter word holds
    assert top.agent_offset == 2 ** 32 - 64
    L = _lib.lib()                                      # ... and the C entry point itself
    assert L.vf_env_set_agent_offset(top._h, -1) == -1 and L.vf_env_set_agent_offset(top._h, 2 ** 32 - 63) == -1
    assert L.vf_env_set_agent_offset(None, 0) == -1
    assert L.vf_env_agent_offset(top._h) == 2 ** 32 - 64
    top.close()


# ---- vf_noise_fill ---------------------------------------------------------------------------------------------------------
def _fill(T, n, row0, seed, step0):
    from visfly_amd import _lib
    eps = torch.full((T, n, 4), float("nan"), device=DEV)
    _lib.check(_lib.lib().vf_noise_fill(eps.data_ptr(), T, n, row0, seed, step0, _lib.current_stream(eps.device)))
    torch.cuda.synchronize()
    return eps


def test_noise_fill_is_a_function_of_global_row_step_and_seed():
    from visfly_amd import _lib
    big = _fill(5, 1000, 0, 77, 40)
    assert torch.isfinite(big).all()
    for row0, n in ((0, 1000), (192, 320), (999, 1), (63, 130)):
        assert torch.equal(_fill(5, n, row0, 77, 40), big[:, row0:row0 + n]), (row0, n)
    assert torch.equal(_fill(2, 1000, 0, 77, 42), big[2:4])                  # step0 + t is the step
    assert not torch.equal(_fill(5, 1000, 0, 77, 45), big) and not torch.equal(_fill(5, 1000, 0, 78, 40), big)
    assert (_fill(1, 1000, 0, 77, 41)[0] != big[0]).float().mean() > 0.99
    # the PPO head's stream (same key, row and step; its own domain tag): action = tanh(0 + exp(0) * eps)
    L = _lib.lib()
    mean, ls, act, lp = torch.zeros(1000, 4, device=DEV), torch.zeros(4, device=DEV), torch.empty(1000, 4, device=DEV), torch.empty(1000, device=DEV)
    _lib.check(L.vf_head_sample_at(mean.data_ptr(), ls.data_ptr(), act.data_ptr(), lp.data_ptr(), 1000, 0, 77, 40, 0, _lib.current_stream(act.device)))
    torch.cuda.synchronize()
    assert ((act - torch.tanh(big[0])).abs() > 1e-3).float().mean() > 0.95
    # vf_head_sample_at: rows of a window == rows of the whole; vf_head_sample == row0 0
    mean = torch.randn(1000, 4, device=DEV)
    a0, l0 = torch.empty(1000, 4, device=DEV), torch.empty(1000, device=DEV)
    _lib.check(L.vf_head_sample(mean.data_ptr(), ls.data_ptr(), a0.data_ptr(), l0.data_ptr(), 1000, 77, 40, 0, _lib.current_stream(act.device)))
    _lib.check(L.vf_head_sample_at(mean.data_ptr(), ls.data_ptr(), act.data_ptr(), lp.data_ptr(), 1000, 0, 77, 40, 0, _lib.current_stream(act.device)))
    torch.cuda.synchronize()
    assert torch.equal(a0, act) and torch.equal(l0, lp)
    a1, l1 = torch.empty(320, 4, device=DEV), torch.empty(320, device=DEV)
    m1 = mean[192:512].contiguous()
    _lib.check(L.vf_head_sample_at(m1.data_ptr(), ls.data_ptr(), a1.data_ptr(), l1.data_ptr(), 320, 192, 77, 40, 0, _lib.current_stream(act.device)))
    torch.cuda.synchronize()
    assert torch.equal(a1, a0[192:512]) and torch.equal(l1, l0[192:512])
    # arguments
    assert L.vf_noise_fill(None, 1, 1, 0, 0, 0, None) == -1 and L.vf_noise_fill(big.data_ptr(), 0, 1, 0, 0, 0, None) == -1
    assert L.vf_noise_fill(big.data_ptr(), 1, 1000, 2 ** 32 - 999, 0, 0, None) == -1
    assert L.vf_head_sample_at(mean.data_ptr(), ls.data_ptr(), act.data_ptr(), lp.data_ptr(), 1000, 2 ** 32 - 999, 77, 40, 0, None) == -1


def test_noise_fill_is_standard_normal():
    """mean, variance and lag-1 correlation of 2^22 samples within 5 standard errors of N(0, 1): se(mean) = 1 / sqrt(n), se(variance) =
    sqrt(2 / n) (normal fourth moment 3), se(lag-1 correlation) = 1 / sqrt(n) (white noise)"""
    x = _fill(4, 2 ** 18, 12345, 2024, 7).double().flatten()
    n = x.numel()
    assert n >= 2 ** 20
    mean, var = float(x.mean()), float(x.var(unbiased=True))
    xc = x - x.mean()
    lag1 = float((xc[1:] * xc[:-1]).sum() / (xc * xc).sum())
    # ... also between the same component of neighbouring agents and of consecutive steps of one agent
    y = xc.view(4, 2 ** 18, 4)
    lag_agent = float((y[:, 1:] * y[:, :-1]).sum() / (y * y).sum())
    lag_step = float((y[1:] * y[:-1]).sum() / (y[1:] * y[1:]).sum())
    print(f"n={n} mean={mean:.3e} var-1={var - 1:.3e} lag1={lag1:.3e} lag_agent={lag_agent:.3e} lag_step={lag_step:.3e}")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(var - 1.0) < 5 * math.sqrt(2.0 / n)
    assert abs(lag1) < 5 / math.sqrt(n) and abs(lag_agent) < 5 / math.sqrt(n) and abs(lag_step) < 5 / math.sqrt(n * 3 / 4)


# ---- trainers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_ppo_rollout_buffer_of_the_shards_is_the_whole_buffer(fused):
    """collect_rollouts, persistent launch and per-step loop: the union of the shards' buffers is the single env's buffer (the rewards
    include the TimeLimit bootstrap: episodes of 7 steps, 20-step roll-outs)"""
    from visfly_amd.ppo import PPO

    def run(n, off):
        env = _env("NavigationEnv", n, off, max_episode_steps=7)
        ppo = PPO(env, n_steps=20, batch_size=n * 20, n_epochs=1, seed=2, policy_kwargs=dict(activation_fn="relu"))
        ppo.fused_rollout = fused
        ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert ppo.fused_rollout is fused
        out = {k: getattr(ppo.buf, k).clone() for k in ("actions", "log_probs", "values", "rewards", "episode_starts")}
        out.update({"obs:" + k: ppo.buf.obs[k].clone() for k in ppo.obs_keys})
        out["params"] = ppo.policy.flat.clone()
        env.close()
        return out

    whole = run(N, 0)
    keys = ("obs:state", "obs:target", "actions", "log_probs", "values", "rewards", "episode_starts")
    for split in SPLITS:
        for a, b in _shards(split):
            part = run(b - a, a)
            assert torch.equal(part["params"], whole["params"])
            for k in keys:
                print(f"ppo fused={fused} split={split} rows [{a},{b}) {k}: max|diff| = {float((part[k] - whole[k][:, a:b]).abs().max()):.3e}")
            for k in keys:
                assert torch.equal(part[k], whole[k][:, a:b]), (fused, split, a, k)


def _horizon_run(algo_name, n, off, fused, H=16):
    from visfly_amd.bptt import BPTT
    from visfly_amd.shac import SHAC
    env = _env("HoverEnv", n, off, max_episode_steps=7, requires_grad=True)
    if algo_name == "shac":
        algo = SHAC(env, horizon=H, learning_rate=1e-3, seed=9)
    elif algo_name == "bptt_ref":
        algo = BPTT(env, policy="MultiInputPolicy", horizon=H, learning_rate=1e-3, seed=9)
    else:
        algo = BPTT(env, horizon=H, learning_rate=1e-3, seed=9)
    algo.fused_rollout = algo.fused_reverse = fused
    algo._grad_reverse_sweep()
    torch.cuda.synchronize()
    assert algo._noise_step == (2 * H if algo_name == "shac" else H)
    out = {k: v.clone() for k, v in algo._horizon.items()}
    out["grad"] = algo.policy.grad.clone()
    env.close()
    return out


@pytest.mark.parametrize("algo_name", ["bptt", "bptt_ref", "shac"])
def test_one_horizon_over_the_shards_is_the_horizon_over_the_whole(algo_name):
    """per-agent actions, (SHAC: rewards,) and loss rows of one H = 16 horizon; persistent launches == launch-by-launch loop stays
    bit-identical in globally keyed mode; the shards' gradients (each already divided by its own N) recombine to the whole one"""
    whole = _horizon_run(algo_name, N, 0, True)
    loop = _horizon_run(algo_name, N, 0, False)
    for k in whole:
        assert torch.equal(whole[k], loop[k]), f"{algo_name}: persistent vs loop, {k}"
    for split in SPLITS:
        gsum = torch.zeros_like(whole["grad"])
        for a, b in _shards(split):
            part = _horizon_run(algo_name, b - a, a, True)
            for k in part:
                if k == "grad":
                    continue
                full = whole[k][:, a:b] if whole[k].dim() > 1 else whole[k][a:b]
                print(f"{algo_name} split={split} rows [{a},{b}) {k}: max|diff| = {float((part[k].float() - full.float()).abs().max()):.3e}")
                assert torch.equal(part[k], full), (algo_name, split, a, k)
            gsum += part["grad"] * ((b - a) / N)
        scale = float(whole["grad"].abs().max())
        assert torch.allclose(gsum, whole["grad"], rtol=1e-5, atol=1e-6 * scale)      # same gradient, different summation order


@pytest.mark.parametrize("policy", [None, "MultiInputPolicy"])
def test_checkpoint_carries_the_noise_step(policy, tmp_path):
    """save after one update, load into a fresh trainer, update: the noise of an uninterrupted run's second update (both archive kinds:
    the SB3-layout zip of the MlpPolicy actor, the torch archive of the reference actor)"""
    from visfly_amd.bptt import BPTT

    def trainer():
        env = _env("HoverEnv", 256, 256, max_episode_steps=7, requires_grad=True)
        tr = BPTT(env, policy=policy, horizon=8, learning_rate=1e-3, seed=9)
        drawn, orig = [], tr._noise
        tr._noise = lambda T, n: drawn.append(orig(T, n).clone()) or drawn[-1].clone()
        return env, tr, drawn

    env, a, drawn_a = trainer()
    a._update()
    a._update()
    assert len(drawn_a) == 2 and a._noise_step == 16 and not torch.equal(drawn_a[0], drawn_a[1])
    env.close()
    env, b, drawn_b = trainer()
    b._update()
    path = str(tmp_path / ("ck.zip" if policy is None else "ck.pth"))
    gen_state = b._gen.get_state().clone()
    b.save(path)
    env.close()
    env, c, drawn_c = trainer()
    assert c._noise_step == 0
    c.set_parameters(path)
    assert c._noise_step == 8
    if policy is not None:
        assert torch.equal(c._gen.get_state().cpu(), gen_state.cpu())      # next to, not instead of, the generator state
    c._update()
    assert torch.equal(drawn_b[0], drawn_a[0]) and torch.equal(drawn_c[0], drawn_a[1])
    env.close()


# ---- two processes on one device over gloo ----------------------------------------------------------------------------------
def _worker(rank, world, port, q, algo):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from visfly_amd import parallel
    r, w, _ = parallel.init("gloo")
    assert (r, w) == (rank, world)
    torch.cuda.set_device(0)
    kw = parallel.shard_kwargs(N)
    assert kw == dict(num_agent_per_scene=N // world, agent_offset=rank * (N // world))
    if algo == "ppo":
        from visfly_amd.ppo import PPO
        env = _env("NavigationEnv", kw["num_agent_per_scene"], kw["agent_offset"], max_episode_steps=7)
        tr = PPO(env, n_steps=16, batch_size=16 * N, n_epochs=1, learning_rate=3e-4, seed=3, policy_kwargs=dict(activation_fn="relu"))
        tr.collect_rollouts()
        tr.train()
    else:
        from visfly_amd.bptt import BPTT
        env = _env("HoverEnv", kw["num_agent_per_scene"], kw["agent_offset"], max_episode_steps=7, requires_grad=True)
        tr = BPTT(env, horizon=8, learning_rate=1e-3, seed=3)
        tr._update()
    torch.cuda.synchronize()
    assert tr._opt_step == 1
    q.put((rank, tr.policy.grad.detach().cpu().numpy(), tr.policy.flat.detach().cpu().numpy()))
    if world > 1:
        dist.destroy_process_group()


def _run_world(algo, world, port):
    """each child under its own time limit; join + exit-code check, no retry"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, algo)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=300))
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
                p.join()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return sorted(res, key=lambda x: x[0])


@pytest.mark.parametrize("algo", ["ppo", "bptt"])
def test_two_ranks_take_the_single_rank_step(algo):
    """2 x 256 agents built with shard_kwargs vs one process with 512, same seed: after the first optimiser step the all-reduced gradient
    and the updated parameters are the single-rank ones up to the summation order (sum over agents, PPO's global advantage
    statistics): rtol 1e-5, atol 1e-6 x the largest magnitude of the compared vector"""
    import numpy as np
    base = 29300 + os.getpid() % 200 + (0 if algo == "ppo" else 2)
    (_, g1, p1), = _run_world(algo, 1, base)
    two = _run_world(algo, 2, base + 1)
    assert [r[0] for r in two] == [0, 1]
    assert np.array_equal(two[0][1], two[1][1]) and np.array_equal(two[0][2], two[1][2])         # the ranks agree with each other ...
    for name, x, y in (("gradient", two[0][1], g1), ("parameters", two[0][2], p1)):              # ... and with the single rank
        scale = float(np.abs(y).max())
        err = np.abs(x - y)
        print(f"{algo} {name}: max|diff| = {err.max():.3e}, max|.| = {scale:.3e}, worst excess over rtol = {(err - 1e-5 * np.abs(y)).max():.3e}")
        assert np.isfinite(x).all() and scale > 0
        assert np.allclose(x, y, rtol=1e-5, atol=1e-6 * scale), name
