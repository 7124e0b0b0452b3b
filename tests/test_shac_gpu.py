"""SHAC against ONE iteration of the reference's own ``learn()`` loop (tests/golden/shac_hover.npz, oracle/gen_shac.py:
utils/algorithms/shac.py:215-278 with the reference's Actor / ContinuousCritic / StateExtractor / create_mlp /
SimpleRolloutBuffer / compute_td_returns over the differentiable HoverEnv; repaired-oracle, defect C-10).

fp32 on both sides, but the network arithmetic differs in summation order (fp32 MFMA tiles vs MKL sgemm) and tanh / exp come
from different libraries, so the comparison is at a stated tolerance, not bit level:
  * horizon buffer (observations, actions, rewards, next values)        1e-6 absolute (measured: <= 1.2e-7)
  * done / episode_done masks                                             exact
  * actor loss incl. the bootstrap term                                   2e-6
  * flat gradients (actor, critic)                                        2e-5 of the largest entry (measured: 2e-6 / 1e-7),
                                                                          per-layer blocks 1e-3
  * TD-lambda returns, critic losses                                      1e-5
  * one clipped Adam step / Polyak update from the REFERENCE's gradient   2e-7 absolute (parameters O(0.1))
"""
import ast

import numpy as np
import pytest
import torch

from _golden import assert_bits_equal, consts_of, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PK = dict(features_extractor_class="StateExtractor", features_extractor_kwargs={"net_arch": {"state": {"layer": [128, 64]}}},
          net_arch=dict(pi=[64, 64], qf=[64, 64]), activation_fn="relu", share_features_extractor=False)


def make(fx, share=False, **kw):
    from visfly_amd.envs import HoverEnv
    from visfly_amd.shac import SHAC
    N = fx["fs_init"].shape[0]
    env = HoverEnv(num_agent_per_scene=N, seed=int(fx["seed"]), dynamics_kwargs=ast.literal_eval(str(fx["dyn_kw"])), device=DEV,
                   tensor_output=True, requires_grad=True, max_episode_steps=int(fx["max_episode_steps"]),
                   random_kwargs=ast.literal_eval(str(fx["spawn"])), spawn="replay", replay_trig="cr", constants=consts_of(fx))
    env.reset()
    assert_bits_equal(env.full_state.cpu().numpy(), fx["fs_init"], "spawn states of the replayed stream")
    algo = SHAC(env, policy_kwargs=dict(PK, share_features_extractor=share), horizon=int(fx["H"]), tau=float(fx["tau"]), gamma=float(fx["gamma"]),
                gradient_steps=int(fx["gradient_steps"]), learning_rate=float(fx["lr"]), seed=int(fx["seed"]), **kw)
    a, c = algo.policy, algo.critic
    assert a.n_params == fx["actor_params0"].size == a.n_total and c.n_params == fx["critic_params0"].size == c.n_total - 20
    a.flat[:a.n_params].copy_(torch.from_numpy(fx["actor_params0"]))
    a.mark_updated()
    for net in (c, algo.critic_target):
        net.flat[:c.n_params].copy_(torch.from_numpy(fx["critic_params0"]))
        net.mark_updated()
    return env, algo


def blocks_close(got, want, pol, tol_all, tol_block, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= tol_all * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"
    for ly in pol.layers:
        if ly.frozen:
            continue
        for off, n in ((ly.w_off, ly.K * ly.No), (ly.b_off, ly.No)):
            w, g = want[off:off + n], got[off:off + n]
            s = np.abs(w).max()
            if s > 1e-4 * scale:
                assert np.abs(g - w).max() <= tol_block * s, f"{what}: layer {ly.src}->{ly.dst} block at {off}"
    return err / scale


def test_network_shapes_are_the_references():
    """Actor: extractor 13 -> 128 -> 64, latent_pi / log_latent_pi 64 -> 64 -> 64, mu / log_std 64 -> 4; critic: own extractor,
    features (+) action = 68 -> 64 -> 64 -> 1, twice (td_policies.py:82-143,146-252) -- parameter counts of the reference's modules"""
    fx = load("shac_hover")
    env, algo = make(fx)
    a, c = algo.policy, algo.critic
    assert [(ly.K, ly.No) for ly in a.layers] == [(13, 128), (128, 64), (64, 64), (64, 64), (64, 4), (64, 64), (64, 64), (64, 4)]
    assert [(ly.K, ly.No, ly.frozen) for ly in c.layers] == [(13, 128, False), (128, 64, False), (4, 4, True), (68, 64, False),
                                                             (64, 64, False), (64, 1, False), (68, 64, False), (64, 64, False),
                                                             (64, 1, False)]
    assert torch.equal(algo.critic_target.flat, c.flat)
    # the pass-through columns are exact copies of the action
    obs = {"state": torch.randn(300, 13, device=DEV), "action": torch.rand(300, 4, device=DEV) * 2 - 1}
    c.forward(obs, save_activations=True)
    assert torch.equal(c._buffers(300, 0)["feat"][:, 64:], obs["action"])
    env.close()


def test_one_iteration_matches_the_reference_loop():
    fx = load("shac_hover")
    env, algo = make(fx)
    H, N = int(fx["H"]), fx["fs_init"].shape[0]
    algo._eps_override = torch.from_numpy(fx["eps"]).to(DEV)
    # ---- actor: horizon + reverse sweep (shac.py:215-266) ----
    loss = algo._grad_reverse_sweep()
    b = algo._buf
    n = lambda t: t.cpu().numpy()
    assert np.array_equal(n(b["done"]), fx["buf_done"]) and np.array_equal(n(b["ep_done"]), fx["buf_episode_done"])
    for got, want, what in ((b["obs"]["state"], fx["buf_obs"], "observations"), (b["action"], fx["buf_action"], "actions"),
                            (b["reward"], fx["buf_reward"], "rewards"), (b["next_value"], fx["buf_next_value"], "next values")):
        err = np.abs(n(got) - want).max()
        print(f"horizon buffer {what}: max abs err {err:.2e}")
        assert err <= 1e-6, what
    assert abs(float(loss) - float(fx["actor_loss"])) <= 2e-6, (float(loss), float(fx["actor_loss"]))
    a = algo.policy
    rel = blocks_close(n(a.grad), fx["actor_grad"], a, 2e-5, 1e-3, "actor gradient")
    print(f"actor loss {float(loss):.7f} vs {float(fx['actor_loss']):.7f}; gradient rel err {rel:.2e}")
    # the optimiser step from the reference's own gradient (isolates clip + Adam from the gradient tolerance)
    a.grad.copy_(torch.from_numpy(fx["actor_grad"]))
    algo._apply(loss)
    assert np.abs(n(a.flat[:a.n_params]) - fx["actor_params1"]).max() <= 2e-7
    # ---- TD-lambda returns of the reference's buffer (bit level) and of ours (tolerance) ----
    from visfly_amd import _lib
    L, st = _lib.lib(), _lib.current_stream(torch.device(DEV))
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    ret = torch.empty((H, N), device=DEV)
    r_, d_, e_, v_ = f(fx["buf_reward"]), f(fx["buf_done"]), f(fx["buf_episode_done"]), f(fx["buf_next_value"])
    _lib.check(L.vf_td_returns(r_.data_ptr(), d_.data_ptr(), e_.data_ptr(), v_.data_ptr(), ret.data_ptr(), H, N, 0.99, float(fx["lamda"]), st))
    assert_bits_equal(n(ret), fx["buf_returns"], "vf_td_returns on the reference's buffer")
    # ---- critic updates on the reference's buffer (shac.py:267-274), one step at a time ----
    c, tg = algo.critic, algo.critic_target
    obs, act, target = {"state": f(fx["buf_obs"]).view(H * N, 13)}, f(fx["buf_action"]).view(H * N, 4), f(fx["buf_returns"]).view(-1)
    for i in range(int(fx["gradient_steps"])):
        # gradient at the REFERENCE's parameters of this step
        prev = fx["critic_params0"] if i == 0 else fx["critic_params"][i - 1]
        c.flat[:c.n_params].copy_(torch.from_numpy(prev))
        c.mark_updated()
        tprev = fx["critic_params0"] if i == 0 else fx["target_params"][i - 1]
        tg.flat[:c.n_params].copy_(torch.from_numpy(tprev))
        loss_c = algo._critic_step_once(obs, act, target)
        assert abs(float(loss_c) - float(fx["critic_loss"][i])) <= 1e-5 * max(1.0, abs(float(fx["critic_loss"][i])))
        # _critic_step_once has already stepped: the gradient it used is still in c.grad
        rel = blocks_close(n(c.grad), fx["critic_grad"][i], c, 2e-5, 1e-3, f"critic gradient, step {i}")
        print(f"critic step {i}: loss {float(loss_c):.6f} vs {float(fx['critic_loss'][i]):.6f}; gradient rel err {rel:.2e}")
    # the critic's optimiser trajectory from the reference's own gradients: clip 0.5 (step 0 exceeds it) + Adam + Polyak
    env2, algo2 = make(fx)
    c, tg = algo2.critic, algo2.critic_target
    from visfly_amd.ppo import _ptr
    import ctypes as C
    for i in range(int(fx["gradient_steps"])):
        c.grad.copy_(torch.from_numpy(fx["critic_grad"][i]))
        _lib.check(L.vf_sumsq(_ptr(c.grad), c.n_params, _ptr(algo2._c_sumsq), _ptr(algo2._scratch), st))
        algo2._critic_step += 1
        cfg = _lib.AdamCfg(algo2.lr, 0.9, 0.999, 1e-8, 0.0, 0.5, algo2._critic_step, 0, None, None)
        _lib.check(L.vf_adam_step(_ptr(c.flat), _ptr(c.grad), _ptr(algo2.c_exp_avg), _ptr(algo2.c_exp_avg_sq), c.n_params,
                                  _ptr(algo2._c_sumsq), C.byref(cfg), st))
        _lib.check(L.vf_polyak_update(_ptr(tg.flat), _ptr(c.flat), c.n_params, float(fx["tau"]), st))
        assert np.abs(n(c.flat[:c.n_params]) - fx["critic_params"][i]).max() <= 2e-7, f"critic parameters after step {i}"
        assert np.abs(n(tg.flat[:c.n_params]) - fx["target_params"][i]).max() <= 2e-7, f"target parameters after step {i}"
    assert float(np.linalg.norm(fx["critic_grad"][0])) > 0.5 > float(np.linalg.norm(fx["critic_grad"][-1]))   # both clip branches
    ident = n(tg.flat[c.n_params:]).reshape(-1)
    assert np.array_equal(ident[:16].reshape(4, 4), np.eye(4, dtype=np.float32)) and not ident[16:].any()   # the frozen block stays I
    env.close()
    env2.close()


def test_one_iteration_with_a_shared_extractor_matches_the_reference_loop():
    """r06: MTDPolicy(share_features_extractor=True) (td_policies.py:127; SB3 SACPolicy._build) -- tests/golden/shac_hover_shared.npz is ONE
    iteration of the reference's learn() with that flag (oracle/gen_shac.py --only shac_hover_shared).  The critic runs the ACTOR's extractor
    (its parameters follow the actor step, its optimiser leaves them alone, the gradient clip_grad_norm_ sees for them is the actor loss's,
    still sitting in .grad), the target keeps its own Polyak-averaged extractor.  Stages and tolerances of
    test_one_iteration_matches_the_reference_loop"""
    fx = load("shac_hover_shared")
    env, algo = make(fx, share=True)
    H, N = int(fx["H"]), fx["fs_init"].shape[0]
    a, c, tg = algo.policy, algo.critic, algo.critic_target
    e = algo._ext_end
    assert e == 13 * 128 + 128 + 128 * 64 + 64 and np.array_equal(fx["actor_params0"][:e], fx["critic_params0"][:e])
    n = lambda t: t.cpu().numpy()
    algo._eps_override = torch.from_numpy(fx["eps"]).to(DEV)
    loss = algo._grad_reverse_sweep()
    b = algo._buf
    for got, want, what in ((b["obs"]["state"], fx["buf_obs"], "observations"), (b["action"], fx["buf_action"], "actions"),
                            (b["reward"], fx["buf_reward"], "rewards"), (b["next_value"], fx["buf_next_value"], "next values")):
        assert np.abs(n(got) - want).max() <= 1e-6, what
    assert abs(float(loss) - float(fx["actor_loss"])) <= 2e-6
    blocks_close(n(a.grad), fx["actor_grad"], a, 2e-5, 1e-3, "actor gradient")
    # the actor step from the reference's own gradient, then what follows it in the shared mode
    a.grad.copy_(torch.from_numpy(fx["actor_grad"]))
    algo._apply(loss)
    algo._after_actor_step()
    assert np.abs(n(a.flat[:a.n_params]) - fx["actor_params1"]).max() <= 2e-7
    assert torch.equal(c.flat[:e], a.flat[:e]), "the critic's extractor IS the actor's"
    assert np.abs(n(c.flat[:e]) - fx["critic_params"][0][:e]).max() <= 2e-7
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    obs, act, target = {"state": f(fx["buf_obs"]).view(H * N, 13)}, f(fx["buf_action"]).view(H * N, 4), f(fx["buf_returns"]).view(-1)
    stale0 = algo._stale_ext.clone()
    for i in range(int(fx["gradient_steps"])):
        # loss and gradient at the REFERENCE's parameters of this step (its extractor block = the actor's after its step)
        prev = fx["critic_params0"] if i == 0 else fx["critic_params"][i - 1]
        c.flat[e:c.n_params].copy_(torch.from_numpy(prev[e:]))
        c.mark_updated()
        tg.flat[:c.n_params].copy_(torch.from_numpy(fx["critic_params0"] if i == 0 else fx["target_params"][i - 1]))
        algo._stale_ext.copy_(torch.from_numpy(fx["critic_grad"][i][:e]))        # (exactly what the reference's clip saw; checked against ours below)
        loss_c = algo._critic_step_once(obs, act, target)
        assert abs(float(loss_c) - float(fx["critic_loss"][i])) <= 1e-5 * max(1.0, abs(float(fx["critic_loss"][i])))
        blocks_close(n(c.grad), fx["critic_grad"][i], c, 2e-5, 1e-3, f"critic gradient, step {i}")
    # the extractor block of the gradient the reference's clip saw at step 0 = the actor loss's gradient x the actor's clip coefficient
    assert np.abs(n(stale0) - fx["critic_grad"][0][:e]).max() <= 1e-6 * max(np.abs(fx["critic_grad"][0][:e]).max(), 1e-12) + 1e-12
    # the optimiser trajectory from the reference's own gradients: clip + Adam on the q networks only, extractor untouched, Polyak over everything
    env2, algo2 = make(fx, share=True)
    a2, c2, tg2 = algo2.policy, algo2.critic, algo2.critic_target
    a2.flat[:a2.n_params].copy_(torch.from_numpy(fx["actor_params1"]))
    a2.mark_updated()
    algo2._sync_shared_extractor()
    for i in range(int(fx["gradient_steps"])):
        algo2._stale_ext.copy_(torch.from_numpy(fx["critic_grad"][i][:e]))
        algo2._critic_grad_override = torch.from_numpy(fx["critic_grad"][i]).to(DEV)
        algo2._critic_step_once(obs, act, target)
        assert np.abs(n(c2.flat[:c2.n_params]) - fx["critic_params"][i]).max() <= 2e-7, f"critic parameters after step {i}"
        assert np.abs(n(tg2.flat[:c2.n_params]) - fx["target_params"][i]).max() <= 2e-7, f"target parameters after step {i}"
        assert torch.equal(c2.flat[:e], a2.flat[:e]) and not algo2.c_exp_avg[:e].any() and not algo2.c_exp_avg_sq[:e].any()
    assert not np.array_equal(fx["target_params"][-1][:e], fx["critic_params"][-1][:e]), "the target keeps its own extractor"
    # ... and the loop as a whole runs in this mode
    algo2._critic_grad_override = None
    algo2._eps_override = None
    algo2.learn(2 * H * N)
    assert torch.equal(c2.flat[:e], a2.flat[:e]) and torch.isfinite(c2.flat).all() and torch.isfinite(a2.flat).all()
    env.close()
    env2.close()


@pytest.mark.parametrize("form", ["split", "one-wave"])
@pytest.mark.parametrize("M", [1000, 4096 + 17])
def test_fused_critic_step_equals_the_three_launch_step(M, form, monkeypatch):
    """vf_twin_q_update (forward + twin-Q loss + reverse chain in one launch) leaves the loss and the flat gradient of the
    forward / vf_twin_q_loss / backward path (same chain arithmetic; the masks come from registers instead of the saved activations) --
    row counts that are not multiples of the 32-row tile included; in both forms of the fused kernel: two half-network waves per row tile
    (k_twin_q_update_split, the default up to 32 768 rows) and one wave per tile (k_twin_q_update_chain)"""
    monkeypatch.setenv("VISFLY_AMD_CHAIN_SPLIT", "1" if form == "split" else "0")     # read by the library per call
    fx = load("shac_hover")
    env, algo = make(fx)
    c = algo.critic
    g = torch.Generator(device=DEV).manual_seed(5)
    obs = {"state": torch.randn((M, 13), device=DEV, generator=g)}
    act = torch.tanh(torch.randn((M, 4), device=DEV, generator=g))
    target = torch.randn(M, device=DEV, generator=g)
    out = {}
    for fused in (False, True):
        c.flat[:c.n_params].copy_(torch.from_numpy(fx["critic_params0"]))
        c.mark_updated()
        algo.fused_critic = fused
        algo._dq = None
        loss = algo._critic_step_once(obs, act, target)
        out[fused] = (float(loss), c.grad[:c.n_params].cpu().numpy().copy())
        if not fused:        # the loss kernel's head gradients and the saved activations of the three-launch step: the seed of the reference
            dq, saved = [t.clone().view(M, 1) for t in algo._dq[:2]], {k: v.clone() for k, v in c._buffers(M, 0).items() if torch.is_tensor(v)}
    assert c._fused_twin_q is not False, "the reference's critic shape must run on vf_twin_q_update"
    (l0, g0), (l1, g1) = out[False], out[True]
    assert abs(l0 - l1) <= 1e-6 * max(1.0, abs(l0)), (l0, l1)
    rel = blocks_close(g1, g0, c, 2e-6, 1e-4, "fused critic gradient")
    # every block on its own largest entry (no floor): fused against the three launches, and both against the fp64 network on the
    # parameters the steps started from (tests/_gradcheck.py)
    from _gradcheck import assert_blocks, assert_blocks_agree, pinned_reference
    c.flat[:c.n_params].copy_(torch.from_numpy(fx["critic_params0"]))
    pin = pinned_reference(c, {"state": obs["state"], "action": act}, saved, dq[0], dq[1], False)
    assert_blocks_agree(c, torch.from_numpy(g1), torch.from_numpy(g0), 2e-6, f"critic step M={M} {form}")
    assert_blocks(c, torch.from_numpy(g1), pin, f"critic step M={M} {form} fused")
    assert_blocks(c, torch.from_numpy(g0), pin, f"critic step M={M} {form} separate")
    print(f"M={M}: loss {l1:.7f} vs {l0:.7f}, gradient rel err {rel:.2e}")
    env.close()


def test_forward_steps_equals_the_per_step_forwards():
    """vf_mlp_forward_steps: n blocks of M rows in one launch == n vf_mlp_forward launches of M rows, bit for bit (the rows-per-wave choice is
    made for M rows), for the twin critic and for the actor; vf_shac_accumulate_horizon == H vf_shac_accumulate launches"""
    from visfly_amd import _lib
    fx = load("shac_hover")
    env, algo = make(fx)
    g = torch.Generator(device=DEV).manual_seed(11)
    M, n = 256, 5
    obs = torch.randn((n, M, 13), device=DEV, generator=g)
    act = torch.tanh(torch.randn((n, M, 4), device=DEV, generator=g))
    tg = algo.critic_target
    got = tg.forward_steps({"state": obs.view(n * M, 13), "action": act.view(n * M, 4)}, M, n)
    assert got is not None, "the reference's critic shape must run on vf_mlp_forward_steps"
    q0s, q1s = got[0].view(n, M).clone(), got[1].view(n, M).clone()
    for t in range(n):
        q0, q1 = algo._q(tg, {"state": obs[t]}, act[t])
        assert_bits_equal(q0s[t].cpu().numpy(), q0.cpu().numpy(), f"Q1 of block {t}")
        assert_bits_equal(q1s[t].cpu().numpy(), q1.cpu().numpy(), f"Q2 of block {t}")
    pol = algo.policy
    ga = pol.forward_steps({"state": obs.view(n * M, 13)}, M, n)
    assert ga is not None
    mus, lss = ga[0].view(n, M, 4).clone(), ga[1].view(n, M, 4).clone()
    for t in range(n):
        mu, ls = pol.forward({"state": obs[t].contiguous()}, save_activations=False, slot=0)
        assert_bits_equal(mus[t].cpu().numpy(), mu.cpu().numpy(), f"mu of block {t}")
        assert_bits_equal(lss[t].cpu().numpy(), ls.cpu().numpy(), f"log_std of block {t}")
    # the loss / discount recurrence of a horizon in one launch
    L, st = _lib.lib(), _lib.current_stream(torch.device(DEV))
    from visfly_amd.ppo import _ptr
    H, N = 7, 300
    f = dict(device=DEV)
    rew, qa, qb = (torch.randn((H, N), generator=g, **f) for _ in range(3))
    done = (torch.rand((H, N), generator=g, **f) < 0.2).to(torch.uint8)
    flags = (torch.randint(0, 16, (H, N), generator=g, **f)).to(torch.uint8)
    outs = []
    for batched in (False, True):
        disc, loss = torch.ones(N, **f), torch.zeros(N, **f)
        dr, nv, epd = torch.empty((H, N), **f), torch.empty((H, N), **f), torch.empty((H, N), dtype=torch.uint8, **f)
        if batched:
            _lib.check(L.vf_shac_accumulate_horizon(_ptr(rew), done.data_ptr(), flags.data_ptr(), _ptr(qa), _ptr(qb), _ptr(disc), _ptr(loss),
                                                    _ptr(dr), _ptr(nv), epd.data_ptr(), 0.99, 1.0 / N, H, N, st))
        else:
            for t in range(H):
                _lib.check(L.vf_shac_accumulate(_ptr(rew[t]), done[t].data_ptr(), flags[t].data_ptr(), _ptr(qa[t]), _ptr(qb[t]), _ptr(disc),
                                                _ptr(loss), _ptr(dr[t]), _ptr(nv[t]), epd[t].data_ptr(), 0.99, 1.0 / N, 1 if t == H - 1 else 0, N, st))
        outs.append([x.cpu().numpy() for x in (disc, loss, dr, nv, epd)])
    for a, b, what in zip(outs[0], outs[1], ("disc", "loss", "d_reward", "next_value", "ep_done")):
        assert_bits_equal(b, a, what)
    env.close()


def test_learn_runs_and_is_reproducible():
    """a few full iterations at a larger batch: finite, the critic loss falls, two runs from the same seed are bit-identical"""
    from visfly_amd.envs import HoverEnv
    from visfly_amd.shac import SHAC
    from _golden import ENV_DYN
    flats = []
    for _ in range(2):
        env = HoverEnv(num_agent_per_scene=2048, seed=3, dynamics_kwargs=dict(ENV_DYN), device=DEV, tensor_output=True,
                       requires_grad=True, max_episode_steps=64)
        algo = SHAC(env, policy_kwargs=dict(PK), horizon=16, gradient_steps=4, learning_rate=1e-3, seed=7)
        algo.learn(6 * 16 * 2048)
        assert np.isfinite(algo.logs["train/critic_loss"]) and np.isfinite(algo.logs["train/actor_loss"])
        assert torch.isfinite(algo.policy.flat).all() and torch.isfinite(algo.critic.flat).all()
        assert algo.num_timesteps == 6 * 16 * 2048
        flats.append((algo.policy.flat.clone(), algo.critic.flat.clone(), algo.critic_target.flat.clone()))
        a, _ = algo.predict(env.get_observation(), deterministic=True)
        assert a.shape == (2048, 4) and float(a.abs().max()) <= 1.0
        env.close()
    for x, y in zip(*flats):
        assert torch.equal(x, y)


FAST_SPAWN = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [1., 1., 1.]},
                                                                   "velocity": {"mean": [0., 0., 0.], "half": [9., 9., 9.]}}]}}


@pytest.mark.parametrize("N,H,steps,spawn", [(2048, 16, 20, None), (1000, 8, 5, None), (7, 6, 4, None), (3000, 12, 30, FAST_SPAWN),
                                             (1500, 8, 6, "NavigationEnv2"), (900, 8, 6, "HoverEnv2"), (1200, 8, 6, "RacingEnv2"),
                                             (1100, 8, 6, "generated"), (700, 8, 6, "generated:HoverEnv2")])
def test_persistent_launches_equal_the_loop(N, H, steps, spawn):
    """SHAC's horizon on vf_bptt_rollout / vf_bptt_reverse (actor class (b)) + the next-action / target-critic terms evaluated over the
    recorded horizon, against the launch-by-launch loop: horizon buffer (observations, actions, rewards, done / episode_done, next
    values, returns), actor loss and gradient, and actor / critic / target parameters after three iterations are bit-identical;
    short episodes, so that agents end episodes (terminations and truncations) inside the horizon"""
    import visfly_amd.envs as E
    from visfly_amd.shac import SHAC
    from _golden import ENV_DYN
    # r05: the observation / reward variants (their adjoint is obs_variant_bwd + the NAV2 reward gradient) run SHAC on the persistent
    # launches too -- NavigationEnv2 = the Navigation env kind under the one-observation actor (vf_bptt_*_hover.hip)
    # r06: RacingEnv2 -- the 16 gate-relative columns inside the launches (kernel-side kind VF_ENV_RACING2)
    # r06: "generated": a non-default net_arch -- actor AND twin critic are generated chain classes, the horizon runs from the actor
    # class's BPTT plugin (visfly_amd/_jit.py: PREBUILD_SAC["sac_hover"] / PREBUILD_CRITIC["critic_hover"] / PREBUILD_BPTT)
    pk = dict(PK)
    if isinstance(spawn, str) and spawn.startswith("generated"):
        pk = dict(features_extractor_class="StateExtractor", features_extractor_kwargs={"net_arch": {"state": {"layer": [64, 64, 32]}}},
                  net_arch=dict(pi=[32], qf=[32]), activation_fn="relu", share_features_extractor=False)
        spawn = spawn.partition(":")[2] or None
    generated = pk != PK
    cls, spawn = (getattr(E, spawn), None) if isinstance(spawn, str) else (E.HoverEnv, spawn)
    res = []
    for fused in (True, False):
        env = cls(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(ENV_DYN), device=DEV, tensor_output=True, requires_grad=True,
                  max_episode_steps=steps, **({} if spawn is None else {"random_kwargs": spawn}))
        algo = SHAC(env, policy_kwargs=dict(pk), horizon=H, gradient_steps=2, learning_rate=1e-3, seed=7)
        assert algo.policy.chain_jit == generated and algo.critic.chain_jit == generated
        algo.fused_rollout = algo.fused_reverse = fused
        used = []
        orig = env.rollout_policy
        env.rollout_policy = lambda *a, **k: used.append(orig(*a, **k)) or used[-1]
        out = {}
        for it in range(3):
            algo._update()
            b = algo._buf
            for k in ("action", "reward", "done", "ep_done", "next_value", "returns"):
                out[f"{k}{it}"] = b[k].clone()
            out[f"obs{it}"] = b["obs"]["state"].clone()
            out[f"grad{it}"] = algo.policy.grad.clone()
            out[f"loss{it}"] = algo._last_losses[0].clone().reshape(1)
        out["actor"], out["critic"], out["target"] = algo.policy.flat.clone(), algo.critic.flat.clone(), algo.critic_target.flat.clone()
        out["state"] = env.get_observation()["state"].clone()
        assert used == ([True] * 3 if fused else []), used
        res.append(out)
        env.close()
    n_done = sum(int(res[0][f"done{it}"].sum()) for it in range(3))
    n_ep = sum(int(res[0][f"ep_done{it}"].sum()) for it in range(3))
    print(f"done flags in the three horizons: {n_done}, of them episode_done: {n_ep}")
    assert n_done > 0 and (spawn is None or n_ep > 0)      # fast spawns: agents leave the bounding box = episode_done
    for k in res[0]:
        a, b = res[0][k], res[1][k]
        same = torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert same, f"{k} differs (max abs {float((a.float() - b.float()).abs().max()):.3e})"


def test_default_kwargs_iterations_lower_the_critic_loss():
    """no policy_kwargs (extractor [128, 64], trunks [64, 64]): the critic targets of OUR horizon buffer are the oracle's
    TD-lambda returns bit for bit, and regressing the twin critics onto them lowers the critic loss; save / load round trip"""
    import os
    import tempfile
    import oracle
    from visfly_amd import _lib
    from visfly_amd.envs import HoverEnv
    from visfly_amd.shac import SHAC
    from _golden import ENV_DYN
    env = HoverEnv(num_agent_per_scene=1024, seed=5, dynamics_kwargs=dict(ENV_DYN), device=DEV, tensor_output=True, max_episode_steps=20)
    algo = SHAC(env, horizon=8, gradient_steps=5, learning_rate=1e-3, seed=1)
    p0, t0 = algo.policy.flat.clone(), algo.critic_target.flat.clone()
    losses = []
    for _ in range(8):
        algo._update()
        losses.append(algo.flush_logs()["train/critic_loss"])
    b = algo._buf
    want = oracle.td_returns(b["reward"].cpu().numpy(), b["done"].cpu().numpy(), b["next_value"].cpu().numpy(),
                             b["ep_done"].cpu().numpy(), 0.99, 0.95)
    assert np.array_equal(b["returns"].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert b["done"].any() and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert not torch.equal(p0, algo.policy.flat) and not torch.equal(t0, algo.critic_target.flat)
    assert torch.isfinite(algo.policy.flat).all() and torch.isfinite(algo.critic.flat).all()
    with tempfile.TemporaryDirectory() as d:
        algo.save(os.path.join(d, "shac"))
        new = SHAC.load(os.path.join(d, "shac"), env, horizon=8, seed=99)
        for x, y in ((new.policy, algo.policy), (new.critic, algo.critic), (new.critic_target, algo.critic_target)):
            assert torch.equal(x.flat, y.flat)
    env.close()


@pytest.mark.parametrize("shape", ["critic", "odd"])
def test_forward_does_not_depend_on_stale_lds(shape):
    """layer tables whose widths are not multiples of the 16-step MFMA chunk (features (+) action = 68 columns, a 4-wide
    vector-staged input, hidden widths 100 / 50 / 40 / 24): the pad columns the sweep reads against zero weights must be zeros,
    not what an earlier kernel left in LDS -- with NaNs there a hidden unit turns into a silent 0 behind its ReLU (found in r03:
    next values off by 3e-2 in one run out of three)"""
    from visfly_amd import _lib
    from visfly_amd.ppo import MlpPolicy
    L, st = _lib.lib(), _lib.current_stream(torch.device(DEV))
    g = torch.Generator(device=DEV).manual_seed(5)
    M = 1000
    if shape == "critic":
        pol = MlpPolicy({"state": 13, "action": 4}, {"state": [128, 64]}, [64, 64], [64, 64], DEV, seed=3, ortho_init=False,
                        head_dims=(1, 1), passthrough=("action",), log_std_param=False)
        obs = {"state": torch.randn(M, 13, device=DEV, generator=g), "action": torch.rand(M, 4, device=DEV, generator=g) * 2 - 1}
    else:
        pol = MlpPolicy({"state": 13, "target": 3}, {"state": [100, 50], "target": [24]}, [40, 24], [72], DEV, seed=3, ortho_init=False)
        obs = {"state": torch.randn(M, 13, device=DEV, generator=g), "target": torch.randn(M, 3, device=DEV, generator=g)}
    ref = pol.to_torch().double()
    want = [x.detach() for x in ref({k: v.cpu().double() for k, v in obs.items()})]
    for save in (False, True, False):
        _lib.check(L.vf_debug_poison_lds(st))
        got = pol.forward(obs, save_activations=save)
        for a, b in zip(got, want):
            assert torch.isfinite(a).all()
            assert (a.cpu().double() - b).abs().max() <= 2e-5 * max(1.0, float(b.abs().max()))
