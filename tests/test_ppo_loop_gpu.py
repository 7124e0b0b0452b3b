"""The PPO update LOOP against the reference's own ``PPO.train()`` (tests/golden/ppo_loop_nav*.npz, oracle/gen_ppo_loop.py): the reference's
train() (utils/algorithms/PPO.py:177-337) was run, unmodified, on its own CustomMultiInputActorCriticPolicy / StateTargetExtractor /
DictRolloutBuffer for 2 epochs x (3 full minibatches + a partial one); ``visfly_amd.ppo.PPO.train`` replays the same minibatches (the
recorded permutations) from the same rollout and initial parameters and must reproduce, per optimiser step, the loss, the value loss, the
flat gradient before clipping, its norm and the parameters after clip + Adam -- and per run the epoch / minibatch at which ``target_kl``
stops the loop, the number of optimiser steps and everything train() hands to its logger (equal-weight means over minibatches, the last
minibatch's loss, explained variance, std, n_updates = epochs, learning rate and clip ranges).  Third case: learning_rate / clip_range /
clip_range_vf are callables of SB3's progress_remaining, train() entered with 40 % of the run remaining.  Tolerances: those of the SHAC / BPTT loop fixtures (fp32 MFMA chains
vs MKL sgemm: gradients 2e-5 of the block scale, Adam 2e-7 absolute).

The ROLL-OUT half (tests/golden/ppo_rollout_nav.npz, oracle/gen_ppo_loop.py::gen_ppo_rollout): two consecutive runs of SB3's
``OnPolicyAlgorithm.collect_rollouts`` on the reference's own NavigationEnv / policy / ``compute_returns_and_advantage``;
``PPO.collect_rollouts(replay=...)`` takes the recorded noise and steps a ``spawn="replay"`` env with the recorded actions, so the env side
is compared bit for bit and what the policy kernels write at a tolerance sized from the reference's own fp32-vs-float64 distance."""
import ast
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["ppo_loop_nav", "ppo_loop_nav_kl", "ppo_loop_nav_sched"]


def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_a_run_of_the_references_train(name):
    """what the fixture must contain to pin the loop: both clip_grad_norm_ branches, the trailing partial minibatch, and (second case) an
    early stop inside the second epoch that costs an evaluated minibatch but no optimiser step"""
    fx = load(name)
    T, N, bs = int(fx["T"]), int(fx["N"]), int(fx["batch_size"])
    assert "the reference's own PPO.train" in str(fx["label"])
    assert fx["params0"].size == 43977 == fx["grad"].shape[1] == fx["params"].shape[1]
    per_epoch = [bs] * (T * N // bs) + ([T * N % bs] if T * N % bs else [])
    assert fx["mb_rows"].tolist() == (per_epoch * int(fx["n_epochs"]))[:len(fx["mb_rows"])]
    assert fx["perms"].shape == (int(fx["epochs_started"]), T * N) and all(sorted(p) == list(range(T * N)) for p in fx["perms"].tolist())
    n_opt = len(fx["loss"])
    if name == "ppo_loop_nav":
        assert fx["grad_norm"].min() < float(fx["max_grad_norm"]) < fx["grad_norm"].max(), "both branches of the gradient clip"
    if float(fx["target_kl"]) > 0:
        assert bool(fx["early_stop"]) and len(fx["value_loss"]) == n_opt + 1 and int(fx["epochs_started"]) == 2 and n_opt > len(per_epoch)
    else:
        assert not bool(fx["early_stop"]) and len(fx["value_loss"]) == n_opt == len(per_epoch) * int(fx["n_epochs"])


def _trainer_on_fixture(name):
    """the trainer with the fixture's hyper-parameters, initial parameters and rollout buffer -> (env, ppo, fx, perms, device tensor maker)"""
    import torch
    from visfly_amd.envs import NavigationEnv
    from visfly_amd.ppo import PPO
    from _golden import ENV_DYN
    dev = "cuda:0"
    fx = load(name)
    T, N, bs = int(fx["T"]), int(fx["N"]), int(fx["batch_size"])
    opt = lambda k: None if float(fx[k]) < 0 else float(fx[k])
    lr_arg, clip_arg, clip_vf_arg = float(fx["lr"]), float(fx["clip_range"]), opt("clip_range_vf")
    if bool(fx["sched"]):        # the generator's schedules (oracle/gen_ppo_loop.py: sched_lr, sched_clip), passed as callables
        lr_arg, clip_arg, clip_vf_arg = (lambda p, v=lr_arg: v * p), (lambda p, v=clip_arg: v * (0.5 + 0.5 * p)), (lambda p, v=clip_vf_arg: v * (0.5 + 0.5 * p))
    env = NavigationEnv(num_agent_per_scene=N, seed=1, dynamics_kwargs=dict(ENV_DYN), device=dev, max_episode_steps=64, tensor_output=True)
    ppo = PPO(env, n_steps=T, batch_size=bs, n_epochs=int(fx["n_epochs"]), gamma=float(fx["gamma"]), gae_lambda=float(fx["gae_lambda"]),
              clip_range=clip_arg, ent_coef=float(fx["ent_coef"]), vf_coef=float(fx["vf_coef"]),
              max_grad_norm=float(fx["max_grad_norm"]), learning_rate=lr_arg, weight_decay=float(fx["weight_decay"]),
              adam_eps=float(fx["adam_eps"]), target_kl=opt("target_kl"), clip_range_vf=clip_vf_arg, seed=0,
              policy_kwargs=dict(activation_fn="relu"))        # the fixture's networks (oracle/gen_ppo_loop.py: activation_fn=nn.ReLU in both places)
    ppo._current_progress_remaining = float(fx["progress_remaining"])          # what learn() sets before train() (PPO.py:150-152)
    pol = ppo.policy
    n = pol.n_params
    assert n == fx["params0"].size
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pol.flat[:n].copy_(d(fx["params0"]))
    pol.mark_updated()
    b = ppo.buf
    b.obs["state"].copy_(d(fx["obs_state"]))
    b.obs["target"].copy_(d(fx["obs_target"]))
    b.actions.copy_(d(fx["actions"]))
    for dst, key in ((b.values, "values"), (b.log_probs, "log_probs"), (b.advantages, "advantages"), (b.returns, "returns")):
        dst.copy_(d(fx[key]))
    # the reference's rows are env-major (SB3 swap_and_flatten: row = env * T + step), the trainer's step-major
    perms = [(p % T) * N + (p // T) for p in fx["perms"].astype(np.int64)]
    return env, ppo, fx, perms, d


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_train_replays_the_references_train(name):
    import torch
    env, ppo, fx, perms, d = _trainer_on_fixture(name)
    pol = ppo.policy
    n = pol.n_params
    rec = {"loss": [], "value_loss": [], "grad": [], "params": [], "stepped": []}
    real = ppo._minibatch_update

    def spy(mb, stats_acc=None):
        rows = mb["adv"].numel()
        r = real(mb, stats_acc)
        s = ppo._stats[:9].double().cpu().numpy() / rows
        # PPO.py:257-261 with entropy_loss = -mean(-log_prob) (the squashed Gaussian has no analytical entropy, :249-251)
        rec["loss"].append(s[0] + float(fx["ent_coef"]) * s[2] + float(fx["vf_coef"]) * s[1])
        rec["value_loss"].append(s[1])
        rec["stepped"].append(r is not None)
        if r is not None:
            rec["grad"].append(pol.grad[:n].cpu().numpy().copy())
            rec["params"].append(pol.flat[:n].cpu().numpy().copy())
        return r
    ppo._minibatch_update = spy
    ppo.train(permutations=perms)
    torch.cuda.synchronize()

    n_opt = len(fx["loss"])
    assert rec["stepped"] == [True] * n_opt + [False] * (len(fx["value_loss"]) - n_opt), "same minibatches, same early stop"
    assert ppo._opt_step == n_opt and bool(ppo.logs["train/early_stop"]) == bool(fx["early_stop"])
    assert np.allclose(rec["value_loss"], fx["value_loss"], rtol=2e-5, atol=1e-7), (rec["value_loss"], fx["value_loss"])
    assert np.allclose(rec["loss"][:n_opt], fx["loss"], rtol=0, atol=2e-6 * max(1.0, np.abs(fx["loss"]).max())), (rec["loss"], fx["loss"])
    # per-layer blocks of the flat gradient, each against its own scale
    offs = [(ly.w_off, ly.w_off + ly.K * ly.No) for ly in pol.layers] + [(ly.b_off, ly.b_off + ly.No) for ly in pol.layers] + [(pol.log_std_off, n)]
    for i in range(n_opt):
        g, w = rec["grad"][i], fx["grad"][i]
        for lo, hi in offs:
            scale = max(np.abs(w[lo:hi]).max(), 1e-3 * np.abs(w).max())
            # (from the second step on the two runs no longer hold the same parameters to the last bit: the bound grows with the step)
            assert np.abs(g[lo:hi] - w[lo:hi]).max() <= 2e-5 * (i + 1) * scale, f"step {i}: gradient block [{lo}, {hi})"
        assert abs(np.linalg.norm(g.astype(np.float64)) - fx["grad_norm"][i]) <= 2e-5 * (i + 1) * fx["grad_norm"][i]
    # clip + Adam (torch.optim.Adam with weight_decay = L2 term in the gradient, PPO.py:284-292).  An Adam step is lr * m^ / (sqrt(v^) + eps):
    # for the handful of parameters whose gradient is ~1e-8 (units active in a row or two) a 1e-10 difference of the gradient is a
    # visible fraction of lr, whatever computes it -- so (a) the trainer's Adam is checked tightly against a float64 replay from the
    # trainer's OWN gradients, (b) against the reference's parameters the bulk must agree to the SHAC loop's 2e-7 per step and no
    # parameter may be off by more than 2 % of a full-size step
    lr, wd, eps, b1, b2 = float(fx["log_learning_rate"]), float(fx["weight_decay"]), float(fx["adam_eps"]), 0.9, 0.999
    p, m, v = fx["params0"].astype(np.float64), np.zeros(n), np.zeros(n)
    for i in range(n_opt):
        g = rec["grad"][i].astype(np.float64)
        g = g * min(1.0, float(fx["max_grad_norm"]) / (np.linalg.norm(g) + 1e-6)) + wd * p
        m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** (i + 1)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** (i + 1)) + eps)
        assert np.abs(rec["params"][i] - p).max() <= 3e-7 * (i + 1), f"Adam step {i} vs a float64 replay of the trainer's own gradients"
        diff = np.abs(rec["params"][i] - fx["params"][i])
        assert np.quantile(diff, 0.99) <= 2e-7 * (i + 1) and diff.max() <= 0.02 * lr * (i + 1), (i, np.quantile(diff, 0.99), diff.max())
    # what train() logs (PPO.py:322-336): equal-weight means over the evaluated minibatches (approx_kl: those of the last epoch started),
    # the last minibatch's loss, explained variance of the buffer, std, n_updates (+1 per epoch), the schedules' current values
    lg = ppo.logs
    for key, name, tol in (("train/value_loss", "log_value_loss", 2e-5), ("train/policy_gradient_loss", "log_policy_gradient_loss", 2e-5),
                           ("train/entropy_loss", "log_entropy_loss", 2e-6), ("train/approx_kl", "log_approx_kl", 2e-5),
                           ("train/clip_fraction", "log_clip_fraction", 1e-9), ("train/loss", "log_loss", 2e-5),
                           ("train/explained_variance", "log_explained_variance", 1e-5), ("train/std", "log_std_mean", 1e-6),
                           ("train/learning_rate", "log_learning_rate", 1e-12), ("train/clip_range", "log_clip_range", 1e-9)):
        assert abs(lg[key] - float(fx[name])) <= tol * max(1.0, abs(float(fx[name]))), (key, lg[key], float(fx[name]))
    assert lg["train/n_updates"] == int(fx["log_n_updates"]) == int(fx["n_updates"])
    if float(fx["clip_range_vf"]) > 0:
        assert abs(lg["train/clip_range_vf"] - float(fx["log_clip_range_vf"])) <= 1e-9
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_every_optimiser_step_from_the_references_own_state(name):
    """the replay above lets the two runs drift apart (its bounds grow with the step index: r05 verdict).  Here every optimiser step starts
    from the REFERENCE's state -- its parameters after the previous step and the Adam moments a float64 replay of its recorded gradients
    gives -- so that each step is held to the bounds of the first one: gradient 2e-5 of the block scale, norm 2e-5, parameters after clip +
    Adam 99 % within 2e-7 and none off by more than 2 % of a full-size step"""
    import torch
    env, ppo, fx, perms, d = _trainer_on_fixture(name)
    pol = ppo.policy
    n = pol.n_params
    lr, wd, eps, b1, b2, mx = float(fx["log_learning_rate"]), float(fx["weight_decay"]), float(fx["adam_eps"]), 0.9, 0.999, float(fx["max_grad_norm"])
    n_opt = len(fx["loss"])
    # the reference's optimiser state before step k, from its own gradients (float64)
    m, v, states = np.zeros(n), np.zeros(n), []
    for k in range(n_opt):
        states.append((m.copy(), v.copy()))
        p_before = (fx["params0"] if k == 0 else fx["params"][k - 1]).astype(np.float64)
        g = fx["grad"][k].astype(np.float64)
        g = g * min(1.0, mx / (np.linalg.norm(g) + 1e-6)) + wd * p_before
        m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
    rec = {"grad": [], "params": []}
    real = ppo._minibatch_update
    offs = [(ly.w_off, ly.w_off + ly.K * ly.No) for ly in pol.layers] + [(ly.b_off, ly.b_off + ly.No) for ly in pol.layers] + [(pol.log_std_off, n)]

    def spy(mb, stats_acc=None):
        k = len(rec["grad"])
        if 0 < k < n_opt:          # continue from where the REFERENCE stood
            pol.flat[:n].copy_(d(fx["params"][k - 1]))
            pol.mark_updated()
            ppo.exp_avg[:n].copy_(d(states[k][0].astype(np.float32)))
            ppo.exp_avg_sq[:n].copy_(d(states[k][1].astype(np.float32)))
        r = real(mb, stats_acc)
        if r is not None:
            rec["grad"].append(pol.grad[:n].cpu().numpy().copy())
            rec["params"].append(pol.flat[:n].cpu().numpy().copy())
        return r
    ppo._minibatch_update = spy
    ppo.train(permutations=perms)
    torch.cuda.synchronize()
    assert len(rec["grad"]) == n_opt
    for i in range(n_opt):
        g, w = rec["grad"][i], fx["grad"][i]
        for lo, hi in offs:
            scale = max(np.abs(w[lo:hi]).max(), 1e-3 * np.abs(w).max())
            assert np.abs(g[lo:hi] - w[lo:hi]).max() <= 2e-5 * scale, f"step {i}: gradient block [{lo}, {hi})"
        assert abs(np.linalg.norm(g.astype(np.float64)) - fx["grad_norm"][i]) <= 2e-5 * fx["grad_norm"][i]
        diff = np.abs(rec["params"][i] - fx["params"][i])
        assert np.quantile(diff, 0.99) <= 2e-7 and diff.max() <= 0.02 * lr, (i, np.quantile(diff, 0.99), diff.max())
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# the roll-out half: collect_rollouts
# ------------------------------------------------------------------------------------------------------------------------------------
ROLLOUT = "ppo_rollout_nav"
EDGES = ("n_truncated", "n_not_truncated", "n_agents_two_ends", "n_end_last_step", "n_end_step0")


def _rollout(fx, r):
    return {k[len(f"r{r}_"):]: v for k, v in fx.items() if k.startswith(f"r{r}_")}


def _forward_tol(fx):
    """-> (tol, dist): dist = the largest distance between the reference's fp32 value / log-prob rows and the same policy evaluated in
    float64 on the same rows and noise (what fp32 arithmetic costs the reference itself); tol = 4 * dist, the margin for fp32 MFMA chains
    summing in another order than torch's CPU sgemm.  Callers cap it, per element, by the bound test_policy_loss_and_gradients_vs_torch_autograd
    holds for the same network's heads (atol 2e-5 + rtol 1e-4): see _within"""
    dist = 0.0
    for r in range(int(fx["n_rollouts"])):
        ro = _rollout(fx, r)
        dist = max(dist, float(np.abs(ro["values"] - ro["value_fp64"]).max()), float(np.abs(ro["log_probs"] - ro["log_prob_fp64"]).max()),
                   float(np.abs(ro["last_values"] - ro["last_value_fp64"]).max()))
    return 4.0 * dist, dist


def _within(got, want, tol, what, scale=1.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = scale * np.minimum(tol, 2e-5 + 1e-4 * np.abs(want))
    err = np.abs(got - want)
    print(f"{what}: max |HIP - reference| = {err.max() if err.size else 0.0:.3e} (bound {bound.min() if bound.size else 0.0:.3e} .. {bound.max() if bound.size else 0.0:.3e})")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} of {err.size} beyond the bound, worst {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    return float(err.max()) if err.size else 0.0


def test_rollout_fixture_is_a_run_of_the_references_collect_rollouts():
    """what the fixture must contain to pin the seam, recounted from the stored arrays: truncated and non-truncated episode ends, an agent
    with two ends in one roll-out, an end at the last step (dones into GAE non-zero) and at step 0, a second roll-out that starts inside
    running episodes; the bootstrap exactly at the listed rows; the reference's GAE from the stored rows, bit for bit"""
    import oracle
    fx = load(ROLLOUT)
    T, N, gamma, lam = int(fx["T"]), int(fx["N"]), float(fx["gamma"]), float(fx["gae_lambda"])
    assert "collect_rollouts" in str(fx["label"]) and "reference's own NavigationEnv" in str(fx["label"])
    assert fx["params0"].size == 43977 and fx["fs_init"].shape == (N, 22) and int(fx["n_rollouts"]) == 2
    total = dict.fromkeys(EDGES, 0)
    prev_dones = np.ones(N, np.float32)
    for r in range(2):
        ro = _rollout(fx, r)
        done, trunc = ro["done"].astype(bool), ro["truncated"].astype(bool)
        assert done.shape == (T, N) and not (trunc & ~done).any()
        cnt = dict(n_truncated=int(trunc.sum()), n_not_truncated=int((done & ~trunc).sum()), n_agents_two_ends=int((done.sum(0) >= 2).sum()),
                   n_end_last_step=int(done[T - 1].sum()), n_end_step0=int(done[0].sum()))
        for k in EDGES:
            assert cnt[k] == int(ro[k]), (r, k)
            total[k] += cnt[k]
        # _last_episode_starts = dones: row t + 1 is the done flags of step t, row 0 what the previous roll-out left, GAE gets the last
        assert np.array_equal(ro["episode_starts"][0], prev_dones) and np.array_equal(ro["episode_starts"][1:], done[:-1].astype(np.float32))
        assert np.array_equal(ro["dones"], done[T - 1].astype(np.float32))
        prev_dones = ro["dones"]
        # every episode end re-spawns its agent, in step order
        ts, ag = np.nonzero(done)
        assert np.array_equal(ro["ev_step"], ts) and np.array_equal(ro["ev_agent"], ag) and ro["ev_fs"].shape == (len(ts), 22)
        # the bootstrap: rewards == rewards_raw + gamma * V(terminal observation) at exactly the truncated rows, in float32 as
        # `rewards[idx] += self.gamma * terminal_value` computes it, and nowhere else
        bs, ba = np.nonzero(trunc)
        assert np.array_equal(ro["boot_step"], bs) and np.array_equal(ro["boot_agent"], ba) and ro["boot_state"].shape == (len(bs), 13)
        want = ro["rewards_raw"].copy()
        want[bs, ba] = want[bs, ba] + np.float32(gamma) * ro["boot_value"]
        assert np.array_equal(want.view(np.uint32), ro["rewards"].view(np.uint32))
        assert np.abs(ro["boot_value"]).min() > 0 and (ro["rewards"][bs, ba] != ro["rewards_raw"][bs, ba]).all()
        # the action that went to env.step next to the one in the buffer: the same to a rounding of (a + 1) (unscale_action on a [-1, 1] box)
        assert np.abs(ro["actions_env"] - ro["actions"]).max() <= 2.0 ** -23 and np.abs(ro["actions_env"]).max() <= 1.0
        adv, ret = oracle.gae(ro["rewards"], ro["values"], ro["episode_starts"], ro["last_values"], ro["dones"], gamma, lam)
        assert np.array_equal(adv.view(np.uint32), ro["advantages"].view(np.uint32))
        assert np.array_equal(ret.view(np.uint32), ro["returns"].view(np.uint32))
    for k in EDGES:
        assert total[k] >= 1 and total[k] == int(fx[k]), k
    assert _rollout(fx, 0)["episode_starts"][0].min() == 1.0 and 0.0 == _rollout(fx, 1)["episode_starts"][0].min() < _rollout(fx, 1)["episode_starts"][0].max()
    tol, dist = _forward_tol(fx)
    assert 0 < dist < 1e-5 and tol <= 2e-5, (tol, dist)       # fp32 noise, and never looser than the head bound of test_ppo_gpu.py


@pytest.mark.gpu
@pytest.mark.parametrize("defer", [True, False], ids=["deferred_bootstrap", "per_step_bootstrap"])
def test_collect_rollouts_replays_the_reference(defer):
    """PPO.collect_rollouts, launch by launch, against the recorded run: env side (spawn states, observation rows, episode starts, raw
    rewards, which rows are bootstrapped and from which terminal rows) bit for bit; values, log-probs, the kernel's own samples and last
    values at the forward tolerance, bootstrapped rewards at gamma times it; vf_gae equal to the reference's recurrence on the GPU's own
    rows bit for bit and within the propagated tolerance of the recorded advantages / returns.  Measured: see DESIGN.md (parity)."""
    import oracle
    import torch
    from visfly_amd.envs import NavigationEnv
    from visfly_amd.ppo import PPO
    from _golden import assert_bits_equal, consts_of
    dev = "cuda:0"
    fx = load(ROLLOUT)
    T, N, gamma, lam = int(fx["T"]), int(fx["N"]), float(fx["gamma"]), float(fx["gae_lambda"])
    tol, dist = _forward_tol(fx)
    print(f"forward tolerance {tol:.3e} = 4 x {dist:.3e} (the reference's fp32 rows vs float64)")
    env = NavigationEnv(num_agent_per_scene=N, num_scene=1, seed=int(fx["seed"]), visual=False, dynamics_kwargs=ast.literal_eval(str(fx["dyn_kw"])),
                        device=dev, tensor_output=True, max_episode_steps=int(fx["max_episode_steps"]),
                        random_kwargs=ast.literal_eval(str(fx["spawn"])), spawn="replay", replay_trig="cr", constants=consts_of(fx))
    ppo = PPO(env, n_steps=T, batch_size=T * N, n_epochs=1, gamma=gamma, gae_lambda=lam, seed=0, policy_kwargs=dict(activation_fn="relu"))
    ppo.defer_bootstrap = defer
    pol = ppo.policy
    assert pol.n_params == fx["params0"].size
    pol.flat[:pol.n_params].copy_(torch.from_numpy(fx["params0"]).to(dev))
    pol.mark_updated()
    n = lambda t: t.detach().cpu().numpy()
    assert_bits_equal(n(env.full_state), fx["fs_init"], "spawn states of the replayed stream")
    assert_bits_equal(n(ppo._last_obs["state"]), fx["obs0_state"], "reset() observation")
    spawned = []
    real_step = env.step

    def step(action, *a, **k):
        out = real_step(action, *a, **k)
        idx = np.nonzero(n(out[2]))[0]
        spawned.append((idx, n(env.full_state)[idx]))
        return out
    env.step = step
    asked = []
    env.collect_policy = lambda *a, **k: asked.append(1) or False
    worst = dict.fromkeys(("values", "log_probs", "actions", "last_values", "boot_rewards", "advantages", "returns"), 0.0)
    for r in range(int(fx["n_rollouts"])):
        ro = _rollout(fx, r)
        del spawned[:]
        last_values = []
        real_pv = ppo.predict_values
        ppo.predict_values = lambda obs: last_values.append(real_pv(obs)) or last_values[-1]
        ppo.collect_rollouts(replay=dict(eps=ro["eps"], actions=ro["actions_env"]))
        ppo.predict_values = real_pv
        torch.cuda.synchronize()
        assert not asked, "a replayed roll-out is stepped launch by launch: the persistent launch draws its own noise"
        buf, w = ppo.buf, f"roll-out {r}: "
        # ---- the env side and the bookkeeping: bit for bit ----
        assert len(spawned) == T
        for t, (idx, fs) in enumerate(spawned):
            sel = ro["ev_step"] == t
            assert np.array_equal(idx, ro["ev_agent"][sel]), f"{w}which agents end an episode at step {t}"
            assert_bits_equal(fs, ro["ev_fs"][sel].reshape(-1, 22), f"{w}re-spawn states at step {t}")
        assert_bits_equal(n(buf.obs["state"]), ro["obs_state"], w + "obs['state'] rows")
        assert_bits_equal(n(buf.obs["target"]), ro["obs_target"], w + "obs['target'] rows")
        assert_bits_equal(n(buf.episode_starts), ro["episode_starts"], w + "episode_starts")
        assert_bits_equal(n(ppo._last_starts), ro["dones"], w + "_last_starts (dones into GAE)")
        assert_bits_equal(n(ppo._last_obs["state"]), ro["last_obs_state"], w + "_last_obs")
        boot = np.zeros((T, N), bool)
        boot[ro["boot_step"], ro["boot_agent"]] = True
        rewards = n(buf.rewards)
        assert_bits_equal(rewards[~boot], ro["rewards"][~boot], w + "rewards of the rows that are not bootstrapped")
        if defer:
            cnt = int(ppo._boot["cursor"].item())
            order = np.argsort(n(ppo._boot["idx"][:cnt]), kind="stable")
            assert np.array_equal(n(ppo._boot["idx"][:cnt])[order], ro["boot_step"].astype(np.int64) * N + ro["boot_agent"]), w + "the set of bootstrapped (step, agent)"
            assert_bits_equal(n(ppo._boot["rows0"][:cnt])[order], ro["boot_state"], w + "terminal rows of the bootstrapped episodes")
        # ---- what the policy kernels wrote: the forward tolerance ----
        worst["values"] = max(worst["values"], _within(n(buf.values), ro["values"], tol, w + "values"))
        worst["log_probs"] = max(worst["log_probs"], _within(n(buf.log_probs), ro["log_probs"], tol, w + "log_probs"))
        worst["actions"] = max(worst["actions"], _within(n(buf.actions), ro["actions"], tol, w + "sampled actions"))
        assert len(last_values) == 1
        worst["last_values"] = max(worst["last_values"], _within(n(last_values[0]), ro["last_values"], tol, w + "last_values"))
        # reward + gamma * V(terminal observation): the raw reward is exact, gamma * V carries gamma times the value's error
        worst["boot_rewards"] = max(worst["boot_rewards"], _within(rewards[boot] - ro["rewards_raw"][boot], ro["rewards"][boot].astype(np.float64) - ro["rewards_raw"][boot],
                                                                   tol, w + "bootstrap term of the bootstrapped rewards", scale=gamma))
        assert (rewards[boot] != ro["rewards_raw"][boot]).all()
        # ---- GAE: the reference's recurrence on the GPU's own rows, bit for bit; against the recorded ones, the propagated tolerance
        # (|delta| error <= (1 + gamma) tol [+ gamma tol on bootstrapped rows, inside the 4x margin], summed over (gamma lambda)^k) ----
        adv, ret = oracle.gae(rewards, n(buf.values), n(buf.episode_starts), n(last_values[0]), n(ppo._last_starts), gamma, lam)
        assert_bits_equal(n(buf.advantages), adv, w + "vf_gae vs the reference's recurrence on the same rows")
        assert_bits_equal(n(buf.returns), ret, w + "returns")
        gtol = tol * (1 + gamma) / (1 - gamma * lam)
        for key, got in (("advantages", adv), ("returns", ret)):
            err = float(np.abs(got.astype(np.float64) - ro[key]).max())
            print(f"{w}{key}: max |HIP - reference| = {err:.3e} (bound {gtol:.3e})")
            assert err <= gtol, (key, err, gtol)
            worst[key] = max(worst[key], err)
    print("measured, both roll-outs:", {k: f"{v:.3e}" for k, v in worst.items()})
    env.close()
