"""Bit record of the trainers' glue: for every case below, env and trainer from fixed seeds, two ``_update()`` calls (PPO: one
``collect_rollouts()`` + ``train()``) and a sha256 of everything an update leaves -- loss, parameters, gradient, Adam moments, the
horizon / roll-out buffers, the env's state rows -- then of ``predict``, ``_state()`` and a save / load round trip.  Run it on two
trees and compare the JSONs: a refactor of bptt.py / shac.py / ppo.py / policy.py has to reproduce every hash.

    python tools/trainer_parity.py OUT.json [case ...]         # writes {case: {field: sha256}}
    python tools/trainer_parity.py --compare A.json B.json     # exit status 1 and the differing fields if any hash differs

Sizes: HoverEnv bodyrate, N = 40 (two full 16-agent waves and a partial one), H = 3, max_episode_steps = 4 (done flags fire inside
the horizon): the smallest that still reach every branch of the sweeps."""
import hashlib
import json
import os
import sys
import tempfile
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DYN = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)        # tests/_golden.py: ENV_DYN
WIND = ["0.3 - 0.05*x", "0.02*x*x", "0.5*y + 0.1", "0*x + 0.125", "-0.01*x", "0.25*y - 0.05"]           # fixture bptt_wind_hover
N, H, DEV = 40, 3, "cuda:0"
WIDE = [256, 256]          # tests/test_wide_layers_gpu.py: wider than 128 -> layer by layer, the weight gradient is not deferred

# name -> (trainer, constructor kwargs, switches set after construction, dynamics kwargs)
CASES = {
    "bptt_mlp_fused": ("BPTT", {}, {}, {}),
    "bptt_mlp_loop": ("BPTT", {}, dict(fused_rollout=False, fused_reverse=False), {}),
    "bptt_mlp_autograd": ("BPTT", {}, dict(use_autograd=True), {}),
    "bptt_actor_fused": ("BPTT", dict(policy="MultiInputPolicy"), {}, {}),
    "bptt_actor_loop": ("BPTT", dict(policy="MultiInputPolicy"), dict(fused_rollout=False, fused_reverse=False), {}),
    "bptt_actor_wide": ("BPTT", dict(policy="MultiInputPolicy", policy_kwargs=dict(net_arch=WIDE)), {}, {}),
    "bptt_actor_wind": ("BPTT", dict(policy="MultiInputPolicy"), {}, dict(wind_settings=WIND)),
    "shac_fused_fused": ("SHAC", {}, {}, {}),
    "shac_fused_loopcritic": ("SHAC", {}, dict(fused_critic=False), {}),
    "shac_loop_fusedcritic": ("SHAC", {}, dict(fused_rollout=False, fused_reverse=False), {}),
    "shac_loop_loopcritic": ("SHAC", {}, dict(fused_rollout=False, fused_reverse=False, fused_critic=False), {}),
    "shac_shared_extractor": ("SHAC", dict(policy_kwargs=dict(share_features_extractor=True)), {}, {}),
    "shac_h1_fused": ("SHAC", dict(horizon=1), {}, {}),
    "shac_h1_loop": ("SHAC", dict(horizon=1), dict(fused_rollout=False, fused_reverse=False), {}),
    "shac_wide": ("SHAC", dict(policy_kwargs=dict(net_arch=dict(pi=WIDE, qf=WIDE))), {}, {}),
    "shac_wind": ("SHAC", {}, {}, dict(wind_settings=WIND)),
    "ppo": ("PPO", dict(n_steps=4, batch_size=64, n_epochs=2), {}, {}),
    "ppo_noclip": ("PPO", dict(n_steps=4, batch_size=64, n_epochs=2, max_grad_norm=None), {}, {}),
}


def sha(x):
    import torch
    if isinstance(x, torch.Tensor):
        x = x.detach().reshape(-1).contiguous().cpu()
        return hashlib.sha256(str((x.dtype, x.numel())).encode() + x.view(torch.uint8).numpy().tobytes()).hexdigest()
    return hashlib.sha256(repr(x).encode()).hexdigest()


def record(out, prefix, x):
    """x: tensor, number, None, or a (nested) dict / tuple of them -> one hash per leaf"""
    if isinstance(x, dict):
        for k in sorted(x):
            record(out, f"{prefix}.{k}", x[k])
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            record(out, f"{prefix}.{i}", v)
    else:
        out[prefix] = sha(x)


def make(name):
    import visfly_amd.envs as E
    from visfly_amd.bptt import BPTT
    from visfly_amd.ppo import PPO
    from visfly_amd.shac import SHAC
    kind, kw, switches, dyn = CASES[name]
    env = E.HoverEnv(num_agent_per_scene=N, seed=5, dynamics_kwargs=dict(DYN, **dyn), device=DEV, tensor_output=True,
                     max_episode_steps=4, requires_grad=kind != "PPO")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")        # (the one-time note that a wide network runs layer by layer)
        if kind == "PPO":
            algo = PPO(env, seed=3, **kw)
        else:
            algo = {"BPTT": BPTT, "SHAC": SHAC}[kind](env, **dict(dict(horizon=H, learning_rate=1e-3, seed=3), **kw))
    for k, v in switches.items():
        assert hasattr(algo, k), k
        setattr(algo, k, v)
    return env, algo


def run(name):
    import torch
    env, algo = make(name)
    kind, out = CASES[name][0], {}
    for it in range(1 if kind == "PPO" else 2):
        p = f"u{it}"
        if kind == "PPO":
            algo.collect_rollouts()
            algo.train()
            record(out, p + ".loss", {k: v for k, v in algo.logs.items() if k.startswith("train/")})
            record(out, p + ".buf", {k: v for k, v in vars(algo.buf).items() if isinstance(v, (torch.Tensor, dict))})
        else:
            record(out, p + ".loss", algo._update())
            record(out, p + ".horizon", getattr(algo, "_horizon", None))          # (use_autograd leaves none)
            record(out, p + ".rollout", algo._buf if kind == "SHAC" else getattr(algo, "_last_rollout", None))
        pol = algo.policy
        record(out, p + ".actor", dict(flat=pol.flat, grad=pol.grad, exp_avg=algo.exp_avg, exp_avg_sq=algo.exp_avg_sq))
        if kind == "SHAC":
            record(out, p + ".critic", dict(flat=algo.critic.flat, target=algo.critic_target.flat, grad=algo.critic.grad,
                                            exp_avg=algo.c_exp_avg, exp_avg_sq=algo.c_exp_avg_sq, stale_ext=algo._stale_ext,
                                            last_losses=algo._last_losses))
        record(out, p + ".env_state", env.get_observation()["state"])
    obs = env.get_observation()
    record(out, "predict.deterministic", algo.predict(obs, deterministic=True)[0])
    record(out, "predict.stochastic", algo.predict(obs)[0])
    if hasattr(algo, "_extractor"):            # the plain torch archive of the reference actor / SHAC
        record(out, "state", algo._state())
    with tempfile.TemporaryDirectory() as d:
        algo.save(os.path.join(d, "trainer"))          # no suffix: save and load add their own
        env2, _ = make(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            restored = type(algo).load(os.path.join(d, "trainer"), env2)
        record(out, "restored.flat", restored.policy.flat)
        env2.close()
    torch.cuda.synchronize()
    env.close()
    return out


def compare(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    bad = [f"{c}: {f}" for c in sorted(set(ra) | set(rb)) for f in sorted(set(ra.get(c, {})) | set(rb.get(c, {})))
           if ra.get(c, {}).get(f) != rb.get(c, {}).get(f)]
    for c in sorted(ra):
        digest = hashlib.sha256("".join(ra[c][f] for f in sorted(ra[c])).encode()).hexdigest()[:12]
        print(f"{c:24s} {len(ra[c]):3d} fields  {digest}  {'differs' if any(x.startswith(c + ': ') for x in bad) else 'equal'}")
    print(f"{len(ra)} cases, {sum(len(v) for v in ra.values())} fields, {len(bad)} differ")
    for x in bad:
        print("  differs:", x)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    result = {}
    for case in sys.argv[2:] or list(CASES):
        result[case] = run(case)
        print(f"{case}: {len(result[case])} fields", flush=True)
        with open(sys.argv[1], "w") as fh:          # (rewritten after every case: a run that stops early leaves what it had)
            json.dump(result, fh, indent=1, sort_keys=True)
