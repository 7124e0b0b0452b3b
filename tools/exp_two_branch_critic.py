"""What the generated two-branch twin-critic classes buy SHAC: one critic update (SHAC._critic_step_once) and one full iteration at the SHAC
leg's own size -- H = 32, N = 16 384 agents, M = 524 288 rows of the horizon buffer, gradient_steps = 5 -- timed with device events.
    python tools/exp_two_branch_critic.py [--root TREE] [--config racing2_gate,nav_target,nav_default] [--short]
--root: the tree whose visfly_amd is measured (default: this one); the same file times an older checkout, for the two columns of
profiles/two_branch_critic.txt.  --short: one warm-up iteration and one short window (a run under a kernel profiler, for the kernel names).
Configurations:
    racing2_gate  RacingEnv2, StateGateExtractor {state: [64, 32], gate: [32]}, pi = qf = [32]        (critic: _jit.PREBUILD_CRITIC["critic_gate"])
    nav_target    NavigationEnv, StateTargetExtractor {state: [64, 64], target: [32]}, pi = qf = [64]  (critic: PREBUILD_CRITIC["critic_nav"])
    nav_default   NavigationEnv, no policy_kwargs: [128, 64] x 2, 132 columns into qf0 / qf1 -- no chain class, layer by layer
One line per configuration: median and spread over the windows, which path the critic took, plugin launches per critic update."""
import argparse
import os
import sys
import warnings

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--config", default="racing2_gate,nav_target,nav_default")
ap.add_argument("--short", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

import visfly_amd.envs as E  # noqa: E402
from visfly_amd import _lib  # noqa: E402
from visfly_amd.shac import SHAC  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
DEV = "cuda:0"
N, H, STEPS = 16384, 32, 5
DYN = dict(integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)
GATES = [[2.0, 2.0, 0.9], [6.0, 2.0, 1.6], [5.0, -4.0, 1.0], [2.0, 0.0, 0.9]]


def setup(config):
    if config == "racing2_gate":
        env = E.RacingEnv2(num_agent_per_scene=N, seed=1, dynamics_kwargs=dict(DYN, action_type="thrust"), device=DEV, tensor_output=True,
                           requires_grad=True, max_episode_steps=256, gates=GATES)
        ext = {"state": [64, 32], "gate": [32]}
        pk = dict(features_extractor_class="StateGateExtractor", features_extractor_kwargs=dict(net_arch={k: dict(layer=v) for k, v in ext.items()}),
                  net_arch=dict(pi=[32], qf=[32]), activation_fn="relu")
        return env, pk
    env = E.NavigationEnv(num_agent_per_scene=N, seed=1, dynamics_kwargs=dict(DYN, action_type="bodyrate"), device=DEV, tensor_output=True,
                          requires_grad=True, max_episode_steps=256)
    if config == "nav_default":
        return env, None
    ext = {"state": [64, 64], "target": [32]}
    pk = dict(features_extractor_class="StateTargetExtractor", features_extractor_kwargs=dict(net_arch={k: dict(layer=v) for k, v in ext.items()}),
              net_arch=dict(pi=[64], qf=[64]), activation_fn="relu", share_features_extractor=False)
    return env, pk


def windows(fn, reps, n_windows):
    """ms per call of fn: n_windows windows of `reps` calls between two device events -> sorted list"""
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return sorted(out)


lib = _lib.lib()
print(f"tree {os.path.abspath(args.root)}   H {H} N {N} rows {H * N} gradient_steps {STEPS}   {torch.cuda.get_device_name(0)}")
for config in args.config.split(","):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        env, pk = setup(config)
        algo = SHAC(env, horizon=H, gradient_steps=STEPS, learning_rate=1e-3, seed=0, **({} if pk is None else {"policy_kwargs": pk}))
        env.reset()
        for _ in range(1 if args.short else 3):          # warm-up: every shape of the timed windows, the packed images, the buffers
            algo._update()
        torch.cuda.synchronize()
        b = algo._buf
        obs = {k: v.view(H * N, -1) for k, v in b["obs"].items()}
        action, target = b["action"].view(H * N, 4), b["returns"].view(-1)
        n0 = lib.vf_chain_plugin_launches()
        algo._critic_step_once(obs, action, target)
        torch.cuda.synchronize()
        per_step = lib.vf_chain_plugin_launches() - n0
        t_c = windows(lambda: algo._critic_step_once(obs, action, target), 5 if args.short else 40, 1 if args.short else 7)
        t_i = windows(algo._update, 2 if args.short else 12, 1 if args.short else 5)
        c = algo.critic
        path = ("fused step (vf_twin_q_update)" if c._fused_twin_q is not False and c._plan is not None and per_step else
                "layer by layer (wide)" if c._plan is None else "three launches: forward / loss / backward")
        finite = bool(torch.isfinite(c.flat).all()) and bool(torch.isfinite(algo.policy.flat).all())
        env.close()
    med = lambda t: t[len(t) // 2]
    notes = sorted({str(x.message)[:100] for x in w if "visfly_amd" in str(x.message)})
    print(f"{config:13s} critic update {med(t_c):8.3f} ms [{t_c[0]:.3f} .. {t_c[-1]:.3f}]   SHAC iteration {med(t_i):8.3f} ms [{t_i[0]:.3f} .. {t_i[-1]:.3f}]"
          f" = {H * N / med(t_i) * 1e3:.3e} env-steps/s   critic: {path}, chain_jit {bool(c.chain_jit)}, plugin launches per update {per_step},"
          f" finite {finite}", flush=True)
    for m in notes:
        print("       warning:", m)
