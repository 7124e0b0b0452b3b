"""ms per evaluation (visfly_amd.evaluate.evaluate_policy: reset + one deterministic episode per agent), persistent launch against the
launch-by-launch loop of the same build, in one process, alternating: HoverEnv, 16 384 agents, max_episode_steps = 256, the built-in ReLU
actor-critic, PPO's default (Tanh, a generated class) and SHAC's actor, each under a policy that lets most agents reach the time limit
(thrust head biased to hover) and one under which most crash early (thrust head at its minimum) -- what the wave exit buys.
python tools/exp_eval.py [--agents N] [--steps T] [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from visfly_amd.evaluate import evaluate_policy

DEV = "cuda:0"
DYN = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from visfly_amd.envs import HoverEnv
    from visfly_amd.ppo import PPO
    from visfly_amd.shac import SHAC
    mk = lambda seed, **kw: HoverEnv(num_agent_per_scene=a.agents, seed=seed, dynamics_kwargs=dict(DYN), device=DEV, tensor_output=True,
                                     max_episode_steps=a.steps, **kw)
    lines = [f"# tools/exp_eval.py: HoverEnv, {a.agents} agents, max_episode_steps {a.steps}, bodyrate / Euler / motor lag; ms per evaluate_policy() "
             f"(env.reset() + the episodes), HIP events, median [min .. max] of {a.reps} after one warm-up each, persistent and loop alternating",
             f"{'network':34s} {'policy':12s} {'at limit':>9s} {'mean len':>9s} {'persistent ms':>24s} {'loop ms':>24s} {'ratio':>6s}  same bits"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        models = [("PPO [128,64]x[64,64] ReLU (built in)", PPO(mk(1), n_steps=4, batch_size=4 * a.agents, n_epochs=1, seed=2, policy_kwargs=dict(activation_fn="relu"))),
                  ("PPO default (Tanh, generated)", PPO(mk(1), n_steps=4, batch_size=4 * a.agents, n_epochs=1, seed=2)),
                  ("SHAC actor (NetSacHover)", SHAC(mk(1, requires_grad=True), horizon=4, gradient_steps=1, seed=7))]
    for name, model in models:
        head = [ly for ly in model.policy.layers if ly.dst == "mean"][0]
        for regime, bias in (("hover", -0.3466), ("min thrust", -3.0)):      # tanh(-0.3466) = -1/3: about the hover thrust
            model.policy.bias(head)[0] = bias
            model.policy.mark_updated()
            envs = {"persistent": mk(11), "loop": mk(11)}
            ms, res = {"persistent": [], "loop": []}, {}
            for rep in range(a.reps + 1):
                for path in ("persistent", "loop"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r = evaluate_policy(model, envs[path], persistent=path == "persistent")
                    e1.record()
                    e1.synchronize()
                    assert r.path == path, (name, r.path)
                    res[path] = r
                    if rep:
                        ms[path].append(e0.elapsed_time(e1))
            same = torch.equal(res["persistent"].ep_length, res["loop"].ep_length) and torch.equal(
                res["persistent"].ep_return.view(torch.int32), res["loop"].ep_return.view(torch.int32))
            f = lambda v: f"{statistics.median(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
            at_limit = float((res["loop"].ep_length == a.steps).float().mean())
            lines.append(f"{name:34s} {regime:12s} {at_limit:9.3f} {res['loop'].mean_l:9.1f} {f(ms['persistent'])} {f(ms['loop'])} "
                         f"{statistics.median(ms['loop']) / statistics.median(ms['persistent']):6.2f}  {same}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
