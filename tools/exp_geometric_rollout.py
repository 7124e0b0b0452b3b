"""us per control step of PPO.collect_rollouts() at the PPO leg's configuration (bench.py: NavigationEnv, 32 768 agents, n_steps = 256, the
built-in ReLU actor-critic), ONE persistent launch (fused_rollout = True) against the launch-by-launch loop (False) of the same build, for the
velocity and position action types (the geometric SO(3) controller) with the bodyrate pair as the yardstick.  All six trainers live in one
process and are timed in turn, `--reps` rounds after `--warmup` untimed ones, so that a drift of the machine reaches all of them alike.
Times by its own means (HIP events around `--rollouts` collect_rollouts() calls, device synchronised); bench.py is not involved.
python tools/exp_geometric_rollout.py [--agents N] [--steps T] [--reps R] [--warmup W] [--rollouts K] [--out FILE]"""
import argparse
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DEV = "cuda:0"
SPAWN = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}}]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rollouts", type=int, default=2, help="collect_rollouts() calls per timed window")
    ap.add_argument("--integrator", default="euler")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a measurement path does not fall back"
    from visfly_amd.envs import NavigationEnv
    from visfly_amd.ppo import PPO
    N, T = a.agents, a.steps
    runs = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # a fallback warning would mean the "persistent" column times the loop
        for act in ("bodyrate", "velocity", "position"):
            for fused in (True, False):
                dkw = dict(action_type=act, integrator=a.integrator, dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)
                env = NavigationEnv(num_agent_per_scene=N, seed=42, dynamics_kwargs=dkw, random_kwargs=SPAWN, device=DEV, max_episode_steps=256)
                ppo = PPO(env, n_steps=T, batch_size=25600, n_epochs=1, learning_rate=1e-4, seed=0, policy_kwargs=dict(activation_fn="relu"))
                ppo.fused_rollout = fused
                runs[(act, fused)] = ppo
        ms = {k: [] for k in runs}
        for rep in range(a.warmup + a.reps):
            for k, ppo in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.rollouts):
                    ppo.collect_rollouts()
                e1.record()
                e1.synchronize()
                assert ppo.fused_rollout is k[1], k
                if rep >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1))
    # the two paths of one action type leave the same buffers (tests/test_geometric_rollout_gpu.py holds that bit for bit at small sizes)
    same = {act: all(torch.equal(getattr(runs[(act, True)].buf, f), getattr(runs[(act, False)].buf, f)) for f in ("actions", "rewards", "values", "log_probs"))
            for act in ("bodyrate", "velocity", "position")}
    us = lambda v: v * 1000.0 / (a.rollouts * T)
    f = lambda v: f"{us(statistics.median(v)):7.2f} [{us(min(v)):7.2f} .. {us(max(v)):7.2f}]"
    lines = [f"# tools/exp_geometric_rollout.py: NavigationEnv, {N} agents, n_steps {T}, {a.integrator} / motor lag, built-in ReLU actor-critic; us per control "
             f"step of collect_rollouts() (HIP events around {a.rollouts} calls = {a.rollouts * T} steps), median [min .. max] of {a.reps} rounds after "
             f"{a.warmup} warm-up rounds, the six trainers in turn within every round",
             f"{'action type':12s} {'persistent us/step':>28s} {'loop us/step':>28s} {'loop / persistent':>18s} {'spread pers.':>13s} {'spread loop':>12s}  same buffers"]
    for act in ("bodyrate", "velocity", "position"):
        p, l = ms[(act, True)], ms[(act, False)]
        spread = lambda v: f"{100.0 * (max(v) - min(v)) / statistics.median(v):5.1f} %"
        lines.append(f"{act:12s} {f(p):>28s} {f(l):>28s} {statistics.median(l) / statistics.median(p):18.2f} {spread(p):>13s} {spread(l):>12s}  {same[act]}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    # the condition for keeping an instance: the persistent launch is not slower than the loop by more than the measured spread
    for act in ("velocity", "position"):
        p, l = ms[(act, True)], ms[(act, False)]
        assert statistics.median(p) <= statistics.median(l) + (max(l) - min(l)) + (max(p) - min(p)), (act, "the persistent launch is slower than the loop")


if __name__ == "__main__":
    main()
