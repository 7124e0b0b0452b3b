"""Update time per BPTT horizon with a Tanh actor next to the ReLU actor, at the bench leg's shape (bench.py --workload bptt: RacingEnv,
thrust, 16 384 agents, H = 64, the reference's two-head actor on its default sizes).  Both trainers live in one process and are timed in
alternating regions (a region = `--updates` updates ending in a device synchronise), so that drift of the box hits both alike; the spread
over the regions of one actor is the run-to-run noise the difference is read against.

    python tools/exp_bptt_activations.py [--agents 16384] [--regions 7] [--updates 8] [--out profiles/bptt_activations.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--updates", type=int, default=8)
    ap.add_argument("--activations", default="relu,tanh")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from visfly_amd.bptt import BPTT
    from visfly_amd.envs import RacingEnv
    N, H = a.agents, a.horizon
    dkw = dict(action_type="thrust", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)
    algos, fused = {}, {}
    for act in a.activations.split(","):
        env = RacingEnv(num_agent_per_scene=N, seed=42, dynamics_kwargs=dkw, device="cuda:0", max_episode_steps=256, requires_grad=True,
                        tensor_output=True)
        algo = BPTT(env, horizon=H, gamma=0.99, learning_rate=1e-3, seed=0, policy="MultiInputPolicy", policy_kwargs=dict(activation_fn=act))
        used = fused[act] = []
        for name in ("rollout_policy", "reverse_policy"):
            orig = getattr(env, name)
            setattr(env, name, lambda *x, _o=orig, _u=used, **k: _u.append(bool(_o(*x, **k))) or _u[-1])
        algo.learn(H * N * 2)          # warm-up: code objects, slot buffers, (cached) plugins
        torch.cuda.synchronize()
        algos[act] = algo
    times = {act: [] for act in algos}
    for _ in range(a.regions):
        for act, algo in algos.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            algo.learn(H * N * a.updates)
            torch.cuda.synchronize()
            times[act].append((time.perf_counter() - t0) / a.updates * 1e3)
    lines = [f"BPTT update time per horizon, RacingEnv thrust, {N} agents, H = {H}, reference actor (extractor [128, 64], trunks [64, 64] x 2)",
             f"{a.regions} alternating regions of {a.updates} updates each, host clock around a device synchronise; ms per update"]
    for act, ts in times.items():
        lines.append(f"{act:>10}: median {statistics.median(ts):.3f}  min {min(ts):.3f}  max {max(ts):.3f}  "
                     f"({H * N / statistics.median(ts) * 1e3:.3e} env-steps/s)  persistent launches: {all(fused[act]) and len(fused[act]) > 0}  "
                     f"regions: {' '.join(f'{t:.3f}' for t in ts)}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
