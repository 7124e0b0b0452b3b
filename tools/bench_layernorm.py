"""Times the two LayerNorm kernels (vf_layernorm_fwd / vf_layernorm_bwd, csrc/vf_layernorm.hip) next to torch's eager route for the same
quantity on the same card in the same process, and PPO's end-to-end rate with LayerNorm in every MLP.

    python tools/bench_layernorm.py [--out profiles/layernorm.txt] [--rows 25600] [--iters 4]

1. Kernels, M = 25 600 (PPO's minibatch), W in {64, 128, 256}, Tanh: warm-up, HIP events around `--launches` back-to-back launches,
   the median of `--repeats` such measurements and their spread (max - min) / median.  GB/s = the bytes the algorithm has to move
   (forward: z in, y / xhat / rstd out; backward: dy / y / xhat / rstd in, dz out) over the time.  At these sizes every array (6.5 -
   26 MB) fits the 256 MiB Infinity Cache and back-to-back launches re-read what the last one wrote, so the figure is a cache-resident
   rate, to be read against the neighbouring torch column and not against the HBM roof (6.3 TB/s measured).
   torch = F.layer_norm + tanh (2 launches) and autograd's backward of them.
2. PPO env-steps/s on bench.py's NavigationEnv configuration (32 768 agents, n_steps 256, batch 25 600, 5 epochs, [128, 64] extractors,
   [64, 64] trunks, ReLU): (a) ln / pi_ln / vf_ln on, (b) the same network without LayerNorm forced layer by layer
   (pol.fused = pol.fused_backward = False: the route (a) runs on, minus the norms), (c) the same network on its default fused path."""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfly_amd import _lib      # noqa: E402

DEV = "cuda:0"
EPS = 1e-3
ACT = 2          # VF_ACTIVATION_TANH


def timed(fn, launches, repeats, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / launches)
    med = statistics.median(us)
    return med, (max(us) - min(us)) / med


def kernels(a, lines):
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    lines.append(f"{'M':>7} {'W':>4} {'pass':>9} {'us':>8} {'spread':>7} {'GB/s':>8} {'torch us':>9} {'spread':>7} {'torch/ours':>10}")
    for M in [int(x) for x in a.rows.split(",")]:
        for W in (64, 128, 256):
            g = torch.Generator(device=DEV).manual_seed(W + M)
            z = torch.randn((M, W), device=DEV, generator=g)
            gamma, beta = 1 + 0.3 * torch.randn(W, device=DEV, generator=g), 0.2 * torch.randn(W, device=DEV, generator=g)
            dy = torch.randn((M, W), device=DEV, generator=g)
            y, xhat, rstd, dz = torch.empty_like(z), torch.empty_like(z), torch.empty(M, device=DEV), torch.empty_like(z)
            dgamma, dbeta = torch.empty(W, device=DEV), torch.empty(W, device=DEV)
            scratch = torch.empty(int(lib.vf_layernorm_bwd_scratch_floats(M, W)), device=DEV)
            ours = {
                "forward": lambda: _lib.check(lib.vf_layernorm_fwd(p(z), W, p(gamma), p(beta), EPS, p(y), W, p(xhat), W, p(rstd), M, W, ACT, st)),
                "backward": lambda: _lib.check(lib.vf_layernorm_bwd(p(dy), W, p(y), W, p(xhat), W, p(rstd), p(gamma), p(dz), W, p(dgamma),
                                                                    p(dbeta), M, W, ACT, 0, p(scratch), st)),
            }
            zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            fwd_t = lambda: torch.tanh(torch.nn.functional.layer_norm(zr, (W,), gr, br, EPS))
            yt = fwd_t()
            ref = {"forward": lambda: fwd_t().detach(), "backward": lambda: torch.autograd.grad(yt, (zr, gr, br), dy, retain_graph=True)}
            ours["forward"]()
            ours["backward"]()
            torch.cuda.synchronize()
            gz, gg, gb = ref["backward"]()
            assert torch.allclose(y, yt.detach(), rtol=1e-4, atol=1e-5) and torch.allclose(dz, gz, rtol=1e-4, atol=1e-5)
            assert torch.allclose(dgamma, gg, rtol=1e-4, atol=1e-3) and torch.allclose(dbeta, gb, rtol=1e-4, atol=1e-3)
            nbytes = {"forward": 4.0 * (3 * M * W + M), "backward": 4.0 * (4 * M * W + M)}
            for name in ("forward", "backward"):
                us, sp = timed(ours[name], a.launches, a.repeats)
                tus, tsp = timed(ref[name], a.launches, a.repeats)
                lines.append(f"{M:>7} {W:>4} {name:>9} {us:>8.1f} {sp:>6.1%} {nbytes[name] / us * 1e-3:>8.0f} {tus:>9.1f} {tsp:>6.1%} {tus / us:>10.2f}")
                print(lines[-1], flush=True)


def ppo_rate(a, lines):
    import bench
    from visfly_amd.envs import NavigationEnv
    from visfly_amd.ppo import PPO
    N = a.agents
    spawn = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}}]}}
    ext = lambda ln: dict(net_arch=dict(state=dict(layer=[128, 64], ln=ln), target=dict(layer=[128, 64], ln=ln)))
    arch = lambda ln: dict(pi=[64, 64], vf=[64, 64], pi_ln=ln, vf_ln=ln)
    cases = [("ln + pi_ln + vf_ln, layer by layer", True, False), ("no LayerNorm, forced layer by layer", False, False),
             ("no LayerNorm, default fused path", False, True)]
    lines.append(f"{'network':>38} {'env-steps/s':>12} {'s / iteration':>14}")
    for name, ln, fused in cases:
        env = NavigationEnv(num_agent_per_scene=N, seed=42, dynamics_kwargs=dict(bench.DYN_KW), random_kwargs=spawn, device=DEV,
                            max_episode_steps=256)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ppo = PPO(env, n_steps=256, batch_size=25600, n_epochs=5, learning_rate=1e-4, seed=0,
                      policy_kwargs=dict(activation_fn="relu", features_extractor_kwargs=ext(ln), net_arch=arch(ln)))
            if not fused:
                ppo.policy.fused = ppo.policy.fused_backward = False
                ppo.fused_rollout = False
            assert ppo.policy.ln == ln
            ppo.learn(256 * N)          # warm-up iteration
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ppo.learn(256 * N * a.iters)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
        lines.append(f"{name:>38} {256 * N * a.iters / el:>12.4e} {el / a.iters:>14.3f}")
        print(lines[-1], flush=True)
        env.close()
        del ppo, env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="25600")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--agents", type=int, default=32768)
    ap.add_argument("--iters", type=int, default=4, help="timed PPO iterations (rollout + train) per network")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_layernorm.py measures on the GPU; there is no fallback"
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; fp32; kernels: median of {a.repeats} x {a.launches} launches between HIP "
             f"events, spread = (max - min) / median; PPO: wall clock around {a.iters} iterations after one warm-up iteration"]
    kernels(a, lines)
    lines.append("")
    ppo_rate(a, lines)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
