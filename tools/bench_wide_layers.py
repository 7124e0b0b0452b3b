"""Times the three products of a wide linear layer (vf_linear_fwd / vf_linear_bwd_data / vf_linear_bwd_weight: 256 x 256 and
512 x 512 on the streamed-operand kernels, 128 x 128 on the weight-stationary ones for scale) against the reference's route for the
same product on the same card in the same process: torch.addmm + relu, and autograd's backward of it, fp32 with TF32 off.

    python tools/bench_wide_layers.py [--out profiles/wide_layers.txt] [--rows 25600,524288]

Per figure: warm-up, HIP events around `--launches` back-to-back launches, the median of `--repeats` such measurements and their spread
(max - min) / median.  The torch column times what autograd runs for the same quantity: forward = addmm + relu (2 launches),
data gradient = threshold_backward + mm, weight gradient = threshold_backward + mm + column sum."""
import argparse
import statistics
import sys
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visfly_amd import _lib      # noqa: E402

PEAK_TF = 157.3          # fp32 v_mfma_f32_32x32x2_f32 dense peak, the figure bench.py's rooflines use
DEV = "cuda:0"


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="25600,524288", help="M: PPO's minibatch, 16384 agents x 32 steps of a BPTT horizon")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; fp32, allow_tf32 off; median of {a.repeats} x {a.launches} launches "
             f"between HIP events, spread = (max - min) / median; peak = {PEAK_TF} TFLOP/s (fp32 MFMA)",
             f"{'M':>7} {'K x No':>9} {'product':>12} {'kernel':>8} {'us':>9} {'spread':>7} {'TFLOP/s':>8} {'of peak':>8} {'torch us':>9} {'spread':>7} {'torch/ours':>10}"]
    for M in [int(x) for x in a.rows.split(",")]:
        for K, No in [(128, 128), (256, 256), (512, 512)]:
            g = torch.Generator(device=DEV).manual_seed(K + M)
            X = torch.randn((M, K), device=DEV, generator=g)
            W = torch.randn((No, K), device=DEV, generator=g) / np.sqrt(K)
            b = torch.randn(No, device=DEV, generator=g)
            dY = torch.randn((M, No), device=DEV, generator=g)
            Y, dX = torch.empty((M, No), device=DEV), torch.empty((M, K), device=DEV)
            dW, db = torch.empty((No, K), device=DEV), torch.empty(No, device=DEV)
            scratch = torch.empty(int(lib.vf_linear_bwd_scratch_floats(M, K, No)), device=DEV)
            p = lambda t: t.data_ptr()
            kern = "wide" if lib.vf_linear_is_wide(K, No) else "resident"
            ours = {
                "forward": lambda: _lib.check(lib.vf_linear_fwd(p(X), K, p(W), p(b), p(Y), No, M, K, No, 1, st)),
                "data grad": lambda: _lib.check(lib.vf_linear_bwd_data(p(dY), No, p(Y), No, p(W), p(dX), K, M, K, No, 0, 1, st)),
                "weight grad": lambda: _lib.check(lib.vf_linear_bwd_weight(p(dY), No, p(Y), No, p(X), K, p(dW), p(db), M, K, No, p(scratch), 1, st)),
            }
            Wt = W.t()
            Yt = torch.relu(torch.addmm(b, X, Wt))
            ref = {
                "forward": lambda: torch.relu(torch.addmm(b, X, Wt)),
                "data grad": lambda: torch.mm(torch.ops.aten.threshold_backward(dY, Yt, 0.0), W),
                "weight grad": lambda: (lambda d: (torch.mm(d.t(), X), d.sum(0)))(torch.ops.aten.threshold_backward(dY, Yt, 0.0)),
            }
            ours["forward"]()
            torch.cuda.synchronize()
            assert torch.allclose(Y, Yt, rtol=1e-4, atol=1e-4)
            tot_o = tot_t = 0.0
            flop = 2.0 * M * K * No
            for name in ("forward", "data grad", "weight grad"):
                us, sp = timed(ours[name], a.launches, a.repeats)
                tus, tsp = timed(ref[name], a.launches, a.repeats)
                tot_o, tot_t = tot_o + us, tot_t + tus
                tf = flop / us * 1e-6
                lines.append(f"{M:>7} {K:>4}x{No:<4} {name:>12} {kern:>8} {us:>9.1f} {sp:>6.1%} {tf:>8.1f} {tf / PEAK_TF:>8.1%} {tus:>9.1f} {tsp:>6.1%} {tus / us:>10.2f}")
                print(lines[-1], flush=True)
            tf = 3 * flop / tot_o * 1e-6
            lines.append(f"{M:>7} {K:>4}x{No:<4} {'sum of 3':>12} {kern:>8} {tot_o:>9.1f} {'':>7} {tf:>8.1f} {tf / PEAK_TF:>8.1%} {tot_t:>9.1f} {'':>7} {tot_t / tot_o:>10.2f}")
            print(lines[-1], flush=True)
            del X, W, dY, Y, dX, scratch, Yt
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
