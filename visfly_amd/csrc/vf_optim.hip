// vf_optim.hip -- the optimiser step on the flat parameter vector: gradient norm (vf_sumsq) and clip_grad_norm_ + Adam (vf_adam_step).
//
// Reference: th.nn.utils.clip_grad_norm_ + torch.optim.Adam.step as PPO.py:285-292 calls them (BPTT and SHAC do the same).  The
// per-parameter arithmetic is vf_adam_device.hpp.  k_sum2_partial / k_sum2_final (sum and sum of squares in fp64, fixed order)
// also serve the advantage normalisation of vf_ppo.hip, through sum2_launch (declared in vf_common.hpp).
#include "vf_common.hpp"
#include "vf_adam_device.hpp"

namespace vf {

// sum and sum of squares in fp64: per-block partials, then one block folds them (deterministic)
__global__ __launch_bounds__(kBlock) void k_sum2_partial(const float* __restrict__ x, long n, double* __restrict__ part)
{
    __shared__ double sh[2][4];
    double s = 0.0, ss = 0.0;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
        const double a = x[i];
        s += a;
        ss += a * a;
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = s; sh[1][w] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        part[2 * blockIdx.x + 1] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    }
}

__global__ void k_sum2_final(const double* __restrict__ part, int nblk, double* __restrict__ out2, float* out_ss_f32)
{
    // one wave: lane-strided partial sums, then the fixed shuffle tree (deterministic)
    double s = 0.0, ss = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) { s += part[2 * b]; ss += part[2 * b + 1]; }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (threadIdx.x == 0) {
        if (out2) { out2[0] = s; out2[1] = ss; }
        if (out_ss_f32) *out_ss_f32 = (float)ss;
    }
}

// sum of squares of a short vector (the flat gradient: tens of thousands of floats) in ONE block: fp64 lane sums,
// fixed-order tree -- one launch instead of the partial/final pair
__global__ __launch_bounds__(1024) void k_sumsq_block(const float* __restrict__ x, long n, float* __restrict__ out)
{
    __shared__ double sh[16];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;       // four independent chains, 16-byte loads (all in flight at once)
    const long n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? n >> 2 : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (long i = threadIdx.x; i < n4; i += 1024) {
        const float4 v = x4[i];
        s0 += (double)v.x * v.x; s1 += (double)v.y * v.y; s2 += (double)v.z * v.z; s3 += (double)v.w * v.w;
    }
    for (long i = 4 * n4 + threadIdx.x; i < n; i += 1024) s0 += (double)x[i] * x[i];
    double ss = wave_sum((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += sh[w];
        *out = (float)t;
    }
}

// clip_grad_norm_ + Adam with L2 weight decay (torch.optim.Adam semantics), PPO.py:285-292
__global__ __launch_bounds__(kBlock) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, long n, const float* __restrict__ sumsq,
                                                 const vf_adam_cfg c, float bc1, float bc2_sqrt)
{
    // the first element's operands are requested ahead of the norm's reduction: they do not depend on it, and a launch this small is
    // nothing but dependent round trips (r06: 5.1 us; the optimiser-step profile of round 6 under profiles/)
    const long i0 = (long)blockIdx.x * kBlock + threadIdx.x;
    float p0 = 0.0f, g0 = 0.0f, m0 = 0.0f, v0 = 0.0f;
    int4 o0 = make_int4(-1, -1, -1, -1);
    if (i0 < n) {
        p0 = p[i0];
        g0 = g[i0];
        m0 = m[i0];
        v0 = v[i0];
        if (c.pack_map) o0 = reinterpret_cast<const int4*>(c.pack_map)[i0];
    }
    float coef = 1.0f;
    if (c.max_grad_norm > 0.0f) {
        float ss;
        if (c.sumsq_partials) {     // every block sums the fold's partials (+ the uncovered tail) in the same fixed order
            __shared__ double sh[4];
            double a = 0.0;
            for (int i = threadIdx.x; i < c.n_sumsq_partials; i += kBlock) a += c.sumsq_partials[i];
            for (long i = c.sumsq_tail_from + threadIdx.x; i < n; i += kBlock) a += (double)g[i] * (double)g[i];
            a = wave_sum(a);
            if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
            __syncthreads();
            ss = (float)((sh[0] + sh[1]) + (sh[2] + sh[3]));
        } else {
            ss = *sumsq;
        }
        coef = adam_clip_coef(ss, c.max_grad_norm);
    }
    const float step = c.lr / bc1;
    if (i0 < n) {
        const float pn = adam_param(p0, g0, m0, v0, coef, c, step, bc2_sqrt);       // vf_adam_device.hpp
        m[i0] = m0;
        v[i0] = v0;
        p[i0] = pn;
        if (o0.x >= 0) c.packed[o0.x] = pn;
        if (o0.y >= 0) c.packed[o0.y] = pn;
        if (o0.z >= 0) c.packed[o0.z] = pn;
        if (o0.w >= 0) c.packed[o0.w] = pn;
    }
    for (long i = i0 + (long)gridDim.x * kBlock; i < n; i += (long)gridDim.x * kBlock) {
        float mi = m[i], vi = v[i];
        const float pn = adam_param(p[i], g[i], mi, vi, coef, c, step, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        p[i] = pn;
        if (c.pack_map) adam_refresh_packed(c, i, pn);
    }
}

void sum2_launch(const float* x, long n, double* part, double* out2, float* out_ss_f32, hipStream_t st)
{
    const int nblk = grid_for(n, 256);
    hipLaunchKernelGGL(k_sum2_partial, dim3(nblk), dim3(kBlock), 0, st, x, n, part);
    hipLaunchKernelGGL(k_sum2_final, dim3(1), dim3(64), 0, st, part, nblk, out2, out_ss_f32);
}

}  // namespace vf

extern "C" {

int vf_sumsq(const float* x, int64_t n, float* out1, float* scratch, vf_stream_t stream)
{
    if (!x || !out1 || !scratch || n <= 0) return vf::fail(VF_EINVAL, "vf_sumsq: bad argument");
    hipStream_t st = vf::as_stream(stream);
    if (n <= (1 << 20))        // the flat gradient of the actor-critic MLP: one block, one launch
        hipLaunchKernelGGL(vf::k_sumsq_block, dim3(1), dim3(1024), 0, st, x, (long)n, out1);
    else
        vf::sum2_launch(x, (long)n, reinterpret_cast<double*>(scratch), nullptr, out1, st);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* grad_sumsq,
                 const vf_adam_cfg* cfg, vf_stream_t stream)
{
    if (!param || !grad || !exp_avg || !exp_avg_sq || !cfg || n <= 0 || cfg->step <= 0 ||
        (cfg->max_grad_norm > 0 && !grad_sumsq && !cfg->sumsq_partials))
        return vf::fail(VF_EINVAL, "vf_adam_step: bad argument");
    if ((cfg->pack_map == nullptr) != (cfg->packed == nullptr))
        return vf::fail(VF_EINVAL, "vf_adam_step: pack_map and packed must be given together");
    float bc1, bc2_sqrt;
    vf::adam_bias(*cfg, &bc1, &bc2_sqrt);
    hipLaunchKernelGGL(vf::k_adam, dim3(vf::grid_for(n, 1024)), dim3(vf::kBlock), 0, vf::as_stream(stream), param, grad, exp_avg,
                       exp_avg_sq, (long)n, grad_sumsq, *cfg, bc1, bc2_sqrt);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

}  // extern "C"
