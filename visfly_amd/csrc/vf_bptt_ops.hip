// vf_bptt_ops.hip -- the elementwise glue of the first-order trainers, one thread per row, HBM-bound:
//   k_td_returns                         TD-lambda returns (utils/algorithms/common.py:893-923); SHAC's critic targets
//   k_reparam_fwd / _bwd                 a = tanh(mean + exp(log_std) eps) and its reverse (BPTT.py:107-134)
//   k_bptt_accumulate[_checkpoint]       discounted-loss bookkeeping of one step (BPTT.py:123-124), optionally with the state checkpoint
//   k_noise_fill                         the eps rows both trainers draw ahead of a roll-out (Philox stream of vf_common.hpp)
// vf_shac.hip holds what is specific to SHAC; the fused per-horizon kernels are vf_bptt_rollout.hip / vf_bptt_reverse.hip.
#include "vf_common.hpp"

namespace vf {

// TD-lambda returns (utils/algorithms/common.py:893-923): same access pattern as GAE
__global__ __launch_bounds__(kBlock) void k_td_returns(const float* __restrict__ r, const unsigned char* __restrict__ done,
                                                       const unsigned char* __restrict__ ep_done,
                                                       const float* __restrict__ nv, float* __restrict__ ret, int H, int N,
                                                       float gamma, float lamda, float lg, float oml)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    float Ai = 0.0f, lam = 1.0f;
    float Bi = nv[(size_t)(H - 1) * N + i] * (done[(size_t)(H - 1) * N + i] ? 0.0f : 1.0f);
    for (int t = H - 1; t >= 0; --t) {
        const size_t o = (size_t)t * N + i;
        const float active = done[o] ? 0.0f : 1.0f, dm = done[o] ? 1.0f : 0.0f, ea = ep_done[o] ? 0.0f : 1.0f;
        lam = lam * lamda * active + dm;
        Ai = active * ((lg * Ai + gamma * nv[o]) + ((1.0f - lam) / oml) * r[o]);
        Bi = gamma * (nv[o] * dm * ea + Bi * active) + r[o];
        ret[o] = oml * Ai + lam * Bi;
    }
}

// ---- first-order policy optimisation glue (BPTT.py:107-134): reparameterised action, its reverse, loss bookkeeping ----
// a = tanh(mean + exp(log_std) * eps)   (reparameterised squashed Gaussian, one thread per row)
__global__ __launch_bounds__(kBlock) void k_reparam_fwd(const float4* __restrict__ mean, const float* __restrict__ log_std,
                                                        const float4* __restrict__ eps, float4* __restrict__ action, int N)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const float4 m = mean[i], e = eps[i];
    action[i] = make_float4(tanhf(m.x + expf(log_std[0]) * e.x), tanhf(m.y + expf(log_std[1]) * e.y),
                            tanhf(m.z + expf(log_std[2]) * e.z), tanhf(m.w + expf(log_std[3]) * e.w));
}

// d_mean = d_action * (1 - a^2);  g_log_std += d_mean * exp(log_std) * eps   (per row; summed over rows by the caller)
__global__ __launch_bounds__(kBlock) void k_reparam_bwd(const float4* __restrict__ d_action, const float4* __restrict__ action,
                                                        const float* __restrict__ log_std, const float4* __restrict__ eps,
                                                        float4* __restrict__ d_mean, float4* __restrict__ g_log_std, int N)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const float4 da = d_action[i], a = action[i], e = eps[i];
    const float4 dm = make_float4(da.x * (1.0f - a.x * a.x), da.y * (1.0f - a.y * a.y), da.z * (1.0f - a.z * a.z),
                                  da.w * (1.0f - a.w * a.w));
    d_mean[i] = dm;
    float4 g = g_log_std[i];
    g.x += dm.x * expf(log_std[0]) * e.x; g.y += dm.y * expf(log_std[1]) * e.y;
    g.z += dm.z * expf(log_std[2]) * e.z; g.w += dm.w * expf(log_std[3]) * e.w;
    g_log_std[i] = g;
}

// loss_i += -reward_i * disc_i; d_reward_i = -disc_i * scale; disc_i <- disc_i * gamma * ~done_i + done_i   (BPTT.py:123-124)
__global__ __launch_bounds__(kBlock) void k_bptt_accumulate(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                            float* __restrict__ disc, float* __restrict__ loss,
                                                            float* __restrict__ d_reward, float gamma, float scale, int N)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const float d = disc[i];
    loss[i] = loss[i] + -1.0f * reward[i] * d;
    d_reward[i] = -d * scale;
    const float dn = done[i] ? 1.0f : 0.0f;
    disc[i] = d * gamma * (1.0f - dn) + dn;
}

// k_bptt_accumulate + the state checkpoint of the NEXT step (a plain slab -> tape row copy) in one launch: both sit between
// env step t and env step t + 1 of the BPTT forward pass, one launch boundary (~5 us at 16 384 agents) instead of two
__global__ __launch_bounds__(kBlock) void k_bptt_accumulate_checkpoint(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                                       float* __restrict__ disc, float* __restrict__ loss,
                                                                       float* __restrict__ d_reward, float gamma, float scale, int N,
                                                                       const float4* __restrict__ slab, float4* __restrict__ tape,
                                                                       long long n4)
{
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    for (long long j = tid; j < n4; j += stride) tape[j] = slab[j];
    if (tid < N) {
        const int i = (int)tid;
        const float d = disc[i];
        loss[i] = loss[i] + -1.0f * reward[i] * d;
        d_reward[i] = -d * scale;
        const float dn = done[i] ? 1.0f : 0.0f;
        disc[i] = d * gamma * (1.0f - dn) + dn;
    }
}

// vf_noise_fill: eps[t][i] = the four normals of the Philox block {row0 + i, step0 + t, kTagRowNoise}.  One thread per (t, agent), rows
// coalesced: a wave stores 1 KiB contiguous per instruction.  Pure streaming write (non-temporal: nobody re-reads it from this launch)
__global__ __launch_bounds__(kBlock) void k_noise_fill(float4* __restrict__ eps, int N, unsigned row0, unsigned long long seed,
                                                       unsigned long long step0)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const unsigned t = blockIdx.y;
    float e[4];
    philox_normal4(row0 + (unsigned)i, step0 + t, kTagRowNoise, seed, e);
    float4* dst = eps + (size_t)t * N + i;
    __builtin_nontemporal_store(e[0], &dst->x);
    __builtin_nontemporal_store(e[1], &dst->y);
    __builtin_nontemporal_store(e[2], &dst->z);
    __builtin_nontemporal_store(e[3], &dst->w);
}

}  // namespace vf

extern "C" {

int vf_td_returns(const float* r, const uint8_t* done, const uint8_t* episode_done, const float* next_value, float* returns,
                  int32_t H, int32_t N, double gamma, double lamda, vf_stream_t stream)
{
    if (!r || !done || !next_value || !returns || H <= 0 || N <= 0) return vf::fail(VF_EINVAL, "vf_td_returns: bad argument");
    hipLaunchKernelGGL(vf::k_td_returns, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream), r, done,
                       episode_done ? episode_done : done, next_value, returns, H, N, (float)gamma, (float)lamda,
                       (float)(lamda * gamma), (float)(1.0 - lamda));
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_reparam_fwd(const float* mean, const float* log_std, const float* eps, float* action, int32_t N, vf_stream_t stream)
{
    if (!mean || !log_std || !eps || !action || N <= 0) return vf::fail(VF_EINVAL, "vf_reparam_fwd: bad argument");
    hipLaunchKernelGGL(vf::k_reparam_fwd, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream),
                       reinterpret_cast<const float4*>(mean), log_std, reinterpret_cast<const float4*>(eps),
                       reinterpret_cast<float4*>(action), N);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_reparam_bwd(const float* d_action, const float* action, const float* log_std, const float* eps, float* d_mean,
                   float* g_log_std, int32_t N, vf_stream_t stream)
{
    if (!d_action || !action || !log_std || !eps || !d_mean || !g_log_std || N <= 0)
        return vf::fail(VF_EINVAL, "vf_reparam_bwd: bad argument");
    hipLaunchKernelGGL(vf::k_reparam_bwd, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream),
                       reinterpret_cast<const float4*>(d_action), reinterpret_cast<const float4*>(action), log_std,
                       reinterpret_cast<const float4*>(eps), reinterpret_cast<float4*>(d_mean),
                       reinterpret_cast<float4*>(g_log_std), N);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_bptt_accumulate(const float* reward, const uint8_t* done, float* disc, float* loss, float* d_reward, float gamma,
                       float scale, int32_t N, vf_stream_t stream)
{
    if (!reward || !done || !disc || !loss || !d_reward || N <= 0) return vf::fail(VF_EINVAL, "vf_bptt_accumulate: bad argument");
    hipLaunchKernelGGL(vf::k_bptt_accumulate, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream), reward, done,
                       disc, loss, d_reward, gamma, scale, N);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_bptt_accumulate_checkpoint(const float* reward, const uint8_t* done, float* disc, float* loss, float* d_reward, float gamma,
                                  float scale, int32_t N, const float* slab, float* tape_row, int64_t slab_floats, vf_stream_t stream)
{
    if (!reward || !done || !disc || !loss || !d_reward || N <= 0 || !slab || !tape_row || slab_floats <= 0 || (slab_floats & 3))
        return vf::fail(VF_EINVAL, "vf_bptt_accumulate_checkpoint: bad argument");
    if ((reinterpret_cast<uintptr_t>(slab) | reinterpret_cast<uintptr_t>(tape_row)) & 15)
        return vf::fail(VF_EINVAL, "vf_bptt_accumulate_checkpoint: slab and tape row must be 16-byte aligned");
    const long long n4 = slab_floats / 4;
    long long blocks = (n4 + vf::kBlock - 1) / vf::kBlock;
    if (blocks < vf::blocks_for(N)) blocks = vf::blocks_for(N);
    if (blocks > 4096) blocks = 4096;                    // grid-stride copy; 4096 x 256 threads cover the accumulate for N <= 1 M
    if ((long long)N > blocks * vf::kBlock) return vf::fail(VF_EINVAL, "vf_bptt_accumulate_checkpoint: N too large for one launch");
    hipLaunchKernelGGL(vf::k_bptt_accumulate_checkpoint, dim3((unsigned)blocks), dim3(vf::kBlock), 0, vf::as_stream(stream), reward, done,
                       disc, loss, d_reward, gamma, scale, N, reinterpret_cast<const float4*>(slab), reinterpret_cast<float4*>(tape_row), n4);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_noise_fill(float* eps, int32_t T, int32_t N, uint64_t row0, uint64_t seed, uint64_t step0, vf_stream_t stream)
{
    if (!eps || T <= 0 || N <= 0 || T > 65535) return vf::fail(VF_EINVAL, "vf_noise_fill: null output, T outside [1, 65535] or N <= 0");
    if (row0 + (uint64_t)N > (uint64_t)1 << 32) return vf::fail(VF_EINVAL, "vf_noise_fill: rows [row0, row0 + N) do not fit the 32-bit counter word");
    hipLaunchKernelGGL(vf::k_noise_fill, dim3(vf::blocks_for(N), T), dim3(vf::kBlock), 0, vf::as_stream(stream),
                       reinterpret_cast<float4*>(eps), N, (unsigned)row0, (unsigned long long)seed, (unsigned long long)step0);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

}  // extern "C"
