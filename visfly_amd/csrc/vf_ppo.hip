// vf_ppo.hip -- PPO's buffer operations on the device (gfx950): GAE scan, advantage normalisation, minibatch gather, roll-out
// post-processing with the deferred TimeLimit bootstrap, episode statistics, the squashed-Gaussian head sampler, the
// clipped-surrogate loss, and vf_ppo_update (the fused minibatch step of the chain class table plus its statistics fold).
//
// Reference: utils/algorithms/PPO.py:177-337 (train), SB3 2.2.1 RolloutBuffer / collect_rollouts (mirrored in
// utils/algorithms/common.py:97-132), utils/policies/policies.py:195-254.  The reference runs these as torch ops over the
// roll-out buffer; here each piece is one launch.  What PPO runs between them lives in units of its own: the networks in
// vf_linear.hip / vf_mlp_tile.hip / vf_mlp_chain.hip, clip + Adam in vf_optim.hip (whose fp64 sum kernels the advantage
// normalisation borrows through sum2_launch), the fused roll-out in vf_ppo_rollout.hip.
#include "vf_common.hpp"
#include "vf_ppo_device.hpp"

namespace vf {

// ------------------------------------------------------------------------------------------------
// GAE: thread per env walks T backwards; loads are coalesced across envs (common.py:119-132)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_gae(const float* __restrict__ r, const float* __restrict__ v,
                                                const float* __restrict__ es, const float* __restrict__ lastv,
                                                const float* __restrict__ dones, float* __restrict__ adv,
                                                float* __restrict__ ret, int T, int N, float gamma, float gl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    float last = 0.0f;
    float nnt = 1.0f - dones[i];
    float nv = lastv[i];
    for (int t = T - 1; t >= 0; --t) {
        const size_t o = (size_t)t * N + i;
        const float vt = v[o];
        const float delta = r[o] + gamma * nv * nnt - vt;
        last = delta + gl * nnt * last;
        adv[o] = last;
        ret[o] = last + vt;
        nnt = 1.0f - es[o];  // for step t-1: next_non_terminal = 1 - episode_starts[t]
        nv = vt;
    }
}

// (A - mean) / (std_unbiased + 1e-8)   (PPO.py:217-220)
__global__ __launch_bounds__(kBlock) void k_adv_apply(const float* __restrict__ a, float* __restrict__ out, long n,
                                                      const double* __restrict__ sums, double count)
{
    const double mean = sums[0] / count;
    double var = (sums[1] - sums[0] * mean) / (count - 1.0);
    var = var > 0.0 ? var : 0.0;
    const float m = (float)mean, sd = (float)sqrt(var) + 1e-8f;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) out[i] = (a[i] - m) / sd;
}

// segmented variant: one block per minibatch (contiguous slice of the shuffled epoch buffer)
__global__ __launch_bounds__(kBlock) void k_adv_seg_sums(const float* __restrict__ x, long seg_len, double* __restrict__ sums)
{
    __shared__ double sh[2][4];
    const float* xs = x + (size_t)blockIdx.x * seg_len;
    double s = 0.0, ss = 0.0;
    for (long i = threadIdx.x; i < seg_len; i += kBlock) {
        const double a = xs[i];
        s += a;
        ss += a * a;
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = s; sh[1][w] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[2 * blockIdx.x] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        sums[2 * blockIdx.x + 1] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    }
}

__global__ __launch_bounds__(kBlock) void k_adv_seg_apply(const float* __restrict__ a, float* __restrict__ out, long seg_len,
                                                          const double* __restrict__ sums, double count)
{
    const double s0 = sums[2 * blockIdx.y], s1 = sums[2 * blockIdx.y + 1];
    const double mean = s0 / count;
    double var = (s1 - s0 * mean) / (count - 1.0);
    var = var > 0.0 ? var : 0.0;
    const float m = (float)mean, sd = (float)sqrt(var) + 1e-8f;
    const size_t base = (size_t)blockIdx.y * seg_len;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < seg_len; i += (long)gridDim.x * kBlock)
        out[base + i] = (a[base + i] - m) / sd;
}

// ------------------------------------------------------------------------------------------------
// Squashed diagonal Gaussian head
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_head_sample(const float4* __restrict__ mean, const float* __restrict__ log_std,
                                                        float4* __restrict__ action, float* __restrict__ logp, int M,
                                                        unsigned row0, unsigned long long seed, unsigned long long step, int deterministic)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    float4 a;
    logp[i] = head_sample_row(mean[i], log_std, row0 + (unsigned)i, seed, step, deterministic, a);
    action[i] = a;
}

// the same head with the caller's noise rows instead of Philox (vf_head_sample_eps)
__global__ __launch_bounds__(kBlock) void k_head_sample_eps(const float4* __restrict__ mean, const float* __restrict__ log_std,
                                                            const float4* __restrict__ eps, float4* __restrict__ action,
                                                            float* __restrict__ logp, int M)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    const float4 m4 = mean[i], e4 = eps[i];
    const float mu[4] = {m4.x, m4.y, m4.z, m4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
    const float ls[4] = {log_std[0], log_std[1], log_std[2], log_std[3]};
    float4 a;
    logp[i] = head_row_from_noise(mu, ls, e, a);
    action[i] = a;
}

// PPO clipped surrogate + value MSE + "entropy" (= mean log-prob for the squashed head), PPO.py:210-263
__global__ __launch_bounds__(kBlock) void k_ppo_loss(const float4* __restrict__ mean, const float* __restrict__ value,
                                                     const float* __restrict__ log_std, const float4* __restrict__ action,
                                                     const float* __restrict__ old_lp, const float* __restrict__ adv,
                                                     const float* __restrict__ ret, float4* __restrict__ d_mean,
                                                     float* __restrict__ d_value, float* __restrict__ part, int M,
                                                     const vf_ppo_loss_cfg cfg)
{
    __shared__ float sh[4][kStats];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    float st[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i < M) {
        const float4 m4 = mean[i], a4 = action[i];
        const float mu[4] = {m4.x, m4.y, m4.z, m4.w}, a[4] = {a4.x, a4.y, a4.z, a4.w};
        const float ls[4] = {log_std[0], log_std[1], log_std[2], log_std[3]};
        float dm[4], dvl;
        ppo_row(mu, value[i], ls, a, old_lp[i], adv[i], ret[i], cfg, dm, dvl, st, i);
        d_mean[i] = make_float4(dm[0], dm[1], dm[2], dm[3]);
        d_value[i] = dvl;
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float s = wave_sumf(st[k]);
        if ((threadIdx.x & 63) == 0) sh[w][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * kStats + k] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
    }
}

__global__ __launch_bounds__(1024) void k_fold_stats(const float* __restrict__ part, int nblk, float* __restrict__ stats,
                                                     float* __restrict__ d_log_std_out, float* __restrict__ stats_accum)
{
    // 16 stats x 64 lanes (1024 threads, one wave per statistic): lane-strided sums over the partial rows, then a
    // shuffle tree over the wave -- fixed order, deterministic
    const int k = threadIdx.x >> 6, sl = threadIdx.x & 63;
    float s = 0.0f;
    if (k < 9)
        for (int b = sl; b < nblk; b += 64) s += part[(size_t)b * kStats + k];
    s = wave_sumf(s);
    if (sl == 0) {
        stats[k] = s;
        if (d_log_std_out && k >= 5 && k < 9) d_log_std_out[k - 5] = s;
        if (stats_accum) stats_accum[k] += s;
    }
}

// dst[i, :] = src[perm[i], :] for every field (blockIdx.y); one thread per output element: coalesced stores, the w
// consecutive words of a source row read by consecutive lanes
__global__ __launch_bounds__(kBlock) void k_gather_rows(const vf_gather_fields f, const int64_t* __restrict__ perm, long rows)
{
    // a row's w floats on 2^ceil(log2 w) consecutive lanes: row / column by shift and mask (the flat form `idx / w` was a 64-bit division
    // per element -- 1.1 ms per shuffle of the 8.4 M-row PPO buffer), the permutation entry is read once per row and broadcast by the cache
    const int fi = blockIdx.y;
    const int w = f.width[fi];
    const float* __restrict__ src = f.src[fi];
    float* __restrict__ dst = f.dst[fi];
    const int lg = w > 1 ? 32 - __clz(w - 1) : 0;
    const int c = (int)(threadIdx.x & ((1u << lg) - 1u));
    const long per_block = kBlock >> lg;                      // rows per block and pass (lg <= 8: VF widths are <= 256)
    for (long r = (long)blockIdx.x * per_block + (threadIdx.x >> lg); r < rows; r += (long)gridDim.x * per_block)
        if (c < w) dst[r * w + c] = src[perm[r] * w + c];
}

// reward + gamma * V(terminal obs) on truncated episodes; next episode_start = float(done)   (SB3 collect_rollouts)
__global__ __launch_bounds__(kBlock) void k_rollout_post(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                         const uint8_t* __restrict__ ep_flags, const float* __restrict__ tv, float gamma,
                                                         float* __restrict__ reward_out, float* __restrict__ next_start, int N)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const bool d = done[i] != 0;
    // a select, not a multiply by 0 / 1: SB3 adds to the truncated rows only, so every other reward keeps its bits (-0.0 stays -0.0,
    // a non-finite terminal value of a row that did not truncate never reaches its reward), as in k_rollout_post_collect + scatter
    const float r = reward[i];
    reward_out[i] = (d && (ep_flags[i] & VF_EP_TRUNCATED)) ? r + gamma * tv[i] : r;
    next_start[i] = d ? 1.0f : 0.0f;
}

// The same bookkeeping with the TimeLimit bootstrap DEFERRED: instead of evaluating V(terminal observation) for all N agents
// at every step (a second policy forward per rollout step), the rows that need it -- done && truncated, a handful per step -- are
// appended to a compact list (flat buffer index t * N + i and the terminal observation rows); after the rollout ONE value
// forward over the collected rows and k_bootstrap_scatter add gamma * V to the listed rewards.  The list order depends on the
// atomic cursor, the result does not: every entry is independent and names a distinct reward.
__global__ __launch_bounds__(kBlock) void k_rollout_post_collect(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                                 const uint8_t* __restrict__ ep_flags, float* __restrict__ reward_out,
                                                                 float* __restrict__ next_start, const float* __restrict__ obs0,
                                                                 const float* __restrict__ obs1, int w0, int w1, int* __restrict__ cursor,
                                                                 int capacity, int* __restrict__ idx_list, float* __restrict__ rows0,
                                                                 float* __restrict__ rows1, int flat_base, int N,
                                                                 const float* __restrict__ ep_return, const int* __restrict__ ep_length,
                                                                 float* __restrict__ stat)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const bool d = done[i] != 0;
    reward_out[i] = reward[i];
    next_start[i] = d ? 1.0f : 0.0f;
    if (d && stat) {   // per-agent episode statistics (PPO._dump_logs): every thread owns its agent's four accumulators, summed once per rollout
        float4* a = reinterpret_cast<float4*>(stat) + i;
        float4 v = *a;
        v.x += 1.0f;
        v.y += ep_return[i];
        v.z += (float)ep_length[i];
        v.w += (ep_flags[i] & VF_EP_SUCCESS) ? 1.0f : 0.0f;
        *a = v;
    }
    if (d && (ep_flags[i] & VF_EP_TRUNCATED)) {
        const int slot = atomicAdd(cursor, 1);
        if (slot < capacity) {
            idx_list[slot] = flat_base + i;
            for (int k = 0; k < w0; ++k) rows0[(size_t)slot * w0 + k] = obs0[(size_t)i * w0 + k];
            for (int k = 0; k < w1; ++k) rows1[(size_t)slot * w1 + k] = obs1[(size_t)i * w1 + k];
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_bootstrap_scatter(const int* __restrict__ idx_list, const float* __restrict__ values,
                                                              int count, float gamma, float* __restrict__ rewards_flat)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    const int at = idx_list[j];
    rewards_flat[at] = rewards_flat[at] + gamma * values[j];      // same rounding as reward + (gamma * tv) of k_rollout_post
}

// episode statistics of one env step for the training log (PPO._dump_logs: rollout/ep_rew_mean, ep_len_mean, success rate;
// PPO.py:392-414): acc += {episodes finished, sum of their returns, sum of their lengths, successes}.  One block, fixed
// reduction order, no host synchronisation in the rollout loop.
__global__ __launch_bounds__(1024) void k_episode_stats(const uint8_t* __restrict__ done, const float* __restrict__ ep_return,
                                                        const int32_t* __restrict__ ep_length, const uint8_t* __restrict__ ep_flags,
                                                        double* __restrict__ acc, int N)
{
    __shared__ double sh[4][16];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    // branch-free and unrolled: the loads of eight strides are in flight together (a `if (done[i])` around the other
    // three loads made every iteration a dependent round trip: 16 us for 32 768 agents)
    for (int i0 = threadIdx.x; i0 < N; i0 += 8 * 1024) {
        uint8_t d[8], f[8];
        float r[8];
        int32_t l[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 1024, ic = i < N ? i : N - 1;
            d[u] = i < N ? done[ic] : (uint8_t)0;
            r[u] = ep_return[ic];
            l[u] = ep_length[ic];
            f[u] = ep_flags[ic];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double on = d[u] ? 1.0 : 0.0;
            v[0] += on;
            v[1] += d[u] ? (double)r[u] : 0.0;
            v[2] += d[u] ? (double)l[u] : 0.0;
            v[3] += (d[u] && (f[u] & VF_EP_SUCCESS)) ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += sh[threadIdx.x][w];
        acc[threadIdx.x] += t;
    }
}

}  // namespace vf

extern "C" {

int vf_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values,
           const float* dones, float* adv, float* ret, int32_t T, int32_t N, double gamma, double lam, vf_stream_t stream)
{
    if (!rewards || !values || !episode_starts || !last_values || !dones || !adv || !ret || T <= 0 || N <= 0)
        return vf::fail(VF_EINVAL, "vf_gae: bad argument");
    hipLaunchKernelGGL(vf::k_gae, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream), rewards, values,
                       episode_starts, last_values, dones, adv, ret, T, N, (float)gamma, (float)(gamma * lam));
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_adv_normalize(const float* adv, float* out, int64_t n, int64_t count, double* sums_inout, float* scratch,
                     int32_t phase, vf_stream_t stream)
{
    if (!adv || !out || !scratch || n <= 0 || count < 2 || phase < 0 || phase > 2)
        return vf::fail(VF_EINVAL, "vf_adv_normalize: bad argument");
    hipStream_t st = vf::as_stream(stream);
    double* part = reinterpret_cast<double*>(scratch);  // [2*nblk] + 2 doubles for the sums
    double* sums = sums_inout ? sums_inout : part + 2 * 256;
    if (phase == 0 || phase == 2) vf::sum2_launch(adv, (long)n, part, sums, nullptr, st);
    if (phase == 1 || phase == 2)
        hipLaunchKernelGGL(vf::k_adv_apply, dim3(vf::grid_for(n, 1024)), dim3(vf::kBlock), 0, st, adv, out, (long)n, sums,
                           (double)count);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_adv_normalize_segments(const float* adv, float* out, int32_t n_seg, int64_t seg_len, int64_t count, double* sums,
                              int32_t phase, vf_stream_t stream)
{
    if (!adv || !out || !sums || n_seg <= 0 || n_seg > 65535 || seg_len <= 0 || count < 2 || phase < 0 || phase > 2)
        return vf::fail(VF_EINVAL, "vf_adv_normalize_segments: bad argument");
    hipStream_t st = vf::as_stream(stream);
    if (phase == 0 || phase == 2)
        hipLaunchKernelGGL(vf::k_adv_seg_sums, dim3(n_seg), dim3(vf::kBlock), 0, st, adv, (long)seg_len, sums);
    if (phase == 1 || phase == 2) {
        const int bx = (int)((seg_len + 4 * vf::kBlock - 1) / (4 * vf::kBlock));
        hipLaunchKernelGGL(vf::k_adv_seg_apply, dim3(bx < 64 ? bx : 64, n_seg), dim3(vf::kBlock), 0, st, adv, out, (long)seg_len,
                           sums, (double)count);
    }
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_episode_stats(const uint8_t* done, const float* ep_return, const int32_t* ep_length, const uint8_t* ep_flags, double* acc4,
                     int32_t N, vf_stream_t stream)
{
    if (!done || !ep_return || !ep_length || !ep_flags || !acc4 || N <= 0) return vf::fail(VF_EINVAL, "vf_episode_stats: bad argument");
    hipLaunchKernelGGL(vf::k_episode_stats, dim3(1), dim3(1024), 0, vf::as_stream(stream), done, ep_return, ep_length, ep_flags, acc4, N);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_head_sample_at(const float* mean, const float* log_std, float* action, float* log_prob, int32_t M, uint64_t row0, uint64_t seed,
                      uint64_t step, int32_t deterministic, vf_stream_t stream)
{
    if (!mean || !log_std || !action || !log_prob || M <= 0) return vf::fail(VF_EINVAL, "vf_head_sample: bad argument");
    if (row0 + (uint64_t)M > (uint64_t)1 << 32) return vf::fail(VF_EINVAL, "vf_head_sample_at: rows [row0, row0 + M) do not fit the 32-bit counter word");
    hipLaunchKernelGGL(vf::k_head_sample, dim3(vf::blocks_for(M)), dim3(vf::kBlock), 0, vf::as_stream(stream),
                       reinterpret_cast<const float4*>(mean), log_std, reinterpret_cast<float4*>(action), log_prob, M, (unsigned)row0,
                       (unsigned long long)seed, (unsigned long long)step, deterministic);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_head_sample(const float* mean, const float* log_std, float* action, float* log_prob, int32_t M, uint64_t seed,
                   uint64_t step, int32_t deterministic, vf_stream_t stream)
{
    return vf_head_sample_at(mean, log_std, action, log_prob, M, 0, seed, step, deterministic, stream);
}

int vf_head_sample_eps(const float* mean, const float* log_std, const float* eps, float* action, float* log_prob, int32_t M,
                       vf_stream_t stream)
{
    if (!mean || !log_std || !eps || !action || !log_prob || M <= 0) return vf::fail(VF_EINVAL, "vf_head_sample_eps: bad argument");
    if ((reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(action)) % 16)
        return vf::fail(VF_EINVAL, "vf_head_sample_eps: mean, eps and action must be 16-byte aligned");
    hipLaunchKernelGGL(vf::k_head_sample_eps, dim3(vf::blocks_for(M)), dim3(vf::kBlock), 0, vf::as_stream(stream),
                       reinterpret_cast<const float4*>(mean), log_std, reinterpret_cast<const float4*>(eps),
                       reinterpret_cast<float4*>(action), log_prob, M);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_ppo_loss(const float* mean, const float* value, const float* log_std, const float* action, const float* old_log_prob,
                const float* adv, const float* ret, float* d_mean, float* d_value, float* stats, int32_t M,
                const vf_ppo_loss_cfg* cfg, float* scratch, vf_stream_t stream)
{
    if (!mean || !value || !log_std || !action || !old_log_prob || !adv || !ret || !d_mean || !d_value || !stats || !cfg ||
        !scratch || M <= 0)
        return vf::fail(VF_EINVAL, "vf_ppo_loss: bad argument");
    const int nblk = vf::blocks_for(M);
    if (nblk > 1024) return vf::fail(VF_EINVAL, "vf_ppo_loss: at most 262144 rows per call (scratch contract)");
    hipStream_t st = vf::as_stream(stream);
    hipLaunchKernelGGL(vf::k_ppo_loss, dim3(nblk), dim3(vf::kBlock), 0, st, reinterpret_cast<const float4*>(mean), value,
                       log_std, reinterpret_cast<const float4*>(action), old_log_prob, adv, ret,
                       reinterpret_cast<float4*>(d_mean), d_value, scratch, M, *cfg);
    hipLaunchKernelGGL(vf::k_fold_stats, dim3(1), dim3(1024), 0, st, scratch, nblk, stats, cfg->d_log_std_out, cfg->stats_accum);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_gather_rows(const vf_gather_fields* fields, const int64_t* perm, int64_t rows, vf_stream_t stream)
{
    if (!fields || !perm || rows <= 0 || fields->n_fields < 1 || fields->n_fields > VF_GATHER_MAX_FIELDS)
        return vf::fail(VF_EINVAL, "vf_gather_rows: bad argument");
    int wmax = 1;
    for (int i = 0; i < fields->n_fields; ++i) {
        if (!fields->src[i] || !fields->dst[i] || fields->width[i] < 1) return vf::fail(VF_EINVAL, "vf_gather_rows: field %d: bad pointer / width", i);
        wmax = fields->width[i] > wmax ? fields->width[i] : wmax;
    }
    if (wmax > vf::kBlock) return vf::fail(VF_EINVAL, "vf_gather_rows: rows wider than %d floats", vf::kBlock);
    int wp = 1;
    while (wp < wmax) wp <<= 1;
    const long blocks = (rows * wp + vf::kBlock - 1) / vf::kBlock;
    hipLaunchKernelGGL(vf::k_gather_rows, dim3((unsigned)(blocks < 65536 ? blocks : 65536), fields->n_fields), dim3(vf::kBlock), 0,
                       vf::as_stream(stream), *fields, perm, (long)rows);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_rollout_post(const float* reward, const uint8_t* done, const uint8_t* ep_flags, const float* terminal_value, float gamma,
                    float* reward_out, float* next_episode_start, int32_t N, vf_stream_t stream)
{
    if (!reward || !done || !ep_flags || !terminal_value || !reward_out || !next_episode_start || N <= 0)
        return vf::fail(VF_EINVAL, "vf_rollout_post: bad argument");
    hipLaunchKernelGGL(vf::k_rollout_post, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream), reward, done, ep_flags,
                       terminal_value, gamma, reward_out, next_episode_start, N);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_rollout_post_collect(const float* reward, const uint8_t* done, const uint8_t* ep_flags, float* reward_out,
                            float* next_episode_start, const float* obs0, const float* obs1, int32_t w0, int32_t w1, int32_t* cursor,
                            int32_t capacity, int32_t* idx_list, float* rows0, float* rows1, int32_t flat_base, int32_t N,
                            const float* ep_return, const int32_t* ep_length, float* episode_stat, vf_stream_t stream)
{
    if (!reward || !done || !ep_flags || !reward_out || !next_episode_start || !obs0 || !cursor || !idx_list || !rows0 || N <= 0 ||
        w0 <= 0 || w1 < 0 || capacity <= 0 || (w1 > 0 && (!obs1 || !rows1)) || (episode_stat && (!ep_return || !ep_length)))
        return vf::fail(VF_EINVAL, "vf_rollout_post_collect: bad argument");
    if (episode_stat && reinterpret_cast<uintptr_t>(episode_stat) % 16) return vf::fail(VF_EINVAL, "vf_rollout_post_collect: episode_stat must be 16-byte aligned");
    hipLaunchKernelGGL(vf::k_rollout_post_collect, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream), reward, done,
                       ep_flags, reward_out, next_episode_start, obs0, obs1, w0, w1, cursor, capacity, idx_list, rows0, rows1, flat_base, N,
                       ep_return, ep_length, episode_stat);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_bootstrap_scatter(const int32_t* idx_list, const float* values, int32_t count, float gamma, float* rewards_flat,
                         vf_stream_t stream)
{
    if (!idx_list || !values || !rewards_flat || count < 0) return vf::fail(VF_EINVAL, "vf_bootstrap_scatter: bad argument");
    if (count == 0) return VF_OK;
    hipLaunchKernelGGL(vf::k_bootstrap_scatter, dim3(vf::blocks_for(count)), dim3(vf::kBlock), 0, vf::as_stream(stream), idx_list, values,
                       count, gamma, rewards_flat);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_ppo_update(const vf_mlp_desc* fwd, const vf_mlp_bwd_desc* bwd, const float* params, const float* packed,
                  const float* in0, const float* in1, const float* log_std, const float* action, const float* old_log_prob,
                  const float* adv, const float* ret, float* stats, int32_t M, const vf_ppo_loss_cfg* cfg, float* scratch,
                  vf_stream_t stream)
{
    if (!fwd || !params || !packed || !in0 || !log_std || !action || !old_log_prob || !adv || !ret || !cfg || !scratch || M <= 0)
        return vf::fail(VF_EINVAL, "vf_ppo_update: bad argument");
    if (int rc = vf::check_fwd_desc(fwd, "vf_ppo_update")) return rc;
    if (int rc = vf::check_bwd_desc(bwd, "vf_ppo_update")) return rc;
    const int nwaves = (M + 31) / 32;        // = partial rows of loss statistics in scratch (16 floats each; any count: k_fold_stats strides over them)
    hipStream_t st = vf::as_stream(stream);
    const int rc = vf::ppo_update_chain_try(fwd, bwd, params, packed, in0, in1, log_std, action, old_log_prob, adv, ret, scratch, cfg, M, st);
    if (rc < 0) return rc;
    if (rc == 0) return vf::fail(VF_EUNSUPPORTED, "vf_ppo_update: the layer tables are not an instantiated network class");
    if (stats)      // else: the caller folds the partial rows (vf_mlp_weight_grad_sumsq loss_stats)
        hipLaunchKernelGGL(vf::k_fold_stats, dim3(1), dim3(1024), 0, st, scratch, nwaves, stats, cfg->d_log_std_out, cfg->stats_accum);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

}  // extern "C"
