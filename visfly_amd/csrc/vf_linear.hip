// vf_linear.hip -- one nn.Linear at a time on the fp32 MFMA: forward, data gradient, weight / bias gradient (every vf_linear_*).
//
// Reference: the nn.Linear + activation pairs of create_mlp (utils/policies/extractors.py:376-449) under torch autograd, as the
// policies of utils/policies/policies.py:195-254 and td_policies.py run them.  Here each product of a layer is one launch.
//
// This unit holds the weight-stationary kernels for layers up to kLinearNarrowMax (128) wide -- k_linear<BWD>, k_linear_wgrad --
// and the deterministic second stage of every weight gradient, k_fold_partials.  Wider layers (up to kLinearWideMax) are served by
// the streamed-operand kernels of vf_linear_wide.hip; the entry points below are the only place that decides between the two:
// validate, pick narrow or wide, launch.  Tile staging and MFMA sweeps are shared with vf_mlp_tile.hip through vf_mfma_tile.hpp;
// vf_mlp_backward folds its partials through fold_partials_launch (declared in vf_common.hpp).
#include "vf_mfma_tile.hpp"

namespace vf {

// BWD == false: C[m][n] = act(sum_k A[m][k] * W[n][k] + b[n])          (forward; red = K, cols = No)
// BWD == true : C[m][k] = sum_n (A[m][n] * [Ymask[m][n] > 0]) * W[n][k]  (data grad; red = No, cols = K)
// Weight-stationary: a block stages W once and walks 64-row tiles with stride gridDim.x; the next
// tile's rows are fetched into registers while the MFMAs of the current one run.
template <bool BWD>
__global__ __launch_bounds__(kBlock) void k_linear(const float* __restrict__ A, int lda, const float* __restrict__ Ym,
                                                   int ldym, const float* __restrict__ W, const float* __restrict__ bias,
                                                   float* __restrict__ C, int ldc, int M, int K, int No, int accumulate, int act)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int red = BWD ? No : K;         // reduction length
    const int cols = BWD ? K : No;        // output columns
    const int red16 = (red + 15) & ~15;   // the MFMA sweeps consume 16 reduction steps per chunk; pads are zero
    const int ct = (cols + 31) >> 5;      // 32-column tiles
    const int sa = red16 + 1;             // odd LDS row strides
    float* As = lds;                      // [64][sa]
    float* Ws = lds + kRows * sa;         // fwd: [ct*32][sa] (col-major over red) ; bwd: [red16][ct*32+1]
    const int sw = BWD ? ct * 32 + 1 : sa;
    const int tid = threadIdx.x;
    const int ntiles = (M + kRows - 1) / kRows;

    RowPrefetch<BWD> pf;
    pf.setup(A, lda, Ym, ldym, red);
    int tile = blockIdx.x;
    if (pf.vec && tile < ntiles) pf.load(A, lda, Ym, ldym, tile * kRows, M, act);   // in flight while W is staged

    // W image: Ws[n * sw + k] = W[n][k] for both directions (forward reads it column-major over the
    // reduction, the data gradient row-major); pads are zero.
    const int wrows = BWD ? red16 : ct * 32, wcols = BWD ? ct * 32 : red16;
    const bool padded = wrows != No || wcols != K || red16 != red;
    if (padded) {
        for (int idx = tid; idx < kRows * sa + wrows * sw; idx += kBlock) lds[idx] = 0.0f;
        __syncthreads();
    }
    stage_rows<false>(Ws, sw, W, K, nullptr, 0, 0, No, K, K, wrows);

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform on purpose (SGPR control flow)
    const int lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const int rt = wave & 1;              // row half
    const int c0 = wave >> 1;             // column tiles c0, c0 + 2
    const int nacc = c0 + 2 < ct ? 2 : (c0 < ct ? 1 : 0);
    const float* ap = As + (rt * 32 + lr) * sa + lk;
    const float* b0 = BWD ? Ws + lk * sw + c0 * 32 + lr : Ws + (c0 * 32 + lr) * sw + lk;
    const float* b1 = BWD ? Ws + lk * sw + (c0 + 2) * 32 + lr : Ws + ((c0 + 2) * 32 + lr) * sw + lk;
    const int bs = BWD ? sw : 1;
    for (; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * kRows;
        if (pf.vec) pf.store(As, sa);
        else stage_rows<BWD>(As, sa, A, lda, Ym, ldym, m0, M, red, red, kRows, act);
        __syncthreads();
        if (pf.vec && tile + gridDim.x < ntiles) pf.load(A, lda, Ym, ldym, (tile + gridDim.x) * kRows, M, act);
        f32x16 acc0 = {0}, acc1 = {0};
        if (nacc == 2) mfma_sweep2(ap, b0, b1, bs, red16, acc0, acc1);
        else if (nacc == 1) mfma_sweep1(ap, b0, bs, red16, acc0);
        auto emit = [&](const f32x16& acc, int ctile) {
            const int n = ctile * 32 + lr;
            if (n >= cols) return;
            const float bn = (!BWD && bias) ? bias[n] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int m = m0 + rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lk;
                if (m >= M) continue;
                float y = acc[reg] + bn;
                if (!BWD) y = act_fwd(y, act);
                float* dst = C + (size_t)m * ldc + n;
                *dst = accumulate ? *dst + y : y;
            }
        };
        if (nacc >= 1) emit(acc0, c0);
        if (nacc == 2) emit(acc1, c0 + 2);
        __syncthreads();                  // every wave is done reading As before the next tile overwrites it
    }
}

// dW[n][k] = sum_m dYm[m][n] X[m][k]; block = one chunk of rows, partial written to part[blk][No*K + No]
__global__ __launch_bounds__(kBlock) void k_linear_wgrad(const float* __restrict__ dY, int lddy, const float* __restrict__ Ym,
                                                         int ldym, const float* __restrict__ X, int ldx,
                                                         float* __restrict__ part, int M, int K, int No, int rows_per_block, int act)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nt = (No + 31) >> 5, kt = (K + 31) >> 5;
    const int sd = nt * 32 + 1, sx = kt * 32 + 1;
    float* Ds = lds;               // [64][sd]  masked dY rows
    float* Xs = lds + kRows * sd;  // [64][sx]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const int mb = blockIdx.x * rows_per_block;
    const int me = min(M, mb + rows_per_block);
    const int ntiles = nt * kt;  // <= 16, wave takes tiles wave, wave+4, ...
    f32x16 acc[4] = {{0}, {0}, {0}, {0}};
    float bsum = 0.0f;  // thread tid < No: column sum of masked dY
    for (int idx = tid; idx < kRows * (sd + sx); idx += kBlock) lds[idx] = 0.0f;   // pad columns stay zero
    __syncthreads();
    for (int m0 = mb; m0 < me; m0 += kRows) {
        stage_rows<true>(Ds, sd, dY, lddy, Ym, ldym, m0, me, No, nt * 32, kRows, act);
        stage_rows<false>(Xs, sx, X, ldx, nullptr, 0, m0, me, K, kt * 32);
        __syncthreads();
        {   // bias gradient: every thread owns (column, row-slice); slices are combined at the end
            const int cgrp = No <= 64 ? 64 : 128, c = tid & (cgrp - 1), part = tid / cgrp, rows = kRows * cgrp / kBlock;
            if (c < No) {
                float s0 = 0.0f, s1 = 0.0f;
                const float* dp = Ds + (part * rows) * sd + c;
                for (int r = 0; r < rows; r += 2) { s0 += dp[r * sd]; s1 += dp[(r + 1) * sd]; }
                bsum += s0 + s1;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int tile = wave + 4 * q;
            if (tile >= ntiles) break;
            const int it = tile / kt, jt = tile - it * kt;
            const float* ap = Ds + lk * sd + it * 32 + lr;
            const float* bp = Xs + lk * sx + jt * 32 + lr;
            f32x16 c = acc[q];
#pragma unroll
            for (int k0 = 0; k0 < kRows; k0 += 16) {   // fetch 8 fragment pairs, then 8 MFMAs
                float fa[8], fb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { fa[j] = ap[(k0 + 2 * j) * sd]; fb[j] = bp[(k0 + 2 * j) * sx]; }
#pragma unroll
                for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j], fb[j], c, 0, 0, 0);
            }
            acc[q] = c;
        }
        __syncthreads();
    }
    float* p = part + (size_t)blockIdx.x * ((size_t)No * K + No);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int tile = wave + 4 * q;
        if (tile >= ntiles) break;
        const int it = tile / kt, jt = tile - it * kt;
        const int k = jt * 32 + lr;
        if (k >= K) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int n = it * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lk;
            if (n < No) p[(size_t)n * K + k] = acc[q][reg];
        }
    }
    {
        __syncthreads();
        const int cgrp = No <= 64 ? 64 : 128, c = tid & (cgrp - 1), part = tid / cgrp, nparts = kBlock / cgrp;
        lds[part * cgrp + c] = bsum;
        __syncthreads();
        if (tid < No) {
            float t = 0.0f;
            for (int q = 0; q < nparts; ++q) t += lds[q * cgrp + tid];
            p[(size_t)No * K + tid] = t;
        }
    }
}

// deterministic second stage: a block owns 64 consecutive output elements (one 256-byte row segment per wave-load);
// wave w sums the partial rows b = w, w+4, w+8, ... with four independent chains, the four waves are combined through
// LDS in a fixed order
__global__ __launch_bounds__(kBlock) void k_fold_partials(const float* __restrict__ part, int nblk, int stride, int nw, int nb,
                                                          float* __restrict__ dW, float* __restrict__ db, int accumulate)
{
    const int n = nw + nb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 64 + lane;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (e < n) {
        const float* p = part + e;
        int r = wave;
        for (; r + 12 < nblk; r += 16) {
            s0 += p[(size_t)r * stride];
            s1 += p[(size_t)(r + 4) * stride];
            s2 += p[(size_t)(r + 8) * stride];
            s3 += p[(size_t)(r + 12) * stride];
        }
        for (; r < nblk; r += 4) s0 += p[(size_t)r * stride];
    }
    __shared__ float sh[4][64];
    sh[wave][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (wave == 0 && e < n) {
        const float t = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
        if (e < nw) dW[e] = accumulate ? dW[e] + t : t;
        else if (db) db[e - nw] = accumulate ? db[e - nw] + t : t;
    }
}

void fold_partials_launch(const float* part, int nblk, int stride, int nw, int nb, float* dW, float* db, int accumulate, hipStream_t st)
{
    const int n = nw + nb;
    hipLaunchKernelGGL(k_fold_partials, dim3((n + 63) / 64), dim3(kBlock), 0, st, part, nblk, stride, nw, nb, dW, db, accumulate);
}

}  // namespace vf

namespace {

// ---- the weight-stationary kernels behind the same three calls as vf_linear_wide.hip's linear_wide_* ----
size_t linear_lds_bytes(bool bwd, int K, int No)
{
    const int red = bwd ? No : K, cols = bwd ? K : No;
    const int red16 = (red + 15) & ~15, ct = (cols + 31) >> 5, sa = red16 + 1;
    const size_t ws = bwd ? (size_t)red16 * (ct * 32 + 1) : (size_t)ct * 32 * sa;
    return ((size_t)vf::kRows * sa + ws) * sizeof(float);
}

int linear_grid(int M)
{
    const int ntiles = (M + vf::kRows - 1) / vf::kRows;
    return ntiles < 512 ? ntiles : 512;   // weight-stationary blocks, two per CU
}

int wgrad_rows_per_block(int M)
{
    int rpb = (M + 255) / 256;  // aim at <= 256 chunks (one per CU), each a multiple of the 64-row tile
    rpb = (rpb + vf::kRows - 1) / vf::kRows * vf::kRows;
    return rpb < vf::kRows ? vf::kRows : rpb;
}

int linear_narrow_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int ldy, int M, int K, int No, int act, hipStream_t st)
{
    const size_t lds = linear_lds_bytes(false, K, No);
    if (int rc = vf::allow_lds(vf::k_linear<false>, lds)) return rc;
    hipLaunchKernelGGL((vf::k_linear<false>), dim3(linear_grid(M)), dim3(vf::kBlock), lds, st, X, ldx, (const float*)nullptr, 0, W, b, Y, ldy,
                       M, K, No, 0, act);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int linear_narrow_bwd_data(const float* dY, int lddy, const float* Ymask, int ldym, const float* W, float* dX, int lddx, int M, int K, int No,
                           int accumulate, int act, hipStream_t st)
{
    const size_t lds = linear_lds_bytes(true, K, No);
    if (int rc = vf::allow_lds(vf::k_linear<true>, lds)) return rc;
    hipLaunchKernelGGL((vf::k_linear<true>), dim3(linear_grid(M)), dim3(vf::kBlock), lds, st, dY, lddy, Ymask, ldym, W, (const float*)nullptr,
                       dX, lddx, M, K, No, accumulate, act);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int linear_narrow_wgrad_partials(const float* dY, int lddy, const float* Ymask, int ldym, const float* X, int ldx, float* part, int M, int K,
                                 int No, int act, hipStream_t st)
{
    const int rpb = wgrad_rows_per_block(M);
    const int nt = (No + 31) >> 5, kt = (K + 31) >> 5;
    const size_t lds = (size_t)vf::kRows * ((nt * 32 + 1) + (kt * 32 + 1)) * sizeof(float);
    if (int rc = vf::allow_lds(vf::k_linear_wgrad, lds)) return rc;
    hipLaunchKernelGGL(vf::k_linear_wgrad, dim3((M + rpb - 1) / rpb), dim3(vf::kBlock), lds, st, dY, lddy, Ymask, ldym, X, ldx, part, M, K, No,
                       rpb, act);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

// row ranges of M = partials of No*K + No floats the weight gradient writes, on either side of the predicate
int linear_wgrad_splits(int M, int K, int No)
{
    if (vf::linear_is_wide(K, No)) return vf::linear_wide_splits(M, K, No);
    const int rpb = wgrad_rows_per_block(M);
    return (M + rpb - 1) / rpb;
}

bool bad_dims(int M, int K, int No) { return M <= 0 || K <= 0 || No <= 0 || K > vf::kLinearWideMax || No > vf::kLinearWideMax; }
bool bad_act(int act) { return act < 0 || act > VF_ACTIVATION_LEAKY_RELU; }

int linear_bwd_weight(const float* dY, int32_t lddy, const float* Ymask, int32_t ldym, const float* X, int32_t ldx, float* dW, float* db,
                      int32_t M, int32_t K, int32_t No, float* scratch, vf_stream_t stream, int accumulate, int act)
{
    if (!dY || !X || !dW || !scratch || bad_dims(M, K, No) || bad_act(act))
        return vf::fail(VF_EINVAL, "vf_linear_bwd_weight: bad argument (K, No <= %d)", vf::kLinearWideMax);
    hipStream_t st = vf::as_stream(stream);
    const int splits = linear_wgrad_splits(M, K, No);
    if (int rc = vf::linear_is_wide(K, No) ? vf::linear_wide_wgrad_partials(dY, lddy, Ymask, ldym, X, ldx, scratch, M, K, No, act, st)
                                           : linear_narrow_wgrad_partials(dY, lddy, Ymask, ldym, X, ldx, scratch, M, K, No, act, st))
        return rc;
    vf::fold_partials_launch(scratch, splits, No * K + No, No * K, No, dW, db, accumulate, st);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

}  // namespace

extern "C" {

int vf_linear_is_wide(int32_t K, int32_t No) { return vf::linear_is_wide(K, No) ? 1 : 0; }

int vf_linear_fwd(const float* X, int32_t ldx, const float* W, const float* b, float* Y, int32_t ldy, int32_t M,
                  int32_t K, int32_t No, int32_t relu, vf_stream_t stream)
{
    if (!X || !W || !Y || bad_dims(M, K, No) || ldx < K || ldy < No)
        return vf::fail(VF_EINVAL, "vf_linear_fwd: bad argument (K, No <= %d)", vf::kLinearWideMax);
    if (bad_act(relu)) return vf::fail(VF_EINVAL, "vf_linear_fwd: activation kind %d", relu);
    hipStream_t st = vf::as_stream(stream);
    return vf::linear_is_wide(K, No) ? vf::linear_wide_fwd(X, ldx, W, b, Y, ldy, M, K, No, relu, st)
                                     : linear_narrow_fwd(X, ldx, W, b, Y, ldy, M, K, No, relu, st);
}

int vf_linear_bwd_data(const float* dY, int32_t lddy, const float* Ymask, int32_t ldym, const float* W, float* dX,
                       int32_t lddx, int32_t M, int32_t K, int32_t No, int32_t accumulate, int32_t act, vf_stream_t stream)
{
    if (!dY || !W || !dX || bad_dims(M, K, No) || lddy < No || lddx < K || bad_act(act))
        return vf::fail(VF_EINVAL, "vf_linear_bwd_data: bad argument (K, No <= %d)", vf::kLinearWideMax);
    hipStream_t st = vf::as_stream(stream);
    return vf::linear_is_wide(K, No) ? vf::linear_wide_bwd_data(dY, lddy, Ymask, ldym, W, dX, lddx, M, K, No, accumulate, act, st)
                                     : linear_narrow_bwd_data(dY, lddy, Ymask, ldym, W, dX, lddx, M, K, No, accumulate, act, st);
}

int64_t vf_linear_bwd_scratch_floats(int32_t M, int32_t K, int32_t No)
{
    return (int64_t)linear_wgrad_splits(M, K, No) * ((int64_t)No * K + No);
}

int vf_linear_bwd_weight(const float* dY, int32_t lddy, const float* Ymask, int32_t ldym, const float* X, int32_t ldx,
                         float* dW, float* db, int32_t M, int32_t K, int32_t No, float* scratch, int32_t act, vf_stream_t stream)
{
    return linear_bwd_weight(dY, lddy, Ymask, ldym, X, ldx, dW, db, M, K, No, scratch, stream, 0, act);
}

int vf_linear_bwd_weight_acc(const float* dY, int32_t lddy, const float* Ymask, int32_t ldym, const float* X, int32_t ldx,
                             float* dW, float* db, int32_t M, int32_t K, int32_t No, float* scratch, int32_t act, vf_stream_t stream)
{
    return linear_bwd_weight(dY, lddy, Ymask, ldym, X, ldx, dW, db, M, K, No, scratch, stream, 1, act);
}

}  // extern "C"
