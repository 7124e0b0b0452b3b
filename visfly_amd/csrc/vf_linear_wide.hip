// Linear layers wider than the weight-stationary kernels of vf_linear.hip can hold (128 < K or No <= 512), fp32 MFMA.
//
// k_linear / k_linear_wgrad keep the whole weight matrix of a layer in LDS; 256 x 256 fp32 is 256 KiB and the CU has 160.  Here
// nothing is resident: a workgroup owns one 128 x 128 tile of the product, both operands are streamed through LDS in chunks of 32
// reduction steps, and the four waves hold 2 x 2 tiles of 32 x 32 each (64 accumulator registers) for the whole sweep.  The next
// chunk travels global -> registers while the MFMAs of the current one run; the register and LDS (33 KiB) budgets leave room for
// several workgroups per CU, which is what hides the LDS round trips between MFMAs.
//
// One kernel template serves the three products of a layer.  Every operand is a row-major matrix in global memory and a chunk of
// it is a plain 2-D sub-block (128 x 32 or 32 x 128) copied to LDS without a transpose, zero beyond the matrix edge; what differs
// is whether the reduction index is the minor ("red-minor", odd row stride 33) or the major ("red-major", stride 129) index of
// the LDS image, and so how a lane picks its MFMA fragment:
//                 rows x cols   reduction   A operand                B operand
//   forward       M  x No       K           X   [m][k]  red-minor    W [n][k]  red-minor
//   data grad     M  x K        No          dYm [m][n]  red-minor    W [n][k]  red-major
//   weight grad   No x K        rows of M   dYm [m][n]  red-major    X [m][k]  red-major
// dYm = dY * act'(Y) is formed while the chunk is written to LDS (act_mul of vf_common.hpp, as the narrow kernels do).
// The weight gradient splits M into row ranges: every workgroup writes the partial of its range to part[split][No*K + No] and
// k_fold_partials (vf_linear.hip) adds them in a fixed order - no floating-point atomics, bit-identical from run to run.
#include "vf_common.hpp"

namespace vf {

using f32x16 = __attribute__((ext_vector_type(16))) float;

namespace {

constexpr int kWT = 128;                   // tile edge (rows and columns of the product per workgroup)
constexpr int kWC = 32;                    // reduction steps per chunk
constexpr int kWPer = kWT * kWC / kBlock;  // floats of one operand chunk per thread (16)
enum { kWideFwd = 0, kWideBwdData = 1, kWideWgrad = 2 };

// a thread's share of an R x CN sub-block of a row-major matrix: elements (r + i * (kBlock / CN), c), i < 16
template <int R, int CN>
struct WideChunk {
    static_assert(R * CN == kWT * kWC, "one chunk");
    static constexpr int kStep = kBlock / CN;   // rows per pass: 8 (128 x 32) or 2 (32 x 128)
    float v[kWPer], y[kWPer];
    // rows r0.. (valid below rmax), columns c0.. (valid below cmax); Ym == nullptr: no activation derivative
    __device__ __forceinline__ void load(const float* __restrict__ S, int ld, const float* __restrict__ Ym, int ldym, int r0, int rmax,
                                         int c0, int cmax)
    {
        const int c = c0 + (int)(threadIdx.x % CN), r = r0 + (int)(threadIdx.x / CN);
#pragma unroll
        for (int i = 0; i < kWPer; ++i) {
            const int rr = r + i * kStep;
            const bool ok = rr < rmax && c < cmax;
            v[i] = ok ? S[(size_t)rr * ld + c] : 0.0f;
            y[i] = (ok && Ym) ? Ym[(size_t)rr * ldym + c] : 0.0f;
        }
    }
    __device__ __forceinline__ void store(float* __restrict__ L, bool masked, int act) const
    {
        float* d = L + (threadIdx.x / CN) * (CN + 1) + threadIdx.x % CN;
#pragma unroll
        for (int i = 0; i < kWPer; ++i) d[i * kStep * (CN + 1)] = masked ? act_mul(v[i], y[i], act) : v[i];
    }
};

template <int MODE>
__global__ __launch_bounds__(kBlock, 2) void k_linear_wide(const float* __restrict__ A, int lda, const float* __restrict__ Ym, int ldym,
                                                           const float* __restrict__ B, int ldb, const float* __restrict__ bias,
                                                           float* __restrict__ C, int ldc, int M, int K, int No, int accumulate, int act,
                                                           int rows_per_split)
{
    constexpr bool AT = MODE == kWideWgrad;   // A image red-major
    constexpr bool BT = MODE != kWideFwd;     // B image red-major
    constexpr int AR = AT ? kWC : kWT, AC = AT ? kWT : kWC;
    constexpr int BR = BT ? kWC : kWT, BC = BT ? kWT : kWC;
    constexpr int sa = AC + 1, sb = BC + 1;
    __shared__ float As[AR * sa];
    __shared__ float Bs[BR * sb];

    const int rows = MODE == kWideWgrad ? No : M;
    const int cols = MODE == kWideFwd ? No : K;
    const int ctiles = (cols + kWT - 1) / kWT, rtiles = (rows + kWT - 1) / kWT;
    const int ntile = ctiles * rtiles;
    const int split = (int)(blockIdx.x / (unsigned)ntile), tile = (int)(blockIdx.x % (unsigned)ntile);
    const int row0 = tile / ctiles * kWT, col0 = tile % ctiles * kWT;
    // reduction range [lo, hi)
    int lo = 0, hi = MODE == kWideFwd ? K : No;
    if (MODE == kWideWgrad) {
        const long long b = (long long)split * rows_per_split;
        lo = (int)b;
        hi = (int)(b + rows_per_split < (long long)M ? b + rows_per_split : (long long)M);
    }
    const bool masked = MODE != kWideFwd && Ym != nullptr;
    const float* ym = masked ? Ym : nullptr;

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the tile guards below are scalar branches
    const int lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const int wr = (wave & 1) * 64, wc = (wave >> 1) * 64;       // this wave's 64 x 64 quarter of the tile
    // 32 x 32 tiles of the quarter that lie inside the product (edge tiles of a narrow head layer are skipped, not multiplied by zeros)
    const bool r0v = row0 + wr < rows, r1v = row0 + wr + 32 < rows;
    const bool c0v = col0 + wc < cols, c1v = col0 + wc + 32 < cols;

    const float* a0 = AT ? As + lk * sa + wr + lr : As + (wr + lr) * sa + lk;
    const float* b0 = BT ? Bs + lk * sb + wc + lr : Bs + (wc + lr) * sb + lk;
    constexpr int ak = AT ? sa : 1, at = AT ? 32 : 32 * sa;      // floats per reduction step / per 32-row tile
    constexpr int bk = BT ? sb : 1, bt = BT ? 32 : 32 * sb;

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    float bsum = 0.0f;    // weight gradient, column tile 0, thread < 128: column sum of dYm over this split's rows

    WideChunk<AR, AC> ca;
    WideChunk<BR, BC> cb;
    auto fetch = [&](int k0) {
        if (AT) ca.load(A, lda, ym, ldym, k0, hi, row0, rows);
        else ca.load(A, lda, ym, ldym, row0, rows, k0, hi);
        if (BT) cb.load(B, ldb, nullptr, 0, k0, hi, col0, cols);
        else cb.load(B, ldb, nullptr, 0, col0, cols, k0, hi);
    };
    fetch(lo);
    for (int k0 = lo; k0 < hi; k0 += kWC) {
        ca.store(As, masked, act);
        cb.store(Bs, false, 0);
        __syncthreads();
        if (k0 + kWC < hi) fetch(k0 + kWC);     // in flight while the MFMAs below run
        if (MODE == kWideWgrad && col0 == 0 && tid < kWT) {
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int r = 0; r < kWC; r += 2) { s0 += As[r * sa + tid]; s1 += As[(r + 1) * sa + tid]; }
            bsum += s0 + s1;
        }
#pragma unroll
        for (int kk = 0; kk < kWC; kk += 2) {
            const float fa0 = a0[kk * ak], fa1 = a0[kk * ak + at];
            const float fb0 = b0[kk * bk], fb1 = b0[kk * bk + bt];
            if (r0v && c0v) acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0, fb0, acc00, 0, 0, 0);
            if (r0v && c1v) acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0, fb1, acc01, 0, 0, 0);
            if (r1v && c0v) acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1, fb0, acc10, 0, 0, 0);
            if (r1v && c1v) acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1, fb1, acc11, 0, 0, 0);
        }
        __syncthreads();                        // every wave is done with this chunk before the next one overwrites it
    }

    // epilogue: lane lr owns column lr of a 32 x 32 tile, register `reg` row (reg & 3) + 8 * (reg >> 2) + 4 * lk
    float* out = C;
    if (MODE == kWideWgrad) out = C + (size_t)split * ((size_t)No * K + No);
    const int ldo = MODE == kWideWgrad ? K : ldc;
    auto emit = [&](const f32x16& acc, int rb, int cb0) {
        const int n = col0 + wc + cb0 + lr;
        if (n >= cols) return;
        const float bn = (MODE == kWideFwd && bias) ? bias[n] : 0.0f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = row0 + wr + rb + (reg & 3) + 8 * (reg >> 2) + 4 * lk;
            if (m >= rows) continue;
            float* dst = out + (size_t)m * ldo + n;
            if (MODE == kWideFwd) *dst = act_fwd(acc[reg] + bn, act);
            else if (MODE == kWideBwdData) *dst = accumulate ? *dst + acc[reg] : acc[reg];
            else *dst = acc[reg];
        }
    };
    if (r0v && c0v) emit(acc00, 0, 0);
    if (r0v && c1v) emit(acc01, 0, 32);
    if (r1v && c0v) emit(acc10, 32, 0);
    if (r1v && c1v) emit(acc11, 32, 32);
    if (MODE == kWideWgrad && col0 == 0 && tid < kWT && row0 + tid < No) out[(size_t)No * K + row0 + tid] = bsum;
}

long long tiles_of(int rows, int cols) { return (long long)((rows + kWT - 1) / kWT) * ((cols + kWT - 1) / kWT); }

}  // namespace

int linear_wide_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int ldy, int M, int K, int No, int act, hipStream_t st)
{
    const long long grid = tiles_of(M, No);
    hipLaunchKernelGGL((k_linear_wide<kWideFwd>), dim3((unsigned)grid), dim3(kBlock), 0, st, X, ldx, (const float*)nullptr, 0, W, K, b, Y,
                       ldy, M, K, No, 0, act, 0);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int linear_wide_bwd_data(const float* dY, int lddy, const float* Ymask, int ldym, const float* W, float* dX, int lddx, int M, int K, int No,
                         int accumulate, int act, hipStream_t st)
{
    const long long grid = tiles_of(M, K);
    hipLaunchKernelGGL((k_linear_wide<kWideBwdData>), dim3((unsigned)grid), dim3(kBlock), 0, st, dY, lddy, Ymask, ldym, W, K,
                       (const float*)nullptr, dX, lddx, M, K, No, accumulate, act, 0);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

// Rows of M per split: about 512 workgroups in all (two per CU), every range a whole number of chunks.  The partial of a split is
// No*K + No floats, so at 512 x 512 (16 tiles, 32 splits) the scratch is 32 MiB whatever M is.
int linear_wide_rows_per_split(int M, int K, int No)
{
    const long long tiles = tiles_of(No, K);
    long long want = 512 / tiles;
    if (want < 1) want = 1;
    long long rps = ((long long)M + want - 1) / want;
    rps = (rps + kWC - 1) / kWC * kWC;
    return (int)rps;
}

int linear_wide_splits(int M, int K, int No)
{
    const int rps = linear_wide_rows_per_split(M, K, No);
    return (int)(((long long)M + rps - 1) / rps);
}

int linear_wide_wgrad_partials(const float* dY, int lddy, const float* Ymask, int ldym, const float* X, int ldx, float* part, int M, int K,
                               int No, int act, hipStream_t st)
{
    const int rps = linear_wide_rows_per_split(M, K, No);
    const long long grid = tiles_of(No, K) * linear_wide_splits(M, K, No);
    hipLaunchKernelGGL((k_linear_wide<kWideWgrad>), dim3((unsigned)grid), dim3(kBlock), 0, st, dY, lddy, Ymask, ldym, X, ldx,
                       (const float*)nullptr, part, 0, M, K, No, 0, act, rps);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

}  // namespace vf
