// vf_mfma_tile.hpp -- what the two LDS-staged fp32-MFMA units share: the nn.Linear kernels (vf_linear.hip) and the block-tile
// whole-network kernels (vf_mlp_tile.hip).  Both walk 64-row tiles whose operands sit in LDS rows of odd stride and feed
// v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate, k-ordered; conflict-free ds_read_b32 for the A/B fragments):
//   f32x16, kRows            accumulator fragment and rows per tile
//   mfma_sweep1 / 2          sweeps with both operands in LDS
//   stage_rows, RowPrefetch  global -> LDS staging of one tile, in one go or split around other work
//   allow_lds                host: opt a kernel in to more than 64 KiB of dynamic LDS
// What only one of the two units uses stays in that unit.  Not compiled into chain plugins.
#pragma once
#include "vf_common.hpp"

namespace vf {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ------------------------------------------------------------------------------------------------
// Linear layers on the fp32 MFMA.  Block = 4 waves, 64 output rows; each wave owns one 32-row
// half and every other 32-column tile.  C/D fragment of v_mfma_f32_32x32x2_f32:
// col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
// ------------------------------------------------------------------------------------------------
constexpr int kRows = 64;

// Branch-free MFMA sweeps over a reduction padded to a multiple of 16 (pad columns are zero in LDS):
// per chunk, the fragments of 8 k-pairs are fetched from LDS ahead of the MFMAs that consume them.
// `bs` = LDS stride of one reduction step for the B fragment.  Callers pick the variant with a
// wave-uniform (SGPR) condition, so there is no exec-mask traffic around the matrix instructions.
__device__ __forceinline__ void mfma_sweep1(const float* __restrict__ ap, const float* __restrict__ b0, int bs, int red16,
                                            f32x16& acc0)
{
    for (int k0 = 0; k0 < red16; k0 += 16) {
        float a[8], x0[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] = ap[k0 + 2 * j]; x0[j] = b0[(k0 + 2 * j) * bs]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x0[j], acc0, 0, 0, 0);
    }
}
__device__ __forceinline__ void mfma_sweep2(const float* __restrict__ ap, const float* __restrict__ b0,
                                            const float* __restrict__ b1, int bs, int red16, f32x16& acc0, f32x16& acc1)
{
    for (int k0 = 0; k0 < red16; k0 += 16) {
        float a[8], x0[8], x1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] = ap[k0 + 2 * j]; x0[j] = b0[(k0 + 2 * j) * bs]; x1[j] = b1[(k0 + 2 * j) * bs]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x0[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x1[j], acc1, 0, 0, 0);
        }
    }
}

// Stage one 64-row tile of A (optionally masked by Ym > 0) into LDS rows of odd stride `sa`.
// Vector path: 16-byte global loads when the row length is a multiple of 4 with a power-of-two
// number of float4 per row (K, No in {4, 8, ..., 128}); scalar path otherwise (K = 13, 3).
template <bool MASK, int NT = kBlock>
__device__ __forceinline__ void stage_rows(float* __restrict__ As, int sa, const float* __restrict__ A, int lda,
                                           const float* __restrict__ Ym, int ldym, int m0, int M, int red, int redp,
                                           int nrows = kRows, int act = VF_ACTIVATION_RELU)
{
    const int tid = threadIdx.x;
    const int c4 = red >> 2;
    const bool vec = (red & 3) == 0 && (c4 & (c4 - 1)) == 0 && c4 <= 32 && (lda & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(A) & 15) == 0) && (!MASK || !Ym || ((ldym & 3) == 0 && (reinterpret_cast<uintptr_t>(Ym) & 15) == 0));
    const bool mask = MASK && Ym != nullptr;
    // wave-uniform 64-bit bases + 32-bit lane offsets (one VGPR per address).  Rows past the matrix read row
    // M-1 again (valid address, no divergent branch around the load) and are zeroed by a select.
    const float* Ab = A + (size_t)m0 * lda;
    const float* Yb = mask ? Ym + (size_t)m0 * ldym : nullptr;
    const int rmax = M - 1 - m0;                  // last valid row of this tile
    if (vec) {
        const int sh = 31 - __clz(c4);            // log2(float4 per row)
        const int col = (tid & (c4 - 1)) << 2, r0 = tid >> sh, rstep = NT >> sh;
        for (int rb0 = 0; rb0 < nrows; rb0 += 8 * rstep) {   // batches of <= 8 independent 16-byte loads, then the LDS writes
            const int rb = rb0 + r0;
            const int nj = min(8, (nrows - rb0 + rstep - 1) / rstep);   // wave-uniform trip count: no loads for rows that do not exist
            float4 v[8], y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j < nj) {
                    const int r = min(rb + j * rstep, rmax);
                    v[j] = *reinterpret_cast<const float4*>(Ab + (unsigned)(r * lda + col));
                    if (mask) y[j] = *reinterpret_cast<const float4*>(Yb + (unsigned)(r * ldym + col));
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j < nj) {
                    const int r = rb + j * rstep;
                    const bool ok = r <= rmax;
                    float4 x = v[j];
                    if (mask) {
                        x.x = act_mul(x.x, y[j].x, act); x.y = act_mul(x.y, y[j].y, act);
                        x.z = act_mul(x.z, y[j].z, act); x.w = act_mul(x.w, y[j].w, act);
                    }
                    if (r < nrows) {
                        float* d = As + r * sa + col;
                        d[0] = ok ? x.x : 0.0f; d[1] = ok ? x.y : 0.0f; d[2] = ok ? x.z : 0.0f; d[3] = ok ? x.w : 0.0f;
                    }
                }
            }
        }
#ifndef VF_TEST_NO_PAD_ZERO
        if (redp > red) {      // a vector-loadable row that is not a whole MFMA chunk (4- or 8-wide: the action columns of a
            const int np = redp - red;                     // critic): the pad columns must be zeros, not what LDS held before
            for (int i = tid; i < nrows * np; i += NT) As[(i / np) * sa + red + (i % np)] = 0.0f;
        }
#endif
    } else {
        const int total = nrows * redp;
        for (int base = tid; base < total; base += 4 * NT) {     // 4 independent loads in flight per thread
            float x[4], y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = min(base + j * NT, total - 1);
                const int r = idx / redp, k = idx - r * redp;
                const int rc = min(r, rmax), kc = min(k, red - 1);
                x[j] = Ab[(unsigned)(rc * lda + kc)];
                if (mask) y[j] = Yb[(unsigned)(rc * ldym + kc)];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = base + j * NT;
                if (idx < total) {
                    const int r = idx / redp, k = idx - r * redp;
                    float v = x[j];
                    if (mask) v = act_mul(v, y[j], act);
                    As[r * sa + k] = (r <= rmax && k < red) ? v : 0.0f;
                }
            }
        }
    }
}

// Split staging for latency overlap: `load` issues up to 8 independent 16-byte global loads per thread
// into registers (64 rows x <= 128 floats), `store` parks them in LDS later.  Same vector conditions
// as stage_rows; `ok()` false -> the caller falls back to stage_rows.
template <bool MASK>
struct RowPrefetch {
    float4 v[8];
    int sh, col, r0, rstep;
    bool vec;
    __device__ __forceinline__ void setup(const float* A, int lda, const float* Ym, int ldym, int red)
    {
        const int c4 = red >> 2;
        vec = (red & 3) == 0 && (c4 & (c4 - 1)) == 0 && c4 >= 1 && c4 <= 32 && (lda & 3) == 0 &&
              ((reinterpret_cast<uintptr_t>(A) & 15) == 0) &&
              (!MASK || !Ym || ((ldym & 3) == 0 && (reinterpret_cast<uintptr_t>(Ym) & 15) == 0));
        sh = 31 - __clz(c4 > 0 ? c4 : 1);
        col = (threadIdx.x & (c4 - 1)) << 2;
        r0 = threadIdx.x >> sh;
        rstep = kBlock >> sh;          // rows covered per pass; 64 rows -> 64 / rstep <= 8 passes
    }
    __device__ __forceinline__ void load(const float* __restrict__ A, int lda, const float* __restrict__ Ym, int ldym, int m0,
                                         int M, int act = VF_ACTIVATION_RELU)
    {
        const bool mask = MASK && Ym != nullptr;
        float4 y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {       // rows past the matrix re-read row M-1 (no branch around the load), zeroed below
            const int m = min(m0 + r0 + j * rstep, M - 1);
            v[j] = *reinterpret_cast<const float4*>(A + (size_t)m * lda + col);
            if (mask) y[j] = *reinterpret_cast<const float4*>(Ym + (size_t)m * ldym + col);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool ok = m0 + r0 + j * rstep < M;
            float4 x = v[j];
            if (mask) {
                x.x = act_mul(x.x, y[j].x, act); x.y = act_mul(x.y, y[j].y, act);
                x.z = act_mul(x.z, y[j].z, act); x.w = act_mul(x.w, y[j].w, act);
            }
            v[j] = make_float4(ok ? x.x : 0.0f, ok ? x.y : 0.0f, ok ? x.z : 0.0f, ok ? x.w : 0.0f);
        }
    }
    __device__ __forceinline__ void store(float* __restrict__ As, int sa) const
    {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = r0 + j * rstep;
            if (r < kRows) {
                float* d = As + r * sa + col;
                d[0] = v[j].x; d[1] = v[j].y; d[2] = v[j].z; d[3] = v[j].w;
            }
        }
    }
};

template <typename Kern>
int allow_lds(Kern k, size_t bytes)
{
    if (bytes > 64 * 1024) VF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return VF_OK;
}

}  // namespace vf
