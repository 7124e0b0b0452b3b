// vf_mlp_tile.hip -- a whole MLP per launch, block-tile form: k_mlp_pack_weights, k_mlp_forward, k_mlp_backward, and every
// vf_mlp_* entry point.
//
// Reference: the actor-critic networks of utils/policies/policies.py:195-254 built by create_mlp (utils/policies/extractors.py:
// 376-449), run there as torch autograd over nn.Linear + activation.  Here the layer tables vf_mlp_desc / vf_mlp_bwd_desc describe
// the network; a workgroup keeps a 64-row tile of every activation in LDS and walks the layers, weights streamed from the packed
// images on the fp32 MFMA.  These kernels serve any table; the network classes of the chain class table (vf_mlp_chain.hip, chain
// plugins) and the row-slab weight gradients (vf_mlp_wgrad.hip) take a call first where they can, and the entry points that exist
// only for them forward there.  Descriptor validation for all of them is check_fwd_desc / check_bwd_desc (declared in
// vf_common.hpp: vf_ppo_update uses them too).  Tile staging and the LDS sweeps are shared with vf_linear.hip through
// vf_mfma_tile.hpp; the partials of k_mlp_backward are folded by k_fold_partials of vf_linear.hip (fold_partials_launch).
#include <algorithm>
#include <utility>

#include "vf_mfma_tile.hpp"

namespace vf {

#ifdef VF_PROBE   // tools/exp_probe.py: shader-clock time of block 0 per kernel phase (never part of the product build)
__device__ unsigned long long g_probe[32];
#define VF_PROBE_INIT() unsigned long long probe_t = clock64()
#define VF_PROBE_AT(i)                                                \
    do {                                                              \
        if (blockIdx.x == 0 && threadIdx.x == 0) {                    \
            const unsigned long long t_ = clock64();                  \
            g_probe[i] += t_ - probe_t;                               \
            probe_t = t_;                                             \
        }                                                             \
    } while (0)
#else
#define VF_PROBE_INIT()
#define VF_PROBE_AT(i)
#endif

// ------------------------------------------------------------------------------------------------
// Whole-network forward: activations stay in LDS, weights streamed per layer (see vf_mlp_desc)
// ------------------------------------------------------------------------------------------------
struct MlpIo {
    const float* in[4];
    float* out[2];
};

// MFMA sweeps with the B operand read straight from global memory (L1/L2-resident packed weights,
// coalesced: lane lr = output column) and the A operand from LDS.  Fragments of the next 16 reduction
// steps are fetched while the MFMAs of the current 16 run; the first B chunk is passed in by the caller,
// who issues it before the barrier that publishes the A tile.  `ldb` = floats between reduction steps of B.
struct BFrag {
    float x[8];
};
// bg = wave-uniform base of the layer's packed image, off = this lane's float offset for reduction step 0
__device__ __forceinline__ BFrag load_bfrag(const float* __restrict__ bg, int off, int ldb)
{
    BFrag f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f.x[j] = bg[(unsigned)(off + 2 * j * ldb)];
    return f;
}
__device__ __forceinline__ void mfma_sweep_gb1(const float* __restrict__ ap, const float* __restrict__ bg, int off0, int ldb,
                                               int red16, BFrag x0, f32x16& acc0)
{
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = ap[2 * j];
    for (int k0 = 0; k0 < red16; k0 += 16) {
        float an[8];
        BFrag n0;
        if (k0 + 16 < red16) {
            n0 = load_bfrag(bg, off0 + (k0 + 16) * ldb, ldb);
#pragma unroll
            for (int j = 0; j < 8; ++j) an[j] = ap[k0 + 16 + 2 * j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x0.x[j], acc0, 0, 0, 0);
        if (k0 + 16 < red16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] = an[j]; x0.x[j] = n0.x[j]; }
        }
    }
}
__device__ __forceinline__ void mfma_sweep_gb2(const float* __restrict__ ap, const float* __restrict__ bg, int off0, int off1,
                                               int ldb, int red16, BFrag x0, BFrag x1, f32x16& acc0, f32x16& acc1)
{
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = ap[2 * j];
    for (int k0 = 0; k0 < red16; k0 += 16) {
        float an[8];
        BFrag n0, n1;
        if (k0 + 16 < red16) {
            n0 = load_bfrag(bg, off0 + (k0 + 16) * ldb, ldb);
            n1 = load_bfrag(bg, off1 + (k0 + 16) * ldb, ldb);
#pragma unroll
            for (int j = 0; j < 8; ++j) an[j] = ap[k0 + 16 + 2 * j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x0.x[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x1.x[j], acc1, 0, 0, 0);
        }
        if (k0 + 16 < red16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] = an[j]; x0.x[j] = n0.x[j]; x1.x[j] = n1.x[j]; }
        }
    }
}

// Fully unrolled sweep for a compile-time chunk count (NCH x 16 reduction steps, NACC accumulators): three chunks of B
// fragments are in flight (every launch starts with cold L2s and all CUs walk the layers in lock-step, so each weight
// chunk is a first-touch miss of ~2 k cycles), buffers rotate by NAME -- no register copies, no branches -- so that
// hipcc's waitcnt insertion can leave the younger chunks outstanding (vmcnt(N) instead of vmcnt(0)).
template <int NCH, int NACC>
__device__ __forceinline__ void mfma_sweep_static(const float* __restrict__ ap, const float* __restrict__ bg, int off0, int off1,
                                                  int ldb, f32x16& acc0, f32x16& acc1)
{
    constexpr int D = NCH < 3 ? NCH : 3;
    float xb[3][2][8];
    float a[2][8];
#pragma unroll
    for (int c = 0; c < D; ++c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            xb[c][0][j] = bg[(unsigned)(off0 + (16 * c + 2 * j) * ldb)];
            if (NACC == 2) xb[c][1][j] = bg[(unsigned)(off1 + (16 * c + 2 * j) * ldb)];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) a[0][j] = ap[2 * j];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        // load group: A fragments of the next chunk (LDS) and the refill of the B buffer chunk c-1 just released
        if (c + 1 < NCH) {
#pragma unroll
            for (int j = 0; j < 8; ++j) a[(c + 1) & 1][j] = ap[16 * (c + 1) + 2 * j];
        }
        if (c >= 1 && c - 1 + D < NCH) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                xb[(c - 1) % 3][0][j] = bg[(unsigned)(off0 + (16 * (c - 1 + D) + 2 * j) * ldb)];
                if (NACC == 2) xb[(c - 1) % 3][1][j] = bg[(unsigned)(off1 + (16 * (c - 1 + D) + 2 * j) * ldb)];
            }
        }
        // MFMA group, nothing in between: any other instruction between two MFMAs on the same accumulator costs
        // ~43 extra cycles (MI355X_MICROARCH.md, per-instruction constants), and the narrow layers have one accumulator
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {   // touch every operand of the group: ONE s_waitcnt in front instead of one per MFMA
            asm volatile("" : "+v"(a[c & 1][j]), "+v"(xb[c % 3][0][j]));
            if (NACC == 2) asm volatile("" : "+v"(xb[c % 3][1][j]));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c & 1][j], xb[c % 3][0][j], acc0, 0, 0, 0);
            if (NACC == 2) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c & 1][j], xb[c % 3][1][j], acc1, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Packed forward weights: per layer Wt[k][n] = W[n][k] for k < K16 = round16(K), n < N32 = round32(No), zero padded,
// at float offset wt_off of the packed buffer (vf_mlp_pack_weights) -- the forward B operand without any guard.
__global__ __launch_bounds__(kBlock) void k_mlp_pack_weights(const vf_mlp_desc d, const float* __restrict__ params,
                                                             float* __restrict__ packed)
{
    const vf_mlp_layer L = d.layer[blockIdx.y];
    if ((int)blockIdx.y >= d.n_layers) return;
    const int K16 = (L.K + 15) & ~15, N32 = (L.No + 31) & ~31;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < K16 * N32; idx += gridDim.x * kBlock) {
        const int k = idx / N32, n = idx - k * N32;
        packed[L.wt_off + idx] = (k < L.K && n < L.No) ? params[L.w_off + n * L.K + k] : 0.0f;
    }
    // data-gradient image: Wb[n][k] = W[n][k] for n < round16(No), k < round32(K), zero padded
    const int N16 = (L.No + 15) & ~15, K32 = (L.K + 31) & ~31;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < N16 * K32; idx += gridDim.x * kBlock) {
        const int n = idx / K32, k = idx - n * K32;
        packed[L.wb_off + idx] = (k < L.K && n < L.No) ? params[L.w_off + n * L.K + k] : 0.0f;
    }
    // register-chain image (vf_mlp_chain.hip): block (a, g) = A fragments of four reduction steps, float4 per lane
    const bool nat = L.src < 4;                       // reads an observation: natural k order
    const int G = nat ? (L.K + 7) >> 3 : ((L.K + 31) >> 5) * 4, NT = (L.No + 31) >> 5;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < NT * G * 256; idx += gridDim.x * kBlock) {
        const int j = idx & 3, l = (idx >> 2) & 63, blk = idx >> 8, a = blk / G, g = blk - a * G;
        const int n = 32 * a + (l & 31), h = l >> 5;
        const int k = nat ? 8 * g + 2 * j + h : 32 * (g >> 2) + 8 * (g & 3) + 4 * h + j;
        packed[L.wr_off + idx] = (k < L.K && n < L.No) ? params[L.w_off + n * L.K + k] : 0.0f;
    }
    // reverse-chain image: block (a, g), a < ceil(K / 32), g < ceil(No / 8): W[32 (g / 4) + 8 (g % 4) + 4 h + j][32 a + (l & 31)]
    const int GQ = (L.No + 7) >> 3, KT = (L.K + 31) >> 5;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < KT * GQ * 256; idx += gridDim.x * kBlock) {
        const int j = idx & 3, l = (idx >> 2) & 63, blk = idx >> 8, a = blk / GQ, g = blk - a * GQ;
        const int k = 32 * a + (l & 31), n = 32 * (g >> 2) + 8 * (g & 3) + 4 * (l >> 5) + j;
        packed[L.wq_off + idx] = (k < L.K && n < L.No) ? params[L.w_off + n * L.K + k] : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock, 2) void k_mlp_forward(const vf_mlp_desc d, const float* __restrict__ params,
                                                           const float* __restrict__ packed, const MlpIo io, int M)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const int rt = wave & 1, c0 = wave >> 1;
    const int ntiles = (M + kRows - 1) / kRows;
    VF_PROBE_INIT();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * kRows;
        const bool full = m0 + kRows <= M;                 // no row guards in the epilogue except on the last tile
        __syncthreads();                                   // previous tile is completely consumed
        VF_PROBE_AT(0);
        for (int b = 0; b < d.n_inputs; ++b) {              // observations -> LDS
            const int w = d.in_dim[b], wp16 = (w + 15) & ~15;   // zero padded to the MFMA chunk
            stage_rows<false>(lds + d.lds_off[b], d.lds_stride[b], io.in[b], w, nullptr, 0, m0, M, w, wp16);
        }
        VF_PROBE_AT(1);
        for (int li = 0; li < d.n_layers; ++li) {
            const vf_mlp_layer L = d.layer[li];
            const int red16 = (L.K + 15) & ~15, ct = (L.No + 31) >> 5, ldb = ct * 32;
            const int nacc = c0 + 2 < ct ? 2 : (c0 < ct ? 1 : 0);
            const float* bg = packed + L.wt_off;            // wave-uniform base, 32-bit lane offsets
            const int off0 = lk * ldb + c0 * 32 + lr, off1 = off0 + 64;
#ifndef VF_TEST_NO_PAD_ZERO                                 // (tools/exp_pad_poison.py: shows that the poison test fails without)
            if (L.src >= 4 && (L.K & 15)) {
                // a hidden source whose width is not a multiple of the 16-step MFMA chunk (a concatenation such as
                // features (+) action = 68 columns): the sweep reads [K, round16(K)) as well.  The packed weights are zero
                // there, but 0 x (whatever the recycled LDS region holds) is NaN for NaN / Inf bit patterns, which the ReLU
                // then turns into a silent 0.  Nobody else writes those columns: zero them (rows 64 x < 16 columns).
                float* pad = lds + d.lds_off[L.src] + L.src_col + L.K;
                const int np = red16 - L.K, ss = d.lds_stride[L.src];
                for (int i = tid; i < kRows * np; i += kBlock) pad[(i / np) * ss + (i % np)] = 0.0f;
            }
#endif
            __syncthreads();                               // inputs of this layer are in LDS
            VF_PROBE_AT(2);
            const float* As = lds + d.lds_off[L.src] + L.src_col;
            const int sa = d.lds_stride[L.src];
            const float* ap = As + (rt * 32 + lr) * sa + lk;
            f32x16 acc0 = {0}, acc1 = {0};
            const int nch = red16 >> 4;                    // 1 (K = 13, 3), 4 (K = 64), 8 (K = 128): unrolled sweeps; else generic
            if (nacc == 2) {
                if (nch == 8) mfma_sweep_static<8, 2>(ap, bg, off0, off1, ldb, acc0, acc1);
                else if (nch == 4) mfma_sweep_static<4, 2>(ap, bg, off0, off1, ldb, acc0, acc1);
                else if (nch == 1) mfma_sweep_static<1, 2>(ap, bg, off0, off1, ldb, acc0, acc1);
                else mfma_sweep_gb2(ap, bg, off0, off1, ldb, red16, load_bfrag(bg, off0, ldb), load_bfrag(bg, off1, ldb), acc0, acc1);
            } else if (nacc == 1) {
                if (nch == 8) mfma_sweep_static<8, 1>(ap, bg, off0, off1, ldb, acc0, acc1);
                else if (nch == 4) mfma_sweep_static<4, 1>(ap, bg, off0, off1, ldb, acc0, acc1);
                else if (nch == 1) mfma_sweep_static<1, 1>(ap, bg, off0, off1, ldb, acc0, acc1);
                else mfma_sweep_gb1(ap, bg, off0, ldb, red16, load_bfrag(bg, off0, ldb), acc0);
            }
            VF_PROBE_AT(5);
            // epilogue: bias + ReLU, into the destination region (LDS or global) and the optional saved copy
            const int rb = rt * 32 + 4 * lk;               // first row of this lane's accumulator column
            auto emit = [&](f32x16 acc, int ctile) {
                const int n = ctile * 32 + lr;
                if (n >= L.No) return;
                const float bn = params[L.b_off + n];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    float y = acc[reg] + bn;
                    y = act_fwd(y, L.relu);
                    acc[reg] = y;
                }
                if (L.dst < VF_MLP_OUT0) {
                    float* dl = lds + d.lds_off[L.dst] + L.dst_col + rb * d.lds_stride[L.dst] + n;
                    const int sd = d.lds_stride[L.dst];
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) dl[((reg & 3) + 8 * (reg >> 2)) * sd] = acc[reg];
                }
                float* gp = nullptr;                         // wave-uniform base of this tile's rows
                int ldg = 0;
                if (L.dst >= VF_MLP_OUT0) { gp = io.out[L.dst - VF_MLP_OUT0] + (size_t)m0 * L.No; ldg = L.No; }
                else if (L.save) { gp = L.save + (size_t)m0 * L.save_ld + L.dst_col; ldg = L.save_ld; }
                if (gp) {
                    const int o = rb * ldg + n;
                    if (full) {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) gp[(unsigned)(o + ((reg & 3) + 8 * (reg >> 2)) * ldg)] = acc[reg];
                    } else {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            const int ro = (reg & 3) + 8 * (reg >> 2);
                            if (m0 + rb + ro < M) gp[(unsigned)(o + ro * ldg)] = acc[reg];
                        }
                    }
                }
            };
            if (nacc >= 1) emit(acc0, c0);
            if (nacc == 2) emit(acc1, c0 + 2);
            VF_PROBE_AT(6);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Whole-network backward: block-private row tiles, layer-major sweep (see vf_mlp_bwd_desc)
// ------------------------------------------------------------------------------------------------
constexpr int kBwdThreads = 512;   // 8 waves: (row half) x (4 column tiles) for the data gradient, 2 dW tiles each

// Register prefetch of one [64][w] fp32 tile by 512 threads: `issue` starts the global loads one work item
// ahead, `park` writes them to LDS rows of stride `sa` (optionally masked by a second prefetched tile > 0,
// rows past the matrix and the pad columns w..wpad zeroed).  mode 1: 16-byte loads (w/4 a power of two,
// <= 4 per thread); mode 2: narrow tiles (w <= 16, 2 scalars per thread); mode 0: staged directly at park time.
struct TilePf {
    float4 v[4];
    static __device__ __forceinline__ int mode_of(const float* A, int lda, int w)
    {
        const int c4 = w >> 2;
        if ((w & 3) == 0 && c4 >= 1 && (c4 & (c4 - 1)) == 0 && c4 <= 32 && (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0) return 1;
        return w <= 16 ? 2 : 0;
    }
    __device__ __forceinline__ void issue(int mode, const float* __restrict__ A, int lda, int m0, int M, int w)
    {
        const int tid = threadIdx.x, rmax = M - 1 - m0;
        const float* Ab = A + (size_t)m0 * lda;               // wave-uniform base, 32-bit lane offsets
        if (mode == 1) {
            const int c4 = w >> 2, sh = 31 - __clz(c4), col = (tid & (c4 - 1)) << 2, r0 = tid >> sh, rstep = kBwdThreads >> sh;
            const int nj = rstep >= kRows ? 1 : kRows / rstep;   // 4, 2 or 1 rows per thread
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nj) v[j] = *reinterpret_cast<const float4*>(Ab + (unsigned)(min(r0 + j * rstep, rmax) * lda + col));
        } else if (mode == 2) {
            const int total = kRows * w;
            float t[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = min(tid + j * kBwdThreads, total - 1), r = idx / w, k = idx - r * w;
                t[j] = Ab[(unsigned)(min(r, rmax) * lda + k)];
            }
            v[0].x = t[0]; v[0].y = t[1];
        }
    }
    __device__ __forceinline__ void park(int mode, float* __restrict__ As, int sa, int m0, int M, int w, int wpad, const TilePf* ym,
                                         int act = VF_ACTIVATION_RELU) const
    {
        const int tid = threadIdx.x, rmax = M - 1 - m0;
        if (wpad > w) {                                        // pad columns hold stale words of another layer
            const int pw = wpad - w;
            for (int idx = tid; idx < kRows * pw; idx += kBwdThreads) {
                const int r = idx / pw, k = w + idx - r * pw;
                As[r * sa + k] = 0.0f;
            }
        }
        if (mode == 1) {
            const int c4 = w >> 2, sh = 31 - __clz(c4), col = (tid & (c4 - 1)) << 2, r0 = tid >> sh, rstep = kBwdThreads >> sh;
            const int nj = rstep >= kRows ? 1 : kRows / rstep;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nj) {
                    const int r = r0 + j * rstep;
                    float4 x = v[j];
                    if (ym) {
                        const float4 y = ym->v[j];
                        x.x = act_mul(x.x, y.x, act); x.y = act_mul(x.y, y.y, act);
                        x.z = act_mul(x.z, y.z, act); x.w = act_mul(x.w, y.w, act);
                    }
                    const bool ok = r <= rmax;
                    if (r < kRows) {
                        float* d = As + r * sa + col;
                        d[0] = ok ? x.x : 0.0f; d[1] = ok ? x.y : 0.0f; d[2] = ok ? x.z : 0.0f; d[3] = ok ? x.w : 0.0f;
                    }
                }
            }
        } else if (mode == 2) {
            const int total = kRows * w;
            const float t[2] = {v[0].x, v[0].y};
            const float ty[2] = {ym ? ym->v[0].x : 1.0f, ym ? ym->v[0].y : 1.0f};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + j * kBwdThreads;
                if (idx < total) {
                    const int r = idx / w, k = idx - r * w;
                    As[r * sa + k] = r <= rmax ? (ym ? act_mul(t[j], ty[j], act) : t[j]) : 0.0f;
                }
            }
        }
    }
};

// Work items of a block: (layer, tile) in layer-major order over the block's own tiles.  While the MFMAs of item
// i run on LDS buffer i&1, the global loads of item i+1 (saved input X, saved output Y for the ReLU mask and --
// when its producer is not item i itself -- the upstream gradient dY) are in flight into registers; they are
// parked in the other buffer behind one barrier.  The data-gradient B operand streams from the packed weights.
__global__ __launch_bounds__(kBwdThreads) void k_mlp_backward(const vf_mlp_bwd_desc d, const float* __restrict__ packed,
                                                            float* __restrict__ part, int M)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const int rt = wave & 1, c0 = wave >> 1;   // c0 = 0..3: this wave's 32-column tile of dX
    const int mtiles = (M + kRows - 1) / kRows;
    const int T = (mtiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // tiles of this block (>= 1)
    const int nitems = d.n_layers * T;
    const bool early_dy = T >= 2;              // with one tile per block the producer of the next dY is the current item
    constexpr int kBuf = kRows * (129 + 129);  // floats per staging buffer (max strides)
    float* Bs = lds + 2 * kBuf;                // [kBwdThreads] bias partial sums
    float* prow = part + (size_t)blockIdx.x * d.n_fold;
    VF_PROBE_INIT();

    TilePf pfX, pfY, pfD;
    auto geometry = [&](const vf_mlp_bwd_layer& L, int& sd, int& sx) {
        sd = ((L.No + 31) & ~31) + 1;
        sx = ((L.K + 31) & ~31) + 1;
    };
    auto modes = [&](const vf_mlp_bwd_layer& L, int& mx, int& md) {
        mx = TilePf::mode_of(L.X, L.ld_x, L.K);
        md = TilePf::mode_of(L.dY, L.ld_dy, L.No);
        if (L.Y && TilePf::mode_of(L.Y, L.ld_y, L.No) != md) md = 0;   // mask and gradient must share the thread mapping
    };
    auto park_item = [&](const vf_mlp_bwd_layer& L, int m0, float* buf, bool dy_late) {
        int sd, sx, mx, md;
        geometry(L, sd, sx);
        modes(L, mx, md);
        float* Ds = buf;
        float* Xs = buf + kRows * sd;
        if (dy_late && md) {
            pfD.issue(md, L.dY, L.ld_dy, m0, M, L.No);
        }
        if (mx) pfX.park(mx, Xs, sx, m0, M, L.K, sx - 1, nullptr);
        else {
            if (sx - 1 > L.K) pfX.park(0, Xs, sx, m0, M, L.K, sx - 1, nullptr);   // pads only
            stage_rows<false, kBwdThreads>(Xs, sx, L.X, L.ld_x, nullptr, 0, m0, M, L.K, L.K);
        }
        if (md) pfD.park(md, Ds, sd, m0, M, L.No, sd - 1, L.Y ? &pfY : nullptr, L.act);
        else {
            if (sd - 1 > L.No) pfD.park(0, Ds, sd, m0, M, L.No, sd - 1, nullptr);
            stage_rows<true, kBwdThreads>(Ds, sd, L.dY, L.ld_dy, L.Y, L.ld_y, m0, M, L.No, L.No, kRows, L.act);
        }
    };
    auto issue_item = [&](const vf_mlp_bwd_layer& L, int m0, bool with_dy) {
        int mx, md;
        modes(L, mx, md);
        if (mx) pfX.issue(mx, L.X, L.ld_x, m0, M, L.K);
        if (md && L.Y) pfY.issue(md, L.Y, L.ld_y, m0, M, L.No);
        if (md && with_dy) pfD.issue(md, L.dY, L.ld_dy, m0, M, L.No);
    };

    {   // item 0
        const int m0 = (int)blockIdx.x * kRows;
        issue_item(d.layer[0], m0, true);
        park_item(d.layer[0], m0, lds, false);
    }
    __syncthreads();
    VF_PROBE_AT(8);

    f32x16 acc[2] = {{0}, {0}};
    float bsum = 0.0f;
    int li = 0, ti = 0;                        // layer / tile index of the current item
    for (int it = 0; it < nitems; ++it) {
        const vf_mlp_bwd_layer L = d.layer[li];
        const int K = L.K, No = L.No;
        const int nt = (No + 31) >> 5, kt = (K + 31) >> 5;
        const int sd = nt * 32 + 1, sx = kt * 32 + 1, ldb = kt * 32, red16 = (No + 15) & ~15;
        float* buf = lds + (it & 1) * kBuf;
        const float* Ds = buf;
        const float* Xs = buf + kRows * sd;
        const int m0 = ((int)blockIdx.x + ti * (int)gridDim.x) * kRows;
        const int nli = ti + 1 == T ? li + 1 : li, nti = ti + 1 == T ? 0 : ti + 1;   // next item
        const bool has_next = it + 1 < nitems;
        const int nm0 = ((int)blockIdx.x + nti * (int)gridDim.x) * kRows;
        if (has_next) issue_item(d.layer[nli], nm0, early_dy);
        const int nacc = c0 < kt ? 1 : 0;
        const float* bg = packed + L.wb_off;   // wave-uniform base, 32-bit lane offsets
        const int off0 = lk * ldb + c0 * 32 + lr;
        BFrag x0;
        if (L.need_dx && nacc) x0 = load_bfrag(bg, off0, ldb);
        VF_PROBE_AT(9);
        const int cgrp = No <= 64 ? 64 : 128;
        {   // bias gradient: thread = (column, row slice)
            const int c = tid & (cgrp - 1), sl = tid / cgrp, rows = kRows * cgrp / kBwdThreads;
            if (c < No) {
                float s0 = 0.0f, s1 = 0.0f;
                const float* dp = Ds + (sl * rows) * sd + c;
                for (int r = 0; r < rows; r += 2) { s0 += dp[r * sd]; s1 += dp[(r + 1) * sd]; }
                bsum += s0 + s1;
            }
        }
        const int wtiles = nt * kt;            // <= 16 weight-gradient tiles of 32x32; wave takes wave, wave+8
#pragma unroll
        for (int q = 0; q < 2; ++q) {          // dW[n][k] += sum_m dYm[m][n] X[m][k]
            const int wt = wave + 8 * q;
            if (wt >= wtiles) break;
            const int itn = wt / kt, jt = wt - itn * kt;
            const float* ap = Ds + lk * sd + itn * 32 + lr;
            const float* bp = Xs + lk * sx + jt * 32 + lr;
            f32x16 c = acc[q];
#pragma unroll
            for (int k0 = 0; k0 < kRows; k0 += 16) {
                float fa[8], fb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { fa[j] = ap[(k0 + 2 * j) * sd]; fb[j] = bp[(k0 + 2 * j) * sx]; }
#pragma unroll
                for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j], fb[j], c, 0, 0, 0);
            }
            acc[q] = c;
        }
        VF_PROBE_AT(13);
        if (L.need_dx && nacc) {               // dX[m][k] = sum_n dYm[m][n] W[n][k]
            const float* ap = Ds + (rt * 32 + lr) * sd + lk;
            f32x16 a = {0};
            mfma_sweep_gb1(ap, bg, off0, ldb, red16, x0, a);
            float* dxb = L.dX + (size_t)m0 * L.ld_dx;   // wave-uniform base of this tile's rows
            const int n = c0 * 32 + lr;
            if (n < K) {
                const int rb = rt * 32 + 4 * lk, o = rb * L.ld_dx + n, rmax = M - 1 - m0 - rb;
                if (L.need_dx == 2) {          // second consumer of the same activation: add (all loads first)
                    float old[16];
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        old[reg] = dxb[(unsigned)(min(rb + (reg & 3) + 8 * (reg >> 2), M - 1 - m0) * L.ld_dx + n)];   // rows past M: clamped, never stored
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) a[reg] += old[reg];
                }
                if (rmax >= 27) {              // every row of this lane's column exists
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) dxb[(unsigned)(o + ((reg & 3) + 8 * (reg >> 2)) * L.ld_dx)] = a[reg];
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int ro = (reg & 3) + 8 * (reg >> 2);
                        if (ro <= rmax) dxb[(unsigned)(o + ro * L.ld_dx)] = a[reg];
                    }
                }
            }
        }
        VF_PROBE_AT(14);
        const bool layer_done = ti + 1 == T;
        if (layer_done) {                      // one partial per layer and block: weights, then the bias column sums
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int wt = wave + 8 * q;
                if (wt >= wtiles) break;
                const int itn = wt / kt, jt = wt - itn * kt;
                const int k = jt * 32 + lr;
                if (k < K) {
                    float* pw = prow + L.w_off;    // wave-uniform base
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int n = itn * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lk;
                        if (n < No) pw[(unsigned)(n * K + k)] = acc[q][reg];
                    }
                }
                acc[q] = f32x16{0};
            }
            Bs[tid] = bsum;
            bsum = 0.0f;
        }
        VF_PROBE_AT(10);
        __syncthreads();                       // buffer it&1 is consumed, this item's dX stores have completed
        VF_PROBE_AT(15);
        if (layer_done && tid < No) {
            float t = 0.0f;
            const int nsl = kBwdThreads / cgrp;
            for (int q = 0; q < nsl; ++q) t += Bs[q * cgrp + tid];
            prow[L.b_off + tid] = t;
        }
        if (has_next) park_item(d.layer[nli], nm0, lds + ((it + 1) & 1) * kBuf, !early_dy);
        VF_PROBE_AT(11);
        __syncthreads();
        VF_PROBE_AT(12);
        li = nli; ti = nti;
    }
}

int check_fwd_desc(const vf_mlp_desc* desc, const char* who, int flags)
{
    const bool inputs = flags & kFwdDescInputs;
    if (!desc || desc->n_layers < 1 || desc->n_layers > VF_MLP_MAX_LAYERS || (inputs && (desc->n_inputs < 1 || desc->n_inputs > 4)))
        return fail(VF_EINVAL, inputs ? "%s: bad layer / input count" : "%s: bad layer count", who);
    if (flags & kFwdDescDims) {
        for (int i = 0; i < desc->n_layers; ++i) {
            const vf_mlp_layer& L = desc->layer[i];
            if (L.K < 1 || L.K > kLinearNarrowMax || L.No < 1 || L.No > kLinearNarrowMax)
                return fail(VF_EINVAL, "%s: layer %d: K, No must be 1..%d", who, i, kLinearNarrowMax);
        }
    }
    return VF_OK;
}

int check_bwd_desc(const vf_mlp_bwd_desc* desc, const char* who)
{
    if (!desc || desc->n_layers < 1 || desc->n_layers > VF_MLP_MAX_LAYERS || desc->n_fold < 1) return fail(VF_EINVAL, "%s: bad layer count / n_fold", who);
    for (int i = 0; i < desc->n_layers; ++i) {
        const vf_mlp_bwd_layer& L = desc->layer[i];
        if (L.K < 1 || L.K > kLinearNarrowMax || L.No < 1 || L.No > kLinearNarrowMax)
            return fail(VF_EINVAL, "%s: layer %d: K, No must be 1..%d", who, i, kLinearNarrowMax);
        if (!L.dY || !L.X || L.ld_dy < L.No || L.ld_x < L.K || (L.Y && L.ld_y < L.No) || (L.need_dx && (!L.dX || L.ld_dx < L.K)))
            return fail(VF_EINVAL, "%s: layer %d: missing pointer or short row stride", who, i);
        if (L.w_off < 0 || L.b_off < 0 || L.w_off + (int64_t)L.K * L.No > desc->n_fold || L.b_off + L.No > desc->n_fold)
            return fail(VF_EINVAL, "%s: layer %d: parameter offsets outside n_fold", who, i);
    }
    return VF_OK;
}

}  // namespace vf

// Fold the parameter ranges the listed layers cover (a skipped trunk leaves its columns of `partials` unwritten): the weight and
// bias ranges sorted and coalesced, one fold launch per disjoint range
static void fold_covered_ranges(const vf_mlp_bwd_desc* desc, const float* partials, int nblk, float* grad, int accumulate, hipStream_t st)
{
    std::pair<int64_t, int64_t> iv[2 * VF_MLP_MAX_LAYERS];
    int niv = 0;
    for (int i = 0; i < desc->n_layers; ++i) {
        const vf_mlp_bwd_layer& L = desc->layer[i];
        iv[niv++] = {L.w_off, L.w_off + (int64_t)L.K * L.No};
        iv[niv++] = {L.b_off, L.b_off + L.No};
    }
    std::sort(iv, iv + niv);
    for (int i = 0; i < niv;) {
        int64_t lo = iv[i].first, hi = iv[i].second;
        int j = i + 1;
        while (j < niv && iv[j].first <= hi) { hi = iv[j].second > hi ? iv[j].second : hi; ++j; }
        vf::fold_partials_launch(partials + lo, nblk, desc->n_fold, (int)(hi - lo), 0, grad + lo, nullptr, accumulate ? 1 : 0, st);
        i = j;
    }
}

// what an entry point that only the chain class table serves returns for the answer of a *_chain_try call
static int chain_only(int rc, const char* who, const char* variant = "")
{
    if (rc < 0) return rc;
    return rc ? VF_OK : vf::fail(VF_EUNSUPPORTED, "%s: the layer table is not an instantiated network class%s", who, variant);
}

extern "C" {

int64_t vf_mlp_packed_floats(const vf_mlp_desc* desc)
{
    if (vf::check_fwd_desc(desc, "vf_mlp_packed_floats")) return -1;
    int64_t n = 0;
    for (int i = 0; i < desc->n_layers; ++i) {
        const vf_mlp_layer& L = desc->layer[i];
        const int64_t end = L.wt_off + (int64_t)((L.K + 15) & ~15) * ((L.No + 31) & ~31);
        const int64_t endb = L.wb_off + (int64_t)((L.No + 15) & ~15) * ((L.K + 31) & ~31);
        const int64_t G = L.src < 4 ? (L.K + 7) >> 3 : ((L.K + 31) >> 5) * 4;
        const int64_t endr = L.wr_off + (int64_t)((L.No + 31) >> 5) * G * 256;
        const int64_t endq = L.wq_off + (int64_t)((L.K + 31) >> 5) * ((L.No + 7) >> 3) * 256;
        n = std::max({n, end, endb, endr, endq});
    }
    return n;
}

int vf_mlp_pack_weights(const vf_mlp_desc* desc, const float* params, float* packed, vf_stream_t stream)
{
    if (!desc || !params || !packed) return vf::fail(VF_EINVAL, "vf_mlp_pack_weights: bad argument");
    if (int rc = vf::check_fwd_desc(desc, "vf_mlp_pack_weights")) return rc;
    hipLaunchKernelGGL(vf::k_mlp_pack_weights, dim3(8, desc->n_layers), dim3(vf::kBlock), 0, vf::as_stream(stream), *desc, params,
                       packed);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_mlp_forward(const vf_mlp_desc* desc, const float* params, const float* packed, const float* in0, const float* in1,
                   const float* in2, const float* in3, float* out0, float* out1, int32_t M, vf_stream_t stream)
{
    if (!desc || !params || !packed || !in0 || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_forward: bad argument");
    if (int rc = vf::check_fwd_desc(desc, "vf_mlp_forward", vf::kFwdDescInputs | vf::kFwdDescDims)) return rc;
    // reference-default network shapes: activations chained through MFMA accumulator registers (vf_mlp_chain.hip);
    // out1 == NULL there means "skip the value trunk"
    if (int rc = vf::mlp_forward_chain_try(desc, params, packed, in0, in1, out0, out1, M, vf::as_stream(stream), nullptr, in2)) return rc < 0 ? rc : VF_OK;
    for (int i = 0; i < desc->n_layers; ++i) {
        const vf_mlp_layer& L = desc->layer[i];
        if (L.dst >= VF_MLP_OUT0 && !(L.dst == VF_MLP_OUT0 ? out0 : out1))
            return vf::fail(L.dst == VF_MLP_OUT1 ? VF_EUNSUPPORTED : VF_EINVAL, "vf_mlp_forward: missing output %d", L.dst);
    }
    const size_t lds = (size_t)desc->lds_floats * sizeof(float);
    if (lds > 160 * 1024) return vf::fail(VF_EINVAL, "vf_mlp_forward: LDS plan needs %zu bytes (> 160 KiB)", lds);
    if (int rc = vf::allow_lds(vf::k_mlp_forward, lds)) return rc;
    const int ntiles = (M + vf::kRows - 1) / vf::kRows;
    const int per_cu = lds <= 80 * 1024 ? 2 : 1;           // workgroups that fit one CU's 160 KiB
    const int cap = 256 * per_cu;
    vf::MlpIo io{{in0, in1, in2, in3}, {out0, out1}};
    hipLaunchKernelGGL(vf::k_mlp_forward, dim3(ntiles < cap ? ntiles : cap), dim3(vf::kBlock), lds, vf::as_stream(stream), *desc,
                       params, packed, io, M);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

#ifdef VF_PROBE
int vf_probe_read(unsigned long long* out, int32_t reset)
{
    VF_HIP(hipDeviceSynchronize());
    VF_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(vf::g_probe), sizeof(unsigned long long) * 32));
    if (reset) {
        unsigned long long z[32] = {0};
        VF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(vf::g_probe), z, sizeof(z)));
    }
    return VF_OK;
}
#endif

int32_t vf_mlp_backward_blocks(int32_t M)
{
    if (M <= 0) return 0;
    const int mtiles = (M + vf::kRows - 1) / vf::kRows;
    const int rounds = (mtiles + 255) / 256;      // tiles per block: equal work, at most one (8-wave) block per CU
    return (mtiles + rounds - 1) / rounds;
}

int64_t vf_mlp_backward_partial_floats(const vf_mlp_bwd_desc* desc, int32_t M)
{
    if (!desc || desc->n_layers < 1 || desc->n_layers > VF_MLP_MAX_LAYERS || M <= 0) return -1;
    const int64_t a = (int64_t)vf_mlp_backward_blocks(M) * desc->n_fold, b = vf::mlp_wgrad_partial_floats(desc, M);
    return a > b ? a : b;
}

int vf_mlp_backward(const vf_mlp_bwd_desc* desc, const float* packed, float* partials, float* grad, int32_t M,
                    int32_t accumulate, vf_stream_t stream)
{
    if (!desc || !packed || !partials || !grad || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_backward: bad argument");
    if (int rc = vf::check_bwd_desc(desc, "vf_mlp_backward")) return rc;
    hipStream_t st = vf::as_stream(stream);
    // reference-default network classes: reverse chain in registers + row-slab weight gradients (vf_mlp_chain.hip, vf_mlp_wgrad.hip)
    if (int rc = vf::mlp_backward_chain_try(desc, packed, M, st)) {
        if (rc < 0) return rc;
        return vf::mlp_wgrad_launch(desc, partials, grad, M, accumulate, nullptr, nullptr, st);
    }
    const size_t lds = ((size_t)2 * vf::kRows * (129 + 129) + vf::kBwdThreads) * sizeof(float);   // two staging buffers + bias scratch
    if (int rc = vf::allow_lds(vf::k_mlp_backward, lds)) return rc;
    const int nblk = vf_mlp_backward_blocks(M);
    hipLaunchKernelGGL(vf::k_mlp_backward, dim3(nblk), dim3(vf::kBwdThreads), lds, st, *desc, packed, partials, M);
    fold_covered_ranges(desc, partials, nblk, grad, accumulate, st);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

int vf_mlp_backward_data_supported(const vf_mlp_bwd_desc* desc)
{
    if (vf::check_bwd_desc(desc, "vf_mlp_backward_data_supported")) return 0;
    return vf::mlp_backward_chain_try(desc, nullptr, 1, nullptr) == 1 ? 1 : 0;
}

int vf_mlp_backward_data(const vf_mlp_bwd_desc* desc, const float* packed, int32_t M, vf_stream_t stream)
{
    if (!packed || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_backward_data: bad argument");
    if (int rc = vf::check_bwd_desc(desc, "vf_mlp_backward_data")) return rc;
    return chain_only(vf::mlp_backward_chain_try(desc, packed, M, vf::as_stream(stream)), "vf_mlp_backward_data", " / variant");
}

int vf_mlp_forward_steps(const vf_mlp_desc* desc, const float* params, const float* packed, const float* in0, const float* in1,
                         const float* in2, float* out0, float* out1, int32_t M_step, int32_t n_steps, vf_stream_t stream)
{
    if (!desc || !params || !packed || !in0 || !out0 || M_step <= 0 || n_steps <= 0) return vf::fail(VF_EINVAL, "vf_mlp_forward_steps: bad argument");
    if (int rc = vf::check_fwd_desc(desc, "vf_mlp_forward_steps", vf::kFwdDescInputs)) return rc;
    if (M_step & 31) return vf::fail(VF_EUNSUPPORTED, "vf_mlp_forward_steps: M_step must be a multiple of 32 (whole row tiles per step)");
    if ((int64_t)M_step * n_steps > 0x7fffffff) return vf::fail(VF_EINVAL, "vf_mlp_forward_steps: M_step x n_steps passes 2^31 rows");
    for (int i = 0; i < desc->n_layers; ++i)
        if (desc->layer[i].save) return vf::fail(VF_EINVAL, "vf_mlp_forward_steps: inference only (no saved activations)");
    return chain_only(vf::mlp_forward_chain_try(desc, params, packed, in0, in1, out0, out1, M_step * n_steps, vf::as_stream(stream), nullptr, in2, M_step),
                      "vf_mlp_forward_steps");
}

int vf_mlp_forward_act(const vf_mlp_desc* desc, const float* params, const float* packed, const float* in0, const float* in1,
                       const float* log_std, const float* eps, float* action, float* obs_copy0, float* obs_copy1, int32_t M,
                       vf_stream_t stream)
{
    if (!desc || !params || !packed || !in0 || !log_std || !eps || !action || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_forward_act: bad argument");
    if (int rc = vf::check_fwd_desc(desc, "vf_mlp_forward_act")) return rc;
    const vf::ReparamFwd rp{log_std, eps, action, {obs_copy0, obs_copy1}};
    return chain_only(vf::mlp_forward_chain_try(desc, params, packed, in0, in1, nullptr, nullptr, M, vf::as_stream(stream), &rp), "vf_mlp_forward_act");
}

int vf_mlp_backward_data_act(const vf_mlp_bwd_desc* desc, const float* packed, const float* d_action, const float* action,
                             const float* log_std, const float* eps, float* g_log_std, int32_t M, vf_stream_t stream)
{
    if (!packed || !d_action || !action || !log_std || !eps || !g_log_std || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_backward_data_act: bad argument");
    if (int rc = vf::check_bwd_desc(desc, "vf_mlp_backward_data_act")) return rc;
    const vf::ReparamBwd rp{d_action, action, log_std, eps, g_log_std};
    return chain_only(vf::mlp_backward_chain_try(desc, packed, M, vf::as_stream(stream), &rp), "vf_mlp_backward_data_act", " / variant");
}

int vf_mlp_weight_grad(const vf_mlp_bwd_desc* desc, float* partials, float* grad, int32_t M, int32_t accumulate, vf_stream_t stream)
{
    if (!partials || !grad || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_weight_grad: bad argument");
    if (int rc = vf::check_bwd_desc(desc, "vf_mlp_weight_grad")) return rc;
    return vf::mlp_wgrad_launch(desc, partials, grad, M, accumulate, nullptr, nullptr, vf::as_stream(stream));
}

int32_t vf_mlp_weight_grad_fold_blocks(const vf_mlp_bwd_desc* desc)
{
    if (vf::check_bwd_desc(desc, "vf_mlp_weight_grad_fold_blocks")) return -1;
    return vf::mlp_wgrad_fold_blocks(desc);
}

int vf_mlp_weight_grad_sumsq(const vf_mlp_bwd_desc* desc, float* partials, float* grad, int32_t M, int32_t accumulate,
                             double* sumsq_partials, const vf_stats_fold* loss_stats, vf_stream_t stream)
{
    if (!partials || !grad || !sumsq_partials || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_weight_grad_sumsq: bad argument");
    if (loss_stats && (!loss_stats->part || !loss_stats->stats || loss_stats->n_rows < 1))
        return vf::fail(VF_EINVAL, "vf_mlp_weight_grad_sumsq: bad loss_stats");
    if (int rc = vf::check_bwd_desc(desc, "vf_mlp_weight_grad_sumsq")) return rc;
    return vf::mlp_wgrad_launch(desc, partials, grad, M, accumulate, sumsq_partials, loss_stats, vf::as_stream(stream));
}

int vf_mlp_weight_grad_layers(const vf_mlp_bwd_desc* desc, float* partials, float* grad, int32_t M, int32_t accumulate, uint32_t layer_mask,
                              vf_stream_t stream)
{
    if (!partials || !grad || M <= 0) return vf::fail(VF_EINVAL, "vf_mlp_weight_grad_layers: bad argument");
    if (int rc = vf::check_bwd_desc(desc, "vf_mlp_weight_grad_layers")) return rc;
    return vf::mlp_wgrad_launch_layers(desc, partials, grad, M, accumulate, layer_mask, vf::as_stream(stream));
}

}  // extern "C"
