// nn.LayerNorm(W, eps) + activation between a hidden nn.Linear and the next layer (create_mlp with `ln`, utils/policies/extractors.py:
// 428-430), forward and backward, row-wise in fp32.  Memory-bound: a row is read once and stays in registers for both passes.
//
// A row of W <= 512 values is held by a GROUP of G lanes of one wave64, NV values per lane (G * NV >= W); a wave works on 64 / G rows
// at a time, so narrow rows (W <= 32) leave no lane idle.  Two register layouts:
//   scalar   lane l holds columns l + G j, j < NV                          any W, any pointer, any leading dimension
//   vector   lane l holds columns 4 (l + G q) .. + 3, q < NV / 4           one 16-byte access per q: W, the row pointers and the leading
//                                                                            dimensions multiples of 4 floats (gamma / beta stay scalar:
//                                                                            their offsets in the flat parameter buffer are arbitrary)
// Sums over a row are xor-butterflies over the group's lanes (every lane ends with the same bits); no LDS.
//
// forward    mean = sum z / W, refined once by the mean of the residuals (z - mean): the centred values then carry the rounding of a
//            subtraction, not of a sum of W terms -- a row of 1000 + N(0, 1) keeps its seven digits.  var = sum (z - mean)^2 / W
//            (biased, over the centred registers; never E[z^2] - mean^2), rstd = 1 / sqrt(var + eps) with IEEE sqrt and division,
//            xhat = (z - mean) rstd, y = act(gamma xhat + beta).  xhat and rstd are what the backward needs; xhat may alias z.
// backward   g = dy act'(y) (act_mul of vf_common.hpp), h = g gamma, dz = rstd (h - mean(h) - xhat mean(h xhat)); dz may alias dy.
//            dgamma = sum_rows g xhat and dbeta = sum_rows g: every wave owns a contiguous range of rows, adds its rows in order in
//            registers and writes ONE partial of 2 W floats; k_fold_partials (vf_linear.hip) adds the partials in a fixed order.
//            No floating-point atomics: bit-identical from run to run.
#include "vf_common.hpp"

namespace vf {
namespace {

constexpr int kLnMaxWidth = 512;     // MAX_WIDTH of visfly_amd/ppo.py: 8 values per lane of a whole wave
constexpr int kLnMaxPartials = 2048; // waves of a backward launch = partial rows of dgamma / dbeta

template <int G, int NV, bool VEC>
struct LnRow {
    static_assert(!VEC || NV % 4 == 0, "vector layout: whole float4s");
    static __device__ __forceinline__ int col(int l, int j) { return VEC ? 4 * (l + G * (j >> 2)) + (j & 3) : l + G * j; }
    // p: the row's first element, or nullptr for a row past the end (zeros)
    static __device__ __forceinline__ void load(const float* p, int l, int W, float (&v)[NV])
    {
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < NV / 4; ++q) {
                const int c = 4 * (l + G * q);
                float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p && c < W) t = *reinterpret_cast<const float4*>(p + c);
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = l + G * j;
                v[j] = (p && c < W) ? p[c] : 0.0f;
            }
        }
    }
    static __device__ __forceinline__ void store(float* p, int l, int W, const float (&v)[NV])
    {
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < NV / 4; ++q) {
                const int c = 4 * (l + G * q);
                if (p && c < W) *reinterpret_cast<float4*>(p + c) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = l + G * j;
                if (p && c < W) p[c] = v[j];
            }
        }
    }
    // per-column vectors (gamma, beta): scalar loads in either layout
    static __device__ __forceinline__ void load_cols(const float* p, int l, int W, float (&v)[NV])
    {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = col(l, j) < W ? p[col(l, j)] : 0.0f;
    }
};

// sum over the G lanes of a group; every lane of the group gets the same bits (a + b == b + a)
template <int G>
__device__ __forceinline__ float group_sum(float x)
{
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <int NV>
__device__ __forceinline__ float lane_sum(const float (&v)[NV])
{
    float s = v[0];
#pragma unroll
    for (int j = 1; j < NV; ++j) s += v[j];
    return s;
}

template <int G, int NV, bool VEC>
__global__ __launch_bounds__(kBlock) void k_layernorm_fwd(const float* z, int ldz, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float* __restrict__ y, int ldy,
                                                          float* xhat, int ldx, float* __restrict__ rstd_out, int M, int W, int act)
{
    using R = LnRow<G, NV, VEC>;
    constexpr int RPW = 64 / G;
    const int lane = threadIdx.x & 63, l = lane % G, sub = lane / G;
    const long long row = ((long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * RPW + sub;
    const bool live = row < M;
    float v[NV], ga[NV], be[NV];
    R::load(live ? z + (size_t)row * ldz : nullptr, l, W, v);
    R::load_cols(gamma, l, W, ga);
    R::load_cols(beta, l, W, be);
    const float w = (float)W;
    const float mean0 = group_sum<G>(lane_sum<NV>(v)) / w;
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = R::col(l, j) < W ? v[j] - mean0 : 0.0f;
    const float dm = group_sum<G>(lane_sum<NV>(v)) / w;
    float sq[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        v[j] = R::col(l, j) < W ? v[j] - dm : 0.0f;
        sq[j] = v[j] * v[j];
    }
    const float var = group_sum<G>(lane_sum<NV>(sq)) / w;
    const float rstd = 1.0f / sqrtf(var + eps);
    float out[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        v[j] = v[j] * rstd;
        out[j] = act_fwd(ga[j] * v[j] + be[j], act);
    }
    R::store(live ? xhat + (size_t)row * ldx : nullptr, l, W, v);
    R::store(live ? y + (size_t)row * ldy : nullptr, l, W, out);
    if (live && l == 0) rstd_out[row] = rstd;
}

// wave `gw` owns rows [gw rows_per_wave, (gw + 1) rows_per_wave) and writes part[gw][0 .. W) = its dgamma, [W .. 2 W) = its dbeta
template <int G, int NV, bool VEC>
__global__ __launch_bounds__(kBlock) void k_layernorm_bwd(const float* dy, int lddy, const float* __restrict__ y, int ldy,
                                                          const float* __restrict__ xhat, int ldx, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, float* dz, int lddz, float* __restrict__ part,
                                                          int M, int W, int act, int rows_per_wave, int n_waves)
{
    using R = LnRow<G, NV, VEC>;
    constexpr int RPW = 64 / G;
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
    if (gw >= n_waves) return;
    const int lane = threadIdx.x & 63, l = lane % G, sub = lane / G;
    const long long lo = (long long)gw * rows_per_wave;
    const long long hi = lo + rows_per_wave < (long long)M ? lo + rows_per_wave : (long long)M;
    float ga[NV], acc_g[NV], acc_b[NV];
    R::load_cols(gamma, l, W, ga);
#pragma unroll
    for (int j = 0; j < NV; ++j) acc_g[j] = acc_b[j] = 0.0f;
    const float w = (float)W;
    for (long long r0 = lo; r0 < hi; r0 += RPW) {
        const long long row = r0 + sub;
        const bool live = row < hi;
        float g[NV], x[NV], yy[NV], h[NV], hx[NV];
        R::load(live ? dy + (size_t)row * lddy : nullptr, l, W, g);
        R::load(live ? xhat + (size_t)row * ldx : nullptr, l, W, x);
        if (act != VF_ACTIVATION_NONE) {
            R::load(live ? y + (size_t)row * ldy : nullptr, l, W, yy);
#pragma unroll
            for (int j = 0; j < NV; ++j) g[j] = act_mul(g[j], yy[j], act);
        }
        const float rs = live ? rstd[row] : 0.0f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            acc_b[j] += g[j];
            acc_g[j] += g[j] * x[j];
            h[j] = g[j] * ga[j];
            hx[j] = h[j] * x[j];
        }
        const float m1 = group_sum<G>(lane_sum<NV>(h)) / w;
        const float m2 = group_sum<G>(lane_sum<NV>(hx)) / w;
#pragma unroll
        for (int j = 0; j < NV; ++j) h[j] = rs * ((h[j] - m1) - x[j] * m2);
        R::store(live ? dz + (size_t)row * lddz : nullptr, l, W, h);
    }
    // the 64 / G groups of the wave hold the same columns: add them in a fixed order, group 0 writes
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int o = G; o < 64; o <<= 1) {
            acc_g[j] += __shfl_xor(acc_g[j], o, 64);
            acc_b[j] += __shfl_xor(acc_b[j], o, 64);
        }
    }
    if (sub == 0) {
        float* p = part + (size_t)gw * 2 * W;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = R::col(l, j);
            if (c < W) {
                p[c] = acc_g[j];
                p[W + c] = acc_b[j];
            }
        }
    }
}

int pow2_at_least(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

struct LnShape {
    int G, NV;
    bool vec;
};

// aligned: W, every row pointer and every leading dimension a multiple of 4 floats
LnShape ln_shape(int W, bool aligned)
{
    if (aligned && W >= 16) {
        const int q = W / 4;
        int G = pow2_at_least(q);
        G = G < 4 ? 4 : (G > 64 ? 64 : G);
        return {G, q > 64 ? 8 : 4, true};
    }
    int G = pow2_at_least(W);
    G = G < 4 ? 4 : (G > 64 ? 64 : G);
    return {G, W <= 64 ? 1 : pow2_at_least((W + 63) / 64), false};
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// calls F.template operator()<G, NV, VEC>() for the shape; the 14 instances of the two layouts
template <class F>
int ln_dispatch(const LnShape& s, F&& f)
{
#define VF_LN_CASE(g_, nv_, vec_) \
    if (s.G == g_ && s.NV == nv_ && s.vec == vec_) return f.template operator()<g_, nv_, vec_>();
    VF_LN_CASE(4, 4, true) VF_LN_CASE(8, 4, true) VF_LN_CASE(16, 4, true) VF_LN_CASE(32, 4, true) VF_LN_CASE(64, 4, true)
    VF_LN_CASE(64, 8, true)
    VF_LN_CASE(4, 1, false) VF_LN_CASE(8, 1, false) VF_LN_CASE(16, 1, false) VF_LN_CASE(32, 1, false) VF_LN_CASE(64, 1, false)
    VF_LN_CASE(64, 2, false) VF_LN_CASE(64, 4, false) VF_LN_CASE(64, 8, false)
#undef VF_LN_CASE
    return fail(VF_EINVAL, "vf_layernorm: no kernel for the row layout (%d lanes, %d values)", s.G, s.NV);
}

bool bad_ln_dims(int M, int W) { return M <= 0 || W <= 0 || W > kLnMaxWidth; }
bool bad_ln_act(int act) { return act < 0 || act > VF_ACTIVATION_LEAKY_RELU; }

struct LnFwd {
    const float* z; int ldz; const float *gamma, *beta; float eps; float* y; int ldy; float* xhat; int ldx; float* rstd;
    int M, W, act; hipStream_t st;
    template <int G, int NV, bool VEC>
    int operator()() const
    {
        constexpr int rows_per_block = (kBlock / 64) * (64 / G);
        const long long grid = ((long long)M + rows_per_block - 1) / rows_per_block;
        hipLaunchKernelGGL((k_layernorm_fwd<G, NV, VEC>), dim3((unsigned)grid), dim3(kBlock), 0, st, z, ldz, gamma, beta, eps, y, ldy, xhat,
                           ldx, rstd, M, W, act);
        VF_HIP(hipGetLastError());
        return VF_OK;
    }
};

struct LnBwd {
    const float* dy; int lddy; const float* y; int ldy; const float* xhat; int ldx; const float *rstd, *gamma; float* dz; int lddz;
    float *dgamma, *dbeta; int M, W, act, accumulate; float* scratch; hipStream_t st;
    template <int G, int NV, bool VEC>
    int operator()() const
    {
        constexpr int RPW = 64 / G;
        const long long groups = ((long long)M + RPW - 1) / RPW;                      // passes of one wave over the rows
        const long long want = groups < kLnMaxPartials ? groups : kLnMaxPartials;
        const long long rpw = (groups + want - 1) / want * RPW;                       // rows per wave: whole passes
        const int n_waves = (int)(((long long)M + rpw - 1) / rpw);                    // <= want <= min(M, kLnMaxPartials)
        hipLaunchKernelGGL((k_layernorm_bwd<G, NV, VEC>), dim3((unsigned)((n_waves + 3) / 4)), dim3(kBlock), 0, st, dy, lddy, y, ldy, xhat,
                           ldx, rstd, gamma, dz, lddz, scratch, M, W, act, (int)rpw, n_waves);
        VF_HIP(hipGetLastError());
        fold_partials_launch(scratch, n_waves, 2 * W, W, W, dgamma, dbeta, accumulate, st);
        VF_HIP(hipGetLastError());
        return VF_OK;
    }
};

}  // namespace
}  // namespace vf

extern "C" {

int vf_layernorm_fwd(const float* z, int32_t ldz, const float* gamma, const float* beta, float eps, float* y, int32_t ldy, float* xhat,
                     int32_t ldx, float* rstd, int32_t M, int32_t W, int32_t act, vf_stream_t stream)
{
    using namespace vf;
    if (!z || !gamma || !beta || !y || !xhat || !rstd || bad_ln_dims(M, W) || ldz < W || ldy < W || ldx < W || !(eps >= 0.0f))
        return fail(VF_EINVAL, "vf_layernorm_fwd: bad argument (1 <= W <= %d, leading dimensions >= W)", kLnMaxWidth);
    if (bad_ln_act(act)) return fail(VF_EINVAL, "vf_layernorm_fwd: activation kind %d", act);
    const bool aligned = W % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && ldx % 4 == 0 && aligned16(z) && aligned16(y) && aligned16(xhat);
    return ln_dispatch(ln_shape(W, aligned), LnFwd{z, ldz, gamma, beta, eps, y, ldy, xhat, ldx, rstd, M, W, act, as_stream(stream)});
}

int64_t vf_layernorm_bwd_scratch_floats(int32_t M, int32_t W)
{
    if (M <= 0 || W <= 0) return 0;
    return (int64_t)(M < vf::kLnMaxPartials ? M : vf::kLnMaxPartials) * 2 * W;
}

int vf_layernorm_bwd(const float* dy, int32_t lddy, const float* y, int32_t ldy, const float* xhat, int32_t ldx, const float* rstd,
                     const float* gamma, float* dz, int32_t lddz, float* dgamma, float* dbeta, int32_t M, int32_t W, int32_t act,
                     int32_t accumulate, float* scratch, vf_stream_t stream)
{
    using namespace vf;
    if (!dy || !xhat || !rstd || !gamma || !dz || !dgamma || !dbeta || !scratch || bad_ln_dims(M, W) || lddy < W || ldx < W || lddz < W)
        return fail(VF_EINVAL, "vf_layernorm_bwd: bad argument (1 <= W <= %d, leading dimensions >= W)", kLnMaxWidth);
    if (bad_ln_act(act) || (act != VF_ACTIVATION_NONE && (!y || ldy < W)))
        return fail(VF_EINVAL, "vf_layernorm_bwd: activation kind %d needs the saved output y (ldy >= W)", act);
    const bool aligned = W % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddz % 4 == 0 && aligned16(dy) && aligned16(xhat) && aligned16(dz) &&
                         (act == VF_ACTIVATION_NONE || (ldy % 4 == 0 && aligned16(y)));
    return ln_dispatch(ln_shape(W, aligned), LnBwd{dy, lddy, y, ldy, xhat, ldx, rstd, gamma, dz, lddz, dgamma, dbeta, M, W, act,
                                                   accumulate ? 1 : 0, scratch, as_stream(stream)});
}

}  // extern "C"
