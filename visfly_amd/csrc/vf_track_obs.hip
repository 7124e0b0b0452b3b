// vf_track_obs.hip -- TrackEnv's observation rows (envs/TrackingEnv.py:81-98) and their adjoint, one launch each.
//
// "state" = [(waypoint j - p) / max_sense_radius for j < n_points, q, v / 10, w / 10] = 3 n_points + 10 columns (40 for the reference's
// ten waypoints).  The waypoints are constants of the env (the reference forms them once, in its constructor), so the rows are a
// per-agent map of the step kernel's raw state rows: one launch behind it, like vf_race_obs.  The arithmetic is race2_obs's
// (vf_env_device.hpp): IEEE divisions, no contraction.
//
// Both kernels stream.  The forward writes 3x what it reads (160 B against 52 B per agent for ten waypoints), so the launch is indexed over
// the OUTPUT: one lane per 16-byte chunk of the flat (N, W) array, a wave's stores are 1 KiB of consecutive addresses.  A chunk may
// straddle two rows when W is no multiple of 4; the last chunk of the array may be short and is then stored word by word.  The raw
// rows are re-read by the lanes that share them (every p[c] by n_points lanes, from L1 / L2).  The waypoint table travels by value in the
// kernel arguments (at most 48 floats): no device buffer, no LDS.  With the stores contiguous the column differs from lane to lane, so a
// lane reads its table entry from the kernel-argument segment by its own column (a cached 4-byte vector load; the scalar loads fetch the
// pointers, the radius and N); no scratch.
#include "vf_common.hpp"

namespace vf {

constexpr int kTrackMaxPoints = 16;
struct TrackPoints {
    float w[3 * kTrackMaxPoints];
};

// column `col` of the row formed from the raw state row r
template <int P>
__device__ __forceinline__ float track_col(const TrackPoints& wp, const float* __restrict__ r, int col, float radius)
{
    if (col < 3 * P) {
        const int c = col % 3;
        return (wp.w[col] - r[c]) / radius;
    }
    const int k = col - 3 * P;                     // 0..3: q, 4..9: v, w
    const float x = r[3 + k];
    return k < 4 ? x : x / 10.0f;
}

template <int P>
__global__ __launch_bounds__(kBlock) void k_track_obs(const float* __restrict__ raw0, float* __restrict__ out0, const float* __restrict__ raw1,
                                                      float* __restrict__ out1, const TrackPoints wp, float radius, int N)
{
    constexpr int W = 3 * P + 10;
    // blockIdx.y: the live pair, or the terminal one
    const float* __restrict__ raw = blockIdx.y ? raw1 : raw0;
    float* __restrict__ out = blockIdx.y ? out1 : out0;
    const size_t total = (size_t)N * W;
    const size_t e0 = 4 * ((size_t)blockIdx.x * kBlock + threadIdx.x);
    if (e0 >= total) return;
    size_t row = e0 / W;
    int col = (int)(e0 - row * W);
    const int n = total - e0 < 4 ? (int)(total - e0) : 4;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < n) v[k] = track_col<P>(wp, raw + 13 * row, col, radius);
        if (++col == W) {
            col = 0;
            ++row;
        }
    }
    if (n == 4) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < n; ++k) out[e0 + k] = v[k];
    }
}

// one lane per element of the (N, 13) result
__global__ __launch_bounds__(kBlock) void k_track_obs_bwd(const float* __restrict__ d_rows, float* __restrict__ d_raw, int P, float radius, int N)
{
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (size_t)N * 13) return;
    const size_t row = e / 13;
    const int c = (int)(e - row * 13);
    const float* __restrict__ d = d_rows + row * (size_t)(3 * P + 10);
    float g;
    if (c < 3) {
        float acc = d[c] / radius;                                   // divide each term, then add in the order j = 0, 1, ..
        for (int j = 1; j < P; ++j) acc = acc + d[3 * j + c] / radius;
        g = -acc;
    } else {
        const float x = d[3 * P + c - 3];
        g = c < 7 ? x : x / 10.0f;
    }
    d_raw[e] = g;
}

template <int P>
static void launch_track_obs(dim3 grid, hipStream_t s, const float* raw, float* out, const float* raw1, float* out1, const TrackPoints& wp,
                             float radius, int N)
{
    hipLaunchKernelGGL(k_track_obs<P>, grid, dim3(kBlock), 0, s, raw, out, raw1, out1, wp, radius, N);
}

}  // namespace vf

extern "C" int vf_track_obs(const float* raw, float* rows_out, const float* raw_term, float* term_out, const float* waypoints_host,
                            int32_t n_points, float sense_radius, int32_t N, vf_stream_t stream)
{
    using namespace vf;
    if (!raw || !rows_out || !waypoints_host || N < 1) return fail(VF_EINVAL, "vf_track_obs: null argument or N < 1");
    if ((raw_term == nullptr) != (term_out == nullptr)) return fail(VF_EINVAL, "vf_track_obs: raw_term and term_out come as a pair");
    if (n_points < 1 || n_points > kTrackMaxPoints || !(sense_radius > 0.0f))
        return fail(VF_EINVAL, "vf_track_obs: n_points in [1, %d], sense_radius > 0", kTrackMaxPoints);
    if ((reinterpret_cast<uintptr_t>(rows_out) | reinterpret_cast<uintptr_t>(term_out)) & 15)
        return fail(VF_EINVAL, "vf_track_obs: the output rows are written in 16-byte stores: rows_out / term_out must be 16-byte aligned");
    TrackPoints wp{};
    for (int k = 0; k < 3 * n_points; ++k) wp.w[k] = waypoints_host[k];
    const size_t chunks = ((size_t)N * (3 * n_points + 10) + 3) / 4;
    const dim3 grid((unsigned)((chunks + kBlock - 1) / kBlock), term_out ? 2 : 1);
    hipStream_t s = as_stream(stream);
    switch (n_points) {
#define VF_TRACK_CASE(P) case P: launch_track_obs<P>(grid, s, raw, rows_out, raw_term, term_out, wp, sense_radius, N); break;
        VF_TRACK_CASE(1) VF_TRACK_CASE(2) VF_TRACK_CASE(3) VF_TRACK_CASE(4) VF_TRACK_CASE(5) VF_TRACK_CASE(6) VF_TRACK_CASE(7) VF_TRACK_CASE(8)
        VF_TRACK_CASE(9) VF_TRACK_CASE(10) VF_TRACK_CASE(11) VF_TRACK_CASE(12) VF_TRACK_CASE(13) VF_TRACK_CASE(14) VF_TRACK_CASE(15)
        VF_TRACK_CASE(16)
#undef VF_TRACK_CASE
    }
    VF_HIP(hipGetLastError());
    return VF_OK;
}

extern "C" int vf_track_obs_bwd(const float* d_rows, float* d_raw_out, int32_t n_points, float sense_radius, int32_t N, vf_stream_t stream)
{
    using namespace vf;
    if (!d_rows || !d_raw_out || N < 1) return fail(VF_EINVAL, "vf_track_obs_bwd: null argument or N < 1");
    if (n_points < 1 || n_points > kTrackMaxPoints || !(sense_radius > 0.0f))
        return fail(VF_EINVAL, "vf_track_obs_bwd: n_points in [1, %d], sense_radius > 0", kTrackMaxPoints);
    const size_t elems = (size_t)N * 13;
    hipLaunchKernelGGL(k_track_obs_bwd, dim3((unsigned)((elems + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), d_rows, d_raw_out,
                       (int)n_points, sense_radius, (int)N);
    VF_HIP(hipGetLastError());
    return VF_OK;
}
