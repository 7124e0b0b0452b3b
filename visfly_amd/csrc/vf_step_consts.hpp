// The packed step-constant block of a handle: the words of vf_dyn_cfg that the sub-step loop of the straight-line step kernel
// (k_env_step<STRAIGHT>, vf_env.hip) holds in VGPR pairs, copied -- no arithmetic folded -- into the order and pairing in which the
// kernel consumes them, so that a few uniform-address 16-byte vector loads put them straight into those pairs: no scalar load, no
// wait and no v_mov per word.  Built on the host wherever the device copy of vf_dyn_cfg is written (upload_dyn_dev, vf_handles.hpp)
// and device-resident right behind it: the kernels keep their `const vf_dyn_cfg*` argument and find the block at kStepConstsOffset.
// The C ABI (include/visfly_amd.h) is untouched.
//
// Also here: the squared-distance threshold that replaces the square root of the hover kinds' collision test (hit_threshold).
//
// Self-contained, no HIP header: tests/step_consts_host.cpp builds it with the system compiler.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "visfly_amd.h"

namespace vf {

// 8 x 16 bytes; word for word what interval_mats() (vf_dyn_device.hpp) arranges from the scalar copy:
struct vf_step_consts {
    float Bcol[4][4];   // Bcol[k] = (B[0][k], B[1][k], B[2][k], B[3][k]): Mat4P::c01[k], c23[k] (B is row-major in vf_dyn_cfg)
    float J12[3][2];    // J12[k] = (J[1][k], J[2][k]): Mat3P::c12[k] of J
    float Jinv12[3][2]; // the same of Jinv
    float K0[2], K1[2]; // RotorK: (c_motor, tm0), (tm1, tm2)
};
static_assert(sizeof(vf_step_consts) == 128, "eight 16-byte loads");

// device block of a dynamics handle: the public vf_dyn_cfg, then -- on a 64-byte line of its own -- the packed words
constexpr size_t kStepConstsOffset = (sizeof(vf_dyn_cfg) + 63) / 64 * 64;
struct vf_dyn_dev {
    vf_dyn_cfg cfg;
    alignas(64) vf_step_consts k;
};
static_assert(offsetof(vf_dyn_dev, k) == kStepConstsOffset, "the kernels address the block by this offset");

inline void pack_step_consts(const vf_dyn_cfg& c, vf_step_consts* out)
{
    for (int k = 0; k < 4; ++k)
        for (int r = 0; r < 4; ++r) out->Bcol[k][r] = c.B[4 * r + k];
    for (int k = 0; k < 3; ++k) {
        out->J12[k][0] = c.J[3 + k];
        out->J12[k][1] = c.J[6 + k];
        out->Jinv12[k][0] = c.Jinv[3 + k];
        out->Jinv12[k][1] = c.Jinv[6 + k];
    }
    out->K0[0] = c.c_motor; out->K0[1] = c.tm0;
    out->K1[0] = c.tm1; out->K1[1] = c.tm2;
}

// The hover kinds' collision test is `dis < r` with dis = sqrtf(y), y the FMA chain of the squared distance to the closest wall, and
// nothing else reads dis.  A correctly rounded sqrtf is monotone (non-decreasing), so { y : sqrtf(y) < r } is a down-set of the ordered
// non-negative floats, and sqrtf(y) < r  <=>  y < T with T the smallest float whose sqrtf is >= r.  (y is +0 or positive here -- a
// sum of squares -- or NaN; -0 cannot arise from x * x and the FMAs that add squares to it.)
//   r <= 0 (or -0): sqrtf(y) >= 0 >= r for every y, no hit: T = +0, y < +0 is false for every y >= 0.
//   r = +inf: sqrtf(y) < inf for every finite y, false for y = +inf: T = +inf.
//   r NaN: every compare is false: T = NaN.
//   y NaN: sqrtf(y) is NaN, both compares are false.
// Found by bisection over the bit patterns of the non-negative floats (monotone in the value) with the host's correctly rounded sqrtf.
inline float hit_threshold(float r)
{
    if (r != r) return r;
    if (!(r > 0.0f)) return 0.0f;
    if (std::isinf(r)) return r;
    uint32_t lo = 0u, hi = 0x7f800000u;          // invariant: sqrtf(float(hi)) >= r; the answer lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float y;
        std::memcpy(&y, &mid, 4);
        if (std::sqrt(y) >= r) hi = mid;
        else lo = mid + 1;
    }
    float T;
    std::memcpy(&T, &hi, 4);
    return T;
}

}  // namespace vf
