// Host check of the register-pair algebra (visfly_amd/csrc/vf_pair_algebra.hpp): the plain C++ bodies of qmul_p / mat3_p / mat4_p / rotors_p
// against the scalar qmul / mat3 / mat4 / rotor recurrence, bit for bit (a NaN need only be a NaN).  Built and run by tests/test_pair_algebra_host.py.
//
// Inputs: 2^20 random bit patterns per operation, and the special values {+-0, +-denormal, +-1, +-large, +-inf} in every combination:
//   qmul (3 forms)  all 10^8 assignments of the 8 components;
//   mat3            all 10^3 vectors x all 10^3 rows (10^6), the three rows of the matrix being rotations of that row;
//   mat4            all 10^4 vectors x all 10^4 rows (10^8), the four rows being rotations of that row;
//   rotors_p        all 10^6 assignments of a rotor's (speed, set-point) and the four rotor constants, against the scalar recurrence + mat4
// (the rows of a matrix-vector product do not interact, so every row chain sees every combination of its 2 K operands).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <thread>
#include <vector>

#include "vf_pair_algebra.hpp"

using namespace vf;

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }

static const uint32_t kSpecialBits[10] = {0x00000000u, 0x80000000u, 0x00012345u, 0x80012345u, 0x3f800000u,
                                          0xbf800000u, 0x7f0ccccdu, 0xff0ccccdu, 0x7f800000u, 0xff800000u};
static float special(int k) { return from_bits(kSpecialBits[k]); }

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static std::atomic<long long> bad{0}, total{0};
static thread_local long long checked = 0;   // per thread, added to total when the thread is done
static void report(const char* what, const float* in, int n)
{
    if (++bad > 10) return;
    printf("MISMATCH %s:", what);
    for (int k = 0; k < n; ++k) printf(" %08x", bits(in[k]));
    printf("\n");
}

template <bool CA, bool CB>
static void check_qmul(const float* v, const char* what)
{
    const Quat a{v[0], v[1], v[2], v[3]}, b{v[4], v[5], v[6], v[7]};
    const Quat r = qmul(CA ? qconj(a) : a, CB ? qconj(b) : b);
    const Quat p = to_quat(qmul_p<CA, CB>(to_pairs(a), to_pairs(b)));
    ++checked;
    if (!(same(r.w, p.w) && same(r.x, p.x) && same(r.y, p.y) && same(r.z, p.z))) report(what, v, 8);
}

static void check_mat3(const float* A, const float* x)
{
    float o[3], p0;
    vf_f2 p12;
    mat3(A, x[0], x[1], x[2], o);
    mat3_p(mat3_pairs(A), pair_of(from_bits(0x7fc00000u), x[0]), pair_of(x[1], x[2]), p0, p12);   // the low half of x0p is not read
    ++checked;
    if (!(same(o[0], p0) && same(o[1], p12[0]) && same(o[2], p12[1]))) report("mat3", x, 3);
}

static void check_mat4(const float* A, const float* x)
{
    float o[4];
    vf_f2 p01, p23;
    mat4(A, x, o);
    mat4_p(mat4_pairs(A), pair_of(x[0], x[1]), pair_of(x[2], x[3]), p01, p23);
    ++checked;
    if (!(same(o[0], p01[0]) && same(o[1], p01[1]) && same(o[2], p23[0]) && same(o[3], p23[1]))) report("mat4", x, 4);
}

// rotors_p against the scalar rotor recurrence + mat4 (motor_substep's scalar form, vf_dyn_device.hpp)
static void check_rotors(const float* v)
{
    const float *B = v, *wd = v + 16, *wm0 = v + 20, cm = v[24], tm0 = v[25], tm1 = v[26], tm2 = v[27];
    float wm[4], T[4], ft[4];
    for (int k = 0; k < 4; ++k) {
        wm[k] = cm * wm0[k] + wd[k];
        const float wp = wm[k] + 0.0f;
        T[k] = (tm0 * (wp * wp) + tm1 * wm[k]) + tm2;
    }
    mat4(B, T, ft);
    const vf_f2 wdp[2] = {pair_of(wd[0], wd[1]), pair_of(wd[2], wd[3])};
    vf_f2 wmp[2] = {pair_of(wm0[0], wm0[1]), pair_of(wm0[2], wm0[3])}, Tp[2], ft01, ft23;
    rotors_p(mat4_pairs(B), pair_of(cm, tm0), pair_of(tm1, tm2), wdp, wmp, Tp, ft01, ft23);
    ++checked;
    bool ok = same(ft[0], ft01[0]) && same(ft[1], ft01[1]) && same(ft[2], ft23[0]) && same(ft[3], ft23[1]);
    for (int k = 0; k < 4; ++k) ok = ok && same(wm[k], wmp[k >> 1][k & 1]) && same(T[k], Tp[k >> 1][k & 1]);
    if (!ok) report("rotors", v + 16, 12);
}

int main()
{
    float v[28];
    // random bit patterns
    for (int it = 0; it < (1 << 20); ++it) {
        for (int k = 0; k < 28; ++k) v[k] = from_bits(rnd());
        check_qmul<false, false>(v, "qmul");
        check_qmul<true, false>(v, "qmul conj(a)");
        check_qmul<false, true>(v, "qmul conj(b)");
        check_mat3(v, v + 9);
        check_mat4(v, v + 16);
        check_rotors(v);
    }
    // special values, every combination (the 10^8 assignments are split over a few threads)
    const int nt = (int)std::thread::hardware_concurrency() >= 8 ? 8 : ((int)std::thread::hardware_concurrency() >= 2 ? 2 : 1);
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([t, nt] {
            float v[8];
            for (int n = t; n < 100000000; n += nt) {
                int m = n;
                for (int k = 0; k < 8; ++k, m /= 10) v[k] = special(m % 10);
                check_qmul<false, false>(v, "qmul");
                check_qmul<true, false>(v, "qmul conj(a)");
                check_qmul<false, true>(v, "qmul conj(b)");
                // the same eight values as a row (v[0..3]) and a vector (v[4..7]) of mat4
                float A[16];
                for (int i = 0; i < 4; ++i)
                    for (int k = 0; k < 4; ++k) A[4 * i + k] = v[(k + i) & 3];
                check_mat4(A, v + 4);
            }
            total += checked;
        });
    for (auto& th : pool) th.join();
    for (int n = 0; n < 1000000; ++n) {
        int m = n;
        for (int k = 0; k < 6; ++k, m /= 10) v[k] = special(m % 10);
        float A[9];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) A[3 * i + k] = v[(k + i) % 3];
        check_mat3(A, v + 3);
    }
    for (int n = 0; n < 1000000; ++n) {   // rotors: (wm, wd) of a rotor x (c_motor, tm0, tm1, tm2), the rotors and B's rows rotated
        int m = n;
        float sv[6];
        for (int k = 0; k < 6; ++k, m /= 10) sv[k] = special(m % 10);
        for (int k = 0; k < 4; ++k) { v[16 + k] = sv[k & 1 ? 1 : 0]; v[20 + k] = sv[k & 1 ? 0 : 1]; v[24 + k] = sv[2 + k]; }
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) v[4 * i + k] = sv[(k + i) % 6];
        check_rotors(v);
    }
    total += checked;
    printf("checked %lld mismatches %lld\n", total.load(), bad.load());
    return bad ? 1 : 0;
}
