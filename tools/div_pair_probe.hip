// div_p (csrc/vf_pair_algebra.hpp) against the `/` of this translation unit, bit for bit, NaNs included.
//   hipcc <the flags of visfly_amd/_build.py for vf_env.hip, without -shared -fPIC> -I visfly_amd/csrc tools/div_pair_probe.hip -o tools/div_pair_probe
// Inputs: every ordered pair (numerator, denominator) from a set S in the low half, with another pair of S (shifted indices) in the high
// half, so that one half takes a scaling path while the other does not; then 2^22 random bit patterns per operand.  Both forms of div_p,
// and the interleaved forms the sub-step loop uses: div_p2 (two pairs by one denominator) and div_p1 (a pair and a scalar by one).
// S = +-0, +-inf, a NaN, the denormal extremes, and +-(exponents -126 .. 127) x mantissas {0, 1, 0x400000, 0x7FFFFF}.
// Prints "mismatches K of M" (M = quotients compared) and the first mismatch; exit status 1 if K != 0.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "vf_pair_algebra.hpp"

struct Result {
    unsigned long long mismatches, first;
};
struct First {
    unsigned a, b, got, want, form, half;
};

__device__ __forceinline__ float as_f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ unsigned as_u(float f) { return __builtin_bit_cast(unsigned, f); }

// the reference: this translation unit's `/`, in a function of its own
__device__ __noinline__ float ref_div(float a, float b) { return a / b; }

__device__ void check(unsigned long long id, unsigned form, vf::vf_f2 a, vf::vf_f2 b, vf::vf_f2 got, Result* res, First* first)
{
    unsigned bad = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned want = as_u(ref_div(a[h], b[h]));
        if (as_u(got[h]) != want) {
            ++bad;
            const unsigned long long key = id * 8 + form * 2 + h;
            if (atomicMin(&res->first, key) > key) {      // diagnostic only (two writers may interleave): the verdict is the count
                first->a = as_u(a[h]);
                first->b = as_u(b[h]);
                first->got = as_u(got[h]);
                first->want = want;
                first->form = form;
                first->half = h;
            }
        }
    }
    if (bad) atomicAdd(&res->mismatches, (unsigned long long)bad);
}

__device__ void both_forms(unsigned long long id, vf::vf_f2 a, vf::vf_f2 b, Result* res, First* first)
{
    check(id, 0, a, b, vf::div_p(a, b), res, first);
    const vf::vf_f2 bb = {b[0], b[0]};
    check(id, 1, a, bb, vf::div_p(a, b[0]), res, first);
    // div_p2: (a, a2) / b[0] with a2 = (b[1], a[0]); div_p1: (a, b[1]) / b[0]
    const vf::vf_f2 a2 = {b[1], a[0]};
    vf::vf_f2 o0, o1, o;
    float ox;
    vf::div_p2(a, a2, b[0], o0, o1);
    check(id, 2, a, bb, o0, res, first);
    check(id, 2, a2, bb, o1, res, first);
    vf::div_p1(a, b[1], b[0], o, ox);
    check(id, 3, a, bb, o, res, first);
    const vf::vf_f2 ax2 = {b[1], b[1]}, ox2 = {ox, ox};
    check(id, 3, ax2, bb, ox2, res, first);      // the scalar quotient, counted once below
}

__global__ void k_pairs(const unsigned* S, unsigned n, Result* res, First* first)
{
    const unsigned long long total = (unsigned long long)n * n;
    for (unsigned long long t = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; t < total;
         t += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned i = (unsigned)(t / n), j = (unsigned)(t % n);
        // the high half: other elements of S, the two indices shifted by different amounts
        const unsigned i2 = (i + n / 2 + 3) % n, j2 = (j + n / 3 + 1) % n;
        const vf::vf_f2 a = {as_f(S[i]), as_f(S[i2])}, b = {as_f(S[j]), as_f(S[j2])};
        both_forms(t, a, b, res, first);
    }
}

__device__ __forceinline__ unsigned long long mix(unsigned long long z)      // splitmix64
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void k_random(unsigned long long count, unsigned long long base_id, Result* res, First* first)
{
    for (unsigned long long t = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; t < count;
         t += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long x = mix(2 * t), y = mix(2 * t + 1);
        const vf::vf_f2 a = {as_f((unsigned)x), as_f((unsigned)(x >> 32))}, b = {as_f((unsigned)y), as_f((unsigned)(y >> 32))};
        both_forms(base_id + t, a, b, res, first);
    }
}

#define CHECK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                         \
            return 2;                                                                   \
        }                                                                               \
    } while (0)

int main()
{
    std::vector<unsigned> S = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u,
                               0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu};
    const unsigned mant[4] = {0u, 1u, 0x400000u, 0x7FFFFFu};
    for (unsigned sign = 0; sign < 2; ++sign)
        for (unsigned e = 1; e <= 254; ++e)           // biased: exponents -126 .. 127
            for (unsigned m : mant) S.push_back((sign << 31) | (e << 23) | m);
    const unsigned n = (unsigned)S.size();
    const unsigned long long n_pairs = (unsigned long long)n * n, n_random = 1ull << 22;

    unsigned* dS;
    Result* dres;
    First* dfirst;
    CHECK(hipMalloc(&dS, n * sizeof(unsigned)));
    CHECK(hipMalloc(&dres, sizeof(Result)));
    CHECK(hipMalloc(&dfirst, sizeof(First)));
    CHECK(hipMemcpy(dS, S.data(), n * sizeof(unsigned), hipMemcpyHostToDevice));
    Result res = {0, ~0ull};
    First first;
    std::memset(&first, 0, sizeof first);
    CHECK(hipMemcpy(dres, &res, sizeof res, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dfirst, &first, sizeof first, hipMemcpyHostToDevice));
    k_pairs<<<2048, 256>>>(dS, n, dres, dfirst);
    CHECK(hipGetLastError());
    k_random<<<2048, 256>>>(n_random, n_pairs, dres, dfirst);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&res, dres, sizeof res, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&first, dfirst, sizeof first, hipMemcpyDeviceToHost));
    const unsigned long long compared = (n_pairs + n_random) * 11;     // per input: 2 + 2 (div_p), 4 (div_p2), 3 (div_p1) quotients
    std::printf("set %u elements, %llu ordered pairs, %llu random\n", n, n_pairs, n_random);
    std::printf("mismatches %llu of %llu\n", res.mismatches, compared);
    if (res.mismatches)
        std::printf("first mismatch: form %s half %u  a = 0x%08X  b = 0x%08X  div_p = 0x%08X  / = 0x%08X\n",
                    (const char*[]){"div_p(pair, pair)", "div_p(pair, scalar)", "div_p2", "div_p1"}[first.form], first.half, first.a, first.b, first.got, first.want);
    return res.mismatches ? 1 : 0;
}
