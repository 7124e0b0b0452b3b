// sqrt_p2 (csrc/vf_pair_algebra.hpp) against the sqrtf of this translation unit, bit for bit, NaNs included.
//   hipcc <the flags of visfly_amd/_build.py for vf_env.hip, without -shared -fPIC> -I visfly_amd/csrc tools/sqrt_pair_probe.hip -o tools/sqrt_pair_probe
// Inputs: every element of the set S of tools/div_pair_probe.hip (+-0, +-inf, a NaN, the denormal extremes, +-(exponents -126 .. 127) x
// mantissas {0, 1, 0x400000, 0x7FFFFF}: 2 041 values, the negative ones included -- their root is a NaN) in each of the four places of
// sqrt_p2, the other three places taken by other elements of S (shifted indices), so that one root takes the scaled path while its
// neighbours do not; then 2^22 random bit patterns per place.
// Prints "mismatches K of M" (M = roots compared) and the first mismatch; exit status 1 if K != 0.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "vf_pair_algebra.hpp"

struct Result {
    unsigned long long mismatches, first;
};
struct First {
    unsigned x, got, want, place;
};

__device__ __forceinline__ float as_f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ unsigned as_u(float f) { return __builtin_bit_cast(unsigned, f); }

// the reference: this translation unit's sqrtf, in a function of its own
__device__ __noinline__ float ref_sqrt(float x) { return sqrtf(x); }

__device__ void check4(unsigned long long id, const unsigned* x, Result* res, First* first)
{
    const vf::vf_f2 a = {as_f(x[0]), as_f(x[1])}, b = {as_f(x[2]), as_f(x[3])};
    vf::vf_f2 oa, ob;
    vf::sqrt_p2(a, b, oa, ob);
    const float got[4] = {oa[0], oa[1], ob[0], ob[1]};
    unsigned bad = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const unsigned want = as_u(ref_sqrt(as_f(x[h])));
        if (as_u(got[h]) != want) {
            ++bad;
            const unsigned long long key = id * 4 + h;
            if (atomicMin(&res->first, key) > key) {      // diagnostic only (two writers may interleave): the verdict is the count
                first->x = x[h];
                first->got = as_u(got[h]);
                first->want = want;
                first->place = h;
            }
        }
    }
    if (bad) atomicAdd(&res->mismatches, (unsigned long long)bad);
}

__global__ void k_set(const unsigned* S, unsigned n, Result* res, First* first)
{
    // element t in place `rot`, the other places from shifted indices
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < 4 * n; t += gridDim.x * blockDim.x) {
        const unsigned i = t % n, rot = t / n;
        const unsigned idx[4] = {i, (i + n / 2 + 3) % n, (i + n / 3 + 1) % n, (i + 7) % n};
        unsigned x[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) x[(h + rot) & 3] = S[idx[h]];
        check4(t, x, res, first);
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
        const unsigned long long p = mix(2 * t), q = mix(2 * t + 1);
        const unsigned x[4] = {(unsigned)p, (unsigned)(p >> 32), (unsigned)q, (unsigned)(q >> 32)};
        check4(base_id + t, x, res, first);
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
    const unsigned long long n_random = 1ull << 22;

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
    k_set<<<32, 256>>>(dS, n, dres, dfirst);
    CHECK(hipGetLastError());
    k_random<<<2048, 256>>>(n_random, 4ull * n, dres, dfirst);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&res, dres, sizeof res, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&first, dfirst, sizeof first, hipMemcpyDeviceToHost));
    const unsigned long long compared = (4ull * n + n_random) * 4;
    std::printf("set %u elements in 4 places, %llu random quadruples\n", n, n_random);
    std::printf("mismatches %llu of %llu\n", res.mismatches, compared);
    if (res.mismatches)
        std::printf("first mismatch: place %u  x = 0x%08X  sqrt_p2 = 0x%08X  sqrtf = 0x%08X\n", first.place, first.x, first.got, first.want);
    return res.mismatches ? 1 : 0;
}
