// Host checks of visfly_amd/csrc/vf_step_consts.hpp (tests/test_step_consts_host.py), built with the system compiler:
//   step_consts_host pack FILE   FILE = raw vf_dyn_cfg structs back to back; prints, per struct, the 32 words of its packed block in hex
//   step_consts_host hit         hit_threshold: `y < T` against `sqrtf(y) < r`; prints "checked K bad B"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "vf_step_consts.hpp"

static float as_f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t as_u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static int pack(const char* path)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    vf_dyn_cfg c;
    while (std::fread(&c, sizeof c, 1, f) == 1) {
        vf::vf_step_consts k;
        std::memset(&k, 0xAB, sizeof k);
        vf::pack_step_consts(c, &k);
        uint32_t w[32];
        std::memcpy(w, &k, sizeof w);
        for (int i = 0; i < 32; ++i) std::printf("%08x%c", w[i], i == 31 ? '\n' : ' ');
    }
    std::fclose(f);
    return 0;
}

static int hit()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float radii[] = {0.1f, 0.0f, -0.0f, -1.0f, 1e-40f, as_f(1u), inf, nan, 1.0f, 0.3f, 1e-20f, 1e19f, 3.4028235e38f, 1.17549435e-38f};
    long long checked = 0, bad = 0;
    for (float r : radii) {
        const float T = vf::hit_threshold(r);
        std::vector<float> ys = {0.0f, as_f(1u), as_f(0x007FFFFFu), inf, nan, as_f(0x7FC00001u), 1.17549435e-38f, 3.4028235e38f};
        if (T == T) {   // y is a sum of squares: +0, positive or NaN, never negative -- the neighbourhood of T stops at +0
            const int64_t t = as_u(T);
            for (int64_t d = -64; d <= 64; ++d)
                if (t + d >= 0 && t + d <= 0x7F800000) ys.push_back(as_f((uint32_t)(t + d)));
        }
        for (float y : ys) {
            const bool want = std::sqrt(y) < r, got = y < T;
            ++checked;
            if (want != got) {
                if (!bad) std::printf("first mismatch: r = %a (0x%08x)  T = 0x%08x  y = 0x%08x  sqrtf(y) < r: %d  y < T: %d\n", r, as_u(r), as_u(T),
                                      as_u(y), (int)want, (int)got);
                ++bad;
            }
        }
        // the table of edge values
        if (r <= 0.0f && as_u(T) != 0u) { std::printf("r = %a: T must be +0\n", r); ++bad; }
        if (r == inf && T != inf) { std::printf("r = inf: T must be +inf\n"); ++bad; }
        if (r != r && T == T) { std::printf("r NaN: T must be NaN\n"); ++bad; }
        // T is the SMALLEST float whose root reaches r
        if (r > 0.0f && r < inf) {
            if (!(std::sqrt(T) >= r)) { std::printf("r = %a: sqrtf(T) < r\n", r); ++bad; }
            if (as_u(T) > 0u && !(std::sqrt(as_f(as_u(T) - 1u)) < r)) { std::printf("r = %a: T is not the smallest\n", r); ++bad; }
        }
    }
    std::printf("checked %lld bad %lld\n", checked, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "pack")) return pack(argv[2]);
    if (argc == 2 && !std::strcmp(argv[1], "hit")) return hit();
    return 2;
}
