// Quaternion and small-matrix algebra of the sub-step loop, in scalar form and on register PAIRS (gfx950).
//
// A lone wave issues one VALU instruction per ~4 cycles whatever it is, and a v_pk_*_f32 instruction does two IEEE fp32 operations in
// that slot (profiles/r02_valu_cost_probe.txt), so the sub-step loop pays per instruction, not per operation.  The pair layout keeps a
// quaternion as two 64-bit register pairs (w, x) and (y, z); the Hamilton product on it is ONE asm statement of 8 packed multiplies and
// 6 packed adds whose swaps and sign flips ride on op_sel / op_sel_hi / neg_lo / neg_hi.  The constant matrices are applied two rows at a
// time from column pairs (A[r][k], A[r+1][k]) arranged once per control interval.  The IEEE divisions keep hipcc's own sequence with the
// six plain operations of two quotients on a pair (div_p, div_p2, div_p1 at the end of this file).
//
// Same products, same additions, same order as the scalar forms (utils/maths.py:168-174; the k-ordered FMA chains of the reference's
// sgemm).  The only rewrites are (-a) * b for -(a * b) and x + (-y) for x - y, both exact in IEEE arithmetic, signed zeros included;
// a pure-vector operand (0, v) keeps its zero and every term.  Each pair operation has a plain C++ body of the same operation order for
// the host (tests/test_pair_algebra_host.py compiles both forms with the system compiler and compares them bit for bit).
//
// Self-contained: no HIP header needed (compiler builtins only on the device side), so that the host test can include it.  Compile with
// -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define VF_PA_FN __device__ __forceinline__
#else
#define VF_PA_FN static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vf {

struct Quat {
    float w, x, y, z;
};

typedef float vf_f2 __attribute__((vector_size(8)));

// (w, x) and (y, z)
struct QuatP {
    vf_f2 wx, yz;
};

VF_PA_FN vf_f2 pair_of(float lo, float hi)
{
    vf_f2 r = {lo, hi};
    return r;
}
VF_PA_FN QuatP to_pairs(const Quat& a) { return QuatP{pair_of(a.w, a.x), pair_of(a.y, a.z)}; }
VF_PA_FN Quat to_quat(const QuatP& a) { return Quat{a.wx[0], a.wx[1], a.yz[0], a.yz[1]}; }

// Hamilton product; term order and rounding of utils/maths.py:168-174
VF_PA_FN Quat qmul(const Quat& a, const Quat& b)
{
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    return r;
}

VF_PA_FN Quat qconj(const Quat& a) { return Quat{a.w, -a.x, -a.y, -a.z}; }

// (3x3) @ x as the k-ordered FMA chain of the reference's sgemm
VF_PA_FN void mat3(const float* __restrict__ A, float x0, float x1, float x2, float* o)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float acc = A[3 * i] * x0;
        acc = __builtin_fmaf(A[3 * i + 1], x1, acc);
        acc = __builtin_fmaf(A[3 * i + 2], x2, acc);
        o[i] = acc;
    }
}

VF_PA_FN void mat4(const float* __restrict__ A, const float* x, float* o)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float acc = A[4 * i] * x[0];
        acc = __builtin_fmaf(A[4 * i + 1], x[1], acc);
        acc = __builtin_fmaf(A[4 * i + 2], x[2], acc);
        acc = __builtin_fmaf(A[4 * i + 3], x[3], acc);
        o[i] = acc;
    }
}

// ---- the pair forms ------------------------------------------------------------------------------------------------------------------
// qmul_p<CA, CB>(a, b) = qmul(CA ? qconj(a) : a, CB ? qconj(b) : b): the conjugate's sign flips are source modifiers of the multiplies
// (the scalar form flips the sign bit first and multiplies then: the same product).  At most one of CA, CB.
//
// The eight packed multiplies (src0 = a pair of a, src1 = a pair of b; [lo,lo]*[lo,hi] and [hi,hi]*[hi,lo] selections):
//   t0 = (aw bw, aw bx)  t1 = (ax bx, ax bw)  t2 = (ay by, ay bz)  t3 = (az bz, az by)        -> (r.w, r.x) = ((t0 -+ t1) -+ t2) -- t3
//   u0 = (aw by, aw bz)  u1 = (ax bz, ax by)  u2 = (ay bw, ay bx)  u3 = (az bx, az bw)        -> (r.y, r.z) = ((u0 -+ u1) +- u2) ++ u3
#if defined(__HIP_DEVICE_COMPILE__)
#define VF_PA_LL " op_sel:[0,0] op_sel_hi:[0,1]"   // (s0.lo * s1.lo, s0.lo * s1.hi)
#define VF_PA_HH " op_sel:[1,1] op_sel_hi:[1,0]"   // (s0.hi * s1.hi, s0.hi * s1.lo)
// N0 .. N7: the neg_lo / neg_hi text of the multiplies t0, u0, t1, u1, t2, u2, t3, u3
#define VF_PA_QMUL(N0, N1, N2, N3, N4, N5, N6, N7)                                                                                  \
    "v_pk_mul_f32 %0, %8, %10" VF_PA_LL N0 "\n\t"                                                                                  \
    "v_pk_mul_f32 %1, %8, %11" VF_PA_LL N1 "\n\t"                                                                                  \
    "v_pk_mul_f32 %2, %8, %10" VF_PA_HH N2 "\n\t"                                                                                  \
    "v_pk_mul_f32 %3, %8, %11" VF_PA_HH N3 "\n\t"                                                                                  \
    "v_pk_mul_f32 %4, %9, %11" VF_PA_LL N4 "\n\t"                                                                                  \
    "v_pk_mul_f32 %5, %9, %10" VF_PA_LL N5 "\n\t"                                                                                  \
    "v_pk_mul_f32 %6, %9, %11" VF_PA_HH N6 "\n\t"                                                                                  \
    "v_pk_mul_f32 %7, %9, %10" VF_PA_HH N7 "\n\t"                                                                                  \
    "v_pk_add_f32 %0, %0, %2 neg_lo:[0,1]\n\t"                                                                                     \
    "v_pk_add_f32 %1, %1, %3 neg_lo:[0,1]\n\t"                                                                                     \
    "v_pk_add_f32 %0, %0, %4 neg_lo:[0,1]\n\t"                                                                                     \
    "v_pk_add_f32 %1, %1, %5 neg_hi:[0,1]\n\t"                                                                                     \
    "v_pk_add_f32 %0, %0, %6 neg_lo:[0,1] neg_hi:[0,1]\n\t"                                                                        \
    "v_pk_add_f32 %1, %1, %7"
#define VF_PA_NA " neg_lo:[1,0] neg_hi:[1,0]"    // src0 negated in both halves
#define VF_PA_NB " neg_lo:[0,1] neg_hi:[0,1]"    // src1 negated in both halves
#define VF_PA_NBL " neg_lo:[0,1]"                // src1 negated where the low result reads it
#define VF_PA_NBH " neg_hi:[0,1]"                // ... the high result
#endif

template <bool CA, bool CB>
VF_PA_FN QuatP qmul_p(const QuatP& a, const QuatP& b)
{
    static_assert(!(CA && CB), "at most one conjugated operand");
    QuatP r;
#if defined(__HIP_DEVICE_COMPILE__)
    vf_f2 t1, u1, t2, u2, t3, u3;
#define VF_PA_OPERANDS : "=&v"(r.wx), "=&v"(r.yz), "=&v"(t1), "=&v"(u1), "=&v"(t2), "=&v"(u2), "=&v"(t3), "=&v"(u3) \
                       : "v"(a.wx), "v"(a.yz), "v"(b.wx), "v"(b.yz)
    if constexpr (CA)         // a = (aw, -ax, -ay, -az): every multiply that reads ax, ay or az
        asm(VF_PA_QMUL("", "", VF_PA_NA, VF_PA_NA, VF_PA_NA, VF_PA_NA, VF_PA_NA, VF_PA_NA) VF_PA_OPERANDS);
    else if constexpr (CB)    // b = (bw, -bx, -by, -bz): the halves that read bx, by or bz
        asm(VF_PA_QMUL(VF_PA_NBH, VF_PA_NB, VF_PA_NBL, VF_PA_NB, VF_PA_NB, VF_PA_NBH, VF_PA_NB, VF_PA_NBL) VF_PA_OPERANDS);
    else
        asm(VF_PA_QMUL("", "", "", "", "", "", "", "") VF_PA_OPERANDS);
#undef VF_PA_OPERANDS
#else
    const float aw = a.wx[0], ax = CA ? -a.wx[1] : a.wx[1], ay = CA ? -a.yz[0] : a.yz[0], az = CA ? -a.yz[1] : a.yz[1];
    const float bw = b.wx[0], bx = CB ? -b.wx[1] : b.wx[1], by = CB ? -b.yz[0] : b.yz[0], bz = CB ? -b.yz[1] : b.yz[1];
    const vf_f2 t0 = {aw * bw, aw * bx}, u0 = {aw * by, aw * bz};
    const vf_f2 t1 = {ax * bx, ax * bw}, u1 = {ax * bz, ax * by};
    const vf_f2 t2 = {ay * by, ay * bz}, u2 = {ay * bw, ay * bx};
    const vf_f2 t3 = {az * bz, az * by}, u3 = {az * bx, az * bw};
    r.wx = pair_of(((t0[0] + -t1[0]) + -t2[0]) + -t3[0], ((t0[1] + t1[1]) + t2[1]) + -t3[1]);
    r.yz = pair_of(((u0[0] + -u1[0]) + u2[0]) + u3[0], ((u0[1] + u1[1]) + -u2[1]) + u3[1]);
#endif
    return r;
}

// column pairs of a row-major 4x4 matrix: c01[k] = (A[0][k], A[1][k]), c23[k] = (A[2][k], A[3][k])
struct Mat4P {
    vf_f2 c01[4], c23[4];
};
// ... of a 3x3 one: row 0 by itself, c12[k] = (A[1][k], A[2][k]) -- the layout of a pure-vector quaternion (0, x0), (x1, x2)
struct Mat3P {
    float r0[3];
    vf_f2 c12[3];
};

// A wave-uniform matrix arrives in SGPRs, and left to itself hipcc re-copies every pair into VGPRs where it is used (inside the loop):
// the empty asm makes the VGPR pair the value's only home.
VF_PA_FN void keep_in_vgprs(vf_f2& v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(v));
#else
    (void)v;
#endif
}

VF_PA_FN Mat4P mat4_pairs(const float* __restrict__ A)
{
    Mat4P m;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m.c01[k] = pair_of(A[k], A[4 + k]);
        m.c23[k] = pair_of(A[8 + k], A[12 + k]);
        keep_in_vgprs(m.c01[k]);
        keep_in_vgprs(m.c23[k]);
    }
    return m;
}
VF_PA_FN Mat3P mat3_pairs(const float* __restrict__ A)
{
    Mat3P m;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m.r0[k] = A[k];
        m.c12[k] = pair_of(A[3 + k], A[6 + k]);
        keep_in_vgprs(m.c12[k]);
    }
    return m;
}

// mat4 on rows (0,1) and (2,3): every row keeps its chain fma(A[i][3], x3, fma(A[i][2], x2, fma(A[i][1], x1, A[i][0] * x0)))
VF_PA_FN void mat4_p(const Mat4P& A, const vf_f2 x01, const vf_f2 x23, vf_f2& o01, vf_f2& o23)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_pk_mul_f32 %0, %2, %10 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
        "v_pk_mul_f32 %1, %6, %10 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %0, %3, %10, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %1, %7, %10, %1 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %0, %4, %11, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %1, %8, %11, %1 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %0, %5, %11, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %1, %9, %11, %1 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "=&v"(o01), "=&v"(o23)
        : "v"(A.c01[0]), "v"(A.c01[1]), "v"(A.c01[2]), "v"(A.c01[3]), "v"(A.c23[0]), "v"(A.c23[1]), "v"(A.c23[2]), "v"(A.c23[3]),
          "v"(x01), "v"(x23));
#else
    const float x[4] = {x01[0], x01[1], x23[0], x23[1]};
    vf_f2 a = {A.c01[0][0] * x[0], A.c01[0][1] * x[0]}, b = {A.c23[0][0] * x[0], A.c23[0][1] * x[0]};
    for (int k = 1; k < 4; ++k) {
        a = pair_of(__builtin_fmaf(A.c01[k][0], x[k], a[0]), __builtin_fmaf(A.c01[k][1], x[k], a[1]));
        b = pair_of(__builtin_fmaf(A.c23[k][0], x[k], b[0]), __builtin_fmaf(A.c23[k][1], x[k], b[1]));
    }
    o01 = a;
    o23 = b;
#endif
}

// The rotor recurrence and the allocation of one sub-step in ONE statement (dynamics.py:514,530-534,339), rotors (0,1) and (2,3) as pairs:
//   wm = c_motor * wm + wd;  T = (tm0 * ((wm + 0) * (wm + 0)) + tm1 * wm) + tm2;  (ft01, ft23) = B @ T
// K0 = (c_motor, tm0), K1 = (tm1, tm2).  The two pairs' chains alternate, so that no packed instruction reads the result of the one
// before it (hipcc schedules the chains one after the other and pads every such pair with an s_nop).
VF_PA_FN void rotors_p(const Mat4P& B, const vf_f2 K0, const vf_f2 K1, const vf_f2* wd, vf_f2* wm, vf_f2* T, vf_f2& ft01, vf_f2& ft23)
{
#if defined(__HIP_DEVICE_COMPILE__)
    vf_f2 a0, a1;
    asm("v_pk_mul_f32 %0, %0, %8 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
        "v_pk_mul_f32 %1, %1, %8 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %10\n\t"
        "v_pk_add_f32 %1, %1, %11\n\t"
        "v_pk_add_f32 %4, %0, 0 op_sel_hi:[1,0]\n\t"
        "v_pk_add_f32 %5, %1, 0 op_sel_hi:[1,0]\n\t"
        "v_pk_mul_f32 %4, %4, %4\n\t"
        "v_pk_mul_f32 %5, %5, %5\n\t"
        "v_pk_mul_f32 %4, %8, %4 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %5, %8, %5 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %2, %9, %0 op_sel:[0,0] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %9, %1 op_sel:[0,0] op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %2, %4, %2\n\t"
        "v_pk_add_f32 %3, %5, %3\n\t"
        "v_pk_add_f32 %2, %2, %9 op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %3, %3, %9 op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %6, %12, %2 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
        "v_pk_mul_f32 %7, %16, %2 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %6, %13, %2, %6 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %7, %17, %2, %7 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %6, %14, %3, %6 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %7, %18, %3, %7 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %6, %15, %3, %6 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %7, %19, %3, %7 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "+v"(wm[0]), "+v"(wm[1]), "=&v"(T[0]), "=&v"(T[1]), "=&v"(a0), "=&v"(a1), "=&v"(ft01), "=&v"(ft23)
        : "v"(K0), "v"(K1), "v"(wd[0]), "v"(wd[1]), "v"(B.c01[0]), "v"(B.c01[1]), "v"(B.c01[2]), "v"(B.c01[3]), "v"(B.c23[0]),
          "v"(B.c23[1]), "v"(B.c23[2]), "v"(B.c23[3]));
#else
    for (int h = 0; h < 2; ++h)
        for (int k = 0; k < 2; ++k) {
            wm[h][k] = K0[0] * wm[h][k] + wd[h][k];
            const float wp = wm[h][k] + 0.0f;
            T[h][k] = (K0[1] * (wp * wp) + K1[0] * wm[h][k]) + K1[1];
        }
    mat4_p(B, T[0], T[1], ft01, ft23);
#endif
}

// mat3 on a vector in the pure-vector layout x = (x0p.hi, x12.lo, x12.hi) (x0p.lo is not read): row 0 by itself, rows (1,2) as a pair;
// every row keeps its chain fma(A[i][2], x2, fma(A[i][1], x1, A[i][0] * x0))
// The three packed instructions read each other's result back to back, with no wait state.  Believed to need none, by this reasoning: a
// VALU result read by the next VALU instruction is interlocked by the hardware, and the s_nop hipcc puts between such a pair in its own
// code follows op_sel_hi[0] of the writer (it leaves v_pk_mul ... op_sel_hi:[0,1] -> v_pk_add unpadded), i.e. LLVM's rule for writes of a
// register HALF, whose flag bit coincides with src0's op_sel_hi in this encoding; no v_pk_*_f32 writes a half.  Every fixture is 0 ulp
// with it.  One observation is unexplained and should be ruled out against this before the reasoning is leaned on elsewhere: the
// persistent PPO roll-out on the pair path did not reproduce the per-step loop (profiles/env_pair_algebra.txt, section 7).
VF_PA_FN void mat3_p(const Mat3P& A, const vf_f2 x0p, const vf_f2 x12, float& o0, vf_f2& o12)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_pk_mul_f32 %0, %1, %4 op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_fma_f32 %0, %2, %5, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %0, %3, %5, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "=&v"(o12)
        : "v"(A.c12[0]), "v"(A.c12[1]), "v"(A.c12[2]), "v"(x0p), "v"(x12));
#else
    o12 = pair_of(__builtin_fmaf(A.c12[2][0], x12[1], __builtin_fmaf(A.c12[1][0], x12[0], A.c12[0][0] * x0p[1])),
                  __builtin_fmaf(A.c12[2][1], x12[1], __builtin_fmaf(A.c12[1][1], x12[0], A.c12[0][1] * x0p[1])));
#endif
    o0 = __builtin_fmaf(A.r0[2], x12[1], __builtin_fmaf(A.r0[1], x12[0], A.r0[0] * x0p[1]));
}

// ---- IEEE division of a pair --------------------------------------------------------------------------------------------------------
// hipcc expands an fp32 `/` in the backend, after the SLP vectoriser has run, into 11 instructions that can never be paired:
//   d = v_div_scale(b, b, a)   n = v_div_scale(a, b, a) (writes the flag v_div_fmas reads)   r = v_rcp(d)
//   e = fma(-d, r, 1)   r = fma(e, r, r)   q = n * r   e = fma(-d, q, n)   q = fma(e, r, q)   e = fma(-d, q, n)
//   v_div_fixup(v_div_fmas(e, r, q), b, a)
// div_p restates that sequence (order and negated operand read off the compiler's own code for `/`) with the six plain operations on the
// pair: v_div_scale, v_rcp, v_div_fmas and v_div_fixup per half with the same operands, the six as v_pk_fma_f32 / v_pk_mul_f32 (the
// negations on neg_lo / neg_hi).  17 instructions for two quotients instead of 22, and the same correctly rounded quotient for every
// input -- specials, denormals and the scaled cases included; there is no guard and no range assumption
// (tools/div_pair_probe.hip compares it with `/` bit for bit).  Written with the compiler's builtins, not as an asm statement: the
// flag of each half stays a value the compiler moves into VCC itself (s_mov_b64 vcc, s[..], as in its own schedules), the scaled halves
// land in one register pair without a move, and the wait states around v_rcp / VCC / v_div_fmas remain the compiler's.
#if defined(__HIP_DEVICE_COMPILE__)
VF_PA_FN vf_f2 div_p(const vf_f2 a, const vf_f2 b)
{
    bool f0, f1, unused;
    const vf_f2 d = {__builtin_amdgcn_div_scalef(a[0], b[0], false, &unused), __builtin_amdgcn_div_scalef(a[1], b[1], false, &unused)};
    const vf_f2 n = {__builtin_amdgcn_div_scalef(a[0], b[0], true, &f0), __builtin_amdgcn_div_scalef(a[1], b[1], true, &f1)};
    vf_f2 r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    const vf_f2 one = {1.0f, 1.0f};
    vf_f2 e = __builtin_elementwise_fma(-d, r, one);
    r = __builtin_elementwise_fma(e, r, r);
    vf_f2 q = n * r;
    e = __builtin_elementwise_fma(-d, q, n);
    q = __builtin_elementwise_fma(e, r, q);
    e = __builtin_elementwise_fma(-d, q, n);
    return pair_of(__builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(e[0], r[0], q[0], f0), b[0], a[0]),
                   __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(e[1], r[1], q[1], f1), b[1], a[1]));
}
#else
VF_PA_FN vf_f2 div_p(const vf_f2 a, const vf_f2 b) { return pair_of(a[0] / b[0], a[1] / b[1]); }
#endif
// ... one denominator for both halves (the two scalings of it still differ: they depend on the numerator)
VF_PA_FN vf_f2 div_p(const vf_f2 a, const float b) { return div_p(a, pair_of(b, b)); }

// A lone div_p is a chain of six packed instructions each reading the one before, and hipcc pads every such pair with an s_nop, which a
// lone wave pays like an instruction; left to itself its scheduler runs neighbouring divisions' chains one after the other.  The two
// forms below are div_p and a second division with their steps ALTERNATING, the order pinned by a scheduling barrier after each step
// (no VALU or transcendental instruction moves across VF_PA_SB, mask 0x3FC lets the other kinds pass; registers, the flags' way into
// VCC and every wait state remain the compiler's): the second chain fills the pads of the first.  hipcc hoists no load out of a loop
// that holds such a barrier, so what the loop reads from memory is loaded in front of it (SubstepCfg in vf_dyn_device.hpp).
#if defined(__HIP_DEVICE_COMPILE__)
#define VF_PA_SB __builtin_amdgcn_sched_barrier(0x3FC)
#define VF_PA_SCALE2(a, b, num, fl0, fl1) {__builtin_amdgcn_div_scalef(a[0], b, num, &fl0), __builtin_amdgcn_div_scalef(a[1], b, num, &fl1)}
#define VF_PA_FINISH(e, r, q, fl, b, a) __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(e, r, q, fl), b, a)
#endif
// (o0, o1) = (a0 / b, a1 / b): the quaternion's normalisation
VF_PA_FN void div_p2(const vf_f2 a0, const vf_f2 a1, const float b, vf_f2& o0, vf_f2& o1)
{
#if defined(__HIP_DEVICE_COMPILE__)
    bool f00, f01, f10, f11, unused;
    const vf_f2 one = {1.0f, 1.0f};
    const vf_f2 d0 = VF_PA_SCALE2(a0, b, false, unused, unused), d1 = VF_PA_SCALE2(a1, b, false, unused, unused);
    vf_f2 r0 = {__builtin_amdgcn_rcpf(d0[0]), __builtin_amdgcn_rcpf(d0[1])}, r1 = {__builtin_amdgcn_rcpf(d1[0]), __builtin_amdgcn_rcpf(d1[1])};
    const vf_f2 n0 = VF_PA_SCALE2(a0, b, true, f00, f01), n1 = VF_PA_SCALE2(a1, b, true, f10, f11);
    VF_PA_SB;
    vf_f2 e0 = __builtin_elementwise_fma(-d0, r0, one);
    VF_PA_SB;
    vf_f2 e1 = __builtin_elementwise_fma(-d1, r1, one);
    VF_PA_SB;
    r0 = __builtin_elementwise_fma(e0, r0, r0);
    VF_PA_SB;
    r1 = __builtin_elementwise_fma(e1, r1, r1);
    VF_PA_SB;
    vf_f2 q0 = n0 * r0;
    VF_PA_SB;
    vf_f2 q1 = n1 * r1;
    VF_PA_SB;
    e0 = __builtin_elementwise_fma(-d0, q0, n0);
    VF_PA_SB;
    e1 = __builtin_elementwise_fma(-d1, q1, n1);
    VF_PA_SB;
    q0 = __builtin_elementwise_fma(e0, r0, q0);
    VF_PA_SB;
    q1 = __builtin_elementwise_fma(e1, r1, q1);
    VF_PA_SB;
    e0 = __builtin_elementwise_fma(-d0, q0, n0);
    VF_PA_SB;
    e1 = __builtin_elementwise_fma(-d1, q1, n1);
    VF_PA_SB;
    o0 = pair_of(VF_PA_FINISH(e0[0], r0[0], q0[0], f00, b, a0[0]), VF_PA_FINISH(e0[1], r0[1], q0[1], f01, b, a0[1]));
    o1 = pair_of(VF_PA_FINISH(e1[0], r1[0], q1[0], f10, b, a1[0]), VF_PA_FINISH(e1[1], r1[1], q1[1], f11, b, a1[1]));
#else
    o0 = div_p(a0, b);
    o1 = div_p(a1, b);
#endif
}
// (o, ox) = (a / b, ax / b), the second a single quotient by the same sequence on scalars: the three components of a vector
VF_PA_FN void div_p1(const vf_f2 a, const float ax, const float b, vf_f2& o, float& ox)
{
#if defined(__HIP_DEVICE_COMPILE__)
    bool f0, f1, fx, unused;
    const vf_f2 one = {1.0f, 1.0f};
    const vf_f2 d = VF_PA_SCALE2(a, b, false, unused, unused);
    const float dx = __builtin_amdgcn_div_scalef(ax, b, false, &unused);
    vf_f2 r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    float rx = __builtin_amdgcn_rcpf(dx);
    const vf_f2 n = VF_PA_SCALE2(a, b, true, f0, f1);
    const float nx = __builtin_amdgcn_div_scalef(ax, b, true, &fx);
    VF_PA_SB;
    vf_f2 e = __builtin_elementwise_fma(-d, r, one);
    VF_PA_SB;
    float ex = __builtin_fmaf(-dx, rx, 1.0f);
    VF_PA_SB;
    r = __builtin_elementwise_fma(e, r, r);
    VF_PA_SB;
    rx = __builtin_fmaf(ex, rx, rx);
    VF_PA_SB;
    vf_f2 q = n * r;
    VF_PA_SB;
    float qx = nx * rx;
    VF_PA_SB;
    e = __builtin_elementwise_fma(-d, q, n);
    VF_PA_SB;
    ex = __builtin_fmaf(-dx, qx, nx);
    VF_PA_SB;
    q = __builtin_elementwise_fma(e, r, q);
    VF_PA_SB;
    qx = __builtin_fmaf(ex, rx, qx);
    VF_PA_SB;
    e = __builtin_elementwise_fma(-d, q, n);
    VF_PA_SB;
    ex = __builtin_fmaf(-dx, qx, nx);
    VF_PA_SB;
    o = pair_of(VF_PA_FINISH(e[0], r[0], q[0], f0, b, a[0]), VF_PA_FINISH(e[1], r[1], q[1], f1, b, a[1]));
    ox = VF_PA_FINISH(ex, rx, qx, fx, b, ax);
#else
    o = div_p(a, b);
    ox = ax / b;
#endif
}

// ---- IEEE square root of two pairs ---------------------------------------------------------------------------------------------------
// hipcc expands sqrtf in the backend into one dependent chain per root (read off its code for the roots outside the sub-step loop):
//   s = x < 2^-96;  a = s ? x * 2^32 : x;  r = v_sqrt(a);  d = float(int(r) - 1);  e = fma(-d, r, a);  r1 = 0 >= e ? d : r;
//   u = float(int(r) + 1);  f = fma(-u, r, a);  r2 = 0 < f ? u : r1;  r3 = s ? r2 * 2^-16 : r2;  result = class(a, +-0 | +inf) ? a : r3
// with two or three s_nop pads behind its compares.  sqrt_p2 restates that sequence for FOUR roots, every operation and operand kept: the
// two multiplies and the two residual FMAs of each pair are v_pk_mul_f32 / v_pk_fma_f32 (the negation on neg_lo / neg_hi), v_sqrt, the
// integer steps, the compares and the selects stay per root.  The two pairs' steps alternate behind scheduling barriers as in div_p2, so
// that no packed instruction reads the one before it and the compares of four roots stand between a compare and its select.  The same
// correctly rounded root for every input, no guard, no range assumption (tools/sqrt_pair_probe.hip compares it with sqrtf bit for bit).
// the float k integer steps from r (by value: __builtin_bit_cast of a vector ELEMENT reads element 0 with this compiler)
VF_PA_FN float ulp_step(float r, int k) { return __builtin_bit_cast(float, __builtin_bit_cast(int, r) + k); }
VF_PA_FN void sqrt_p2(const vf_f2 xa, const vf_f2 xb, vf_f2& oa, vf_f2& ob)
{
#if defined(__HIP_DEVICE_COMPILE__)
#define VF_PA_SEL2(c, t, f) {c##0 ? t[0] : f[0], c##1 ? t[1] : f[1]}
#define VF_PA_STEP2(r, k) {ulp_step(r[0], k), ulp_step(r[1], k)}
    const vf_f2 up = {0x1p+32f, 0x1p+32f}, down = {0x1p-16f, 0x1p-16f};
    const bool sa0 = xa[0] < 0x1p-96f, sa1 = xa[1] < 0x1p-96f, sb0 = xb[0] < 0x1p-96f, sb1 = xb[1] < 0x1p-96f;
    const vf_f2 ua = xa * up;
    VF_PA_SB;
    const vf_f2 ub = xb * up;
    VF_PA_SB;
    const vf_f2 a = VF_PA_SEL2(sa, ua, xa), b = VF_PA_SEL2(sb, ub, xb);
    const vf_f2 ra = {__builtin_amdgcn_sqrtf(a[0]), __builtin_amdgcn_sqrtf(a[1])}, rb = {__builtin_amdgcn_sqrtf(b[0]), __builtin_amdgcn_sqrtf(b[1])};
    const vf_f2 da = VF_PA_STEP2(ra, -1), db = VF_PA_STEP2(rb, -1);
    VF_PA_SB;
    const vf_f2 ea = __builtin_elementwise_fma(-da, ra, a);
    VF_PA_SB;
    const vf_f2 eb = __builtin_elementwise_fma(-db, rb, b);
    VF_PA_SB;
    const bool ca0 = 0.0f >= ea[0], ca1 = 0.0f >= ea[1], cb0 = 0.0f >= eb[0], cb1 = 0.0f >= eb[1];
    vf_f2 va = VF_PA_SEL2(ca, da, ra), vb = VF_PA_SEL2(cb, db, rb);
    const vf_f2 pa = VF_PA_STEP2(ra, 1), pb = VF_PA_STEP2(rb, 1);
    VF_PA_SB;
    const vf_f2 fa = __builtin_elementwise_fma(-pa, ra, a);
    VF_PA_SB;
    const vf_f2 fb = __builtin_elementwise_fma(-pb, rb, b);
    VF_PA_SB;
    const bool ga0 = 0.0f < fa[0], ga1 = 0.0f < fa[1], gb0 = 0.0f < fb[0], gb1 = 0.0f < fb[1];
    const vf_f2 wa = VF_PA_SEL2(ga, pa, va), wb = VF_PA_SEL2(gb, pb, vb);
    VF_PA_SB;
    const vf_f2 ta = wa * down;
    VF_PA_SB;
    const vf_f2 tb = wb * down;
    VF_PA_SB;
    va = VF_PA_SEL2(sa, ta, wa);
    vb = VF_PA_SEL2(sb, tb, wb);
    const bool za0 = __builtin_amdgcn_classf(a[0], 0x260), za1 = __builtin_amdgcn_classf(a[1], 0x260);
    const bool zb0 = __builtin_amdgcn_classf(b[0], 0x260), zb1 = __builtin_amdgcn_classf(b[1], 0x260);
    oa = VF_PA_SEL2(za, a, va);
    ob = VF_PA_SEL2(zb, b, vb);
#undef VF_PA_SEL2
#undef VF_PA_STEP2
#else
    oa = pair_of(__builtin_sqrtf(xa[0]), __builtin_sqrtf(xa[1]));
    ob = pair_of(__builtin_sqrtf(xb[0]), __builtin_sqrtf(xb[1]));
#endif
}

}  // namespace vf
