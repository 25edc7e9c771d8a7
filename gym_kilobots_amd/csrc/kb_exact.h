// kb_exact.h -- short forms of the divisions and the square root of the position sweep that give the bits of the IEEE
// operation (plain C++17, also compiled as HIP: the host enumerates them in tests/test_exact_forms_cpu.py and in kb_create).
//
// hipcc lowers `a / b` to v_div_scale x2, v_rcp_f32, five fma, v_div_fmas, v_div_fixup and `sqrtf` to a range test with
// scaling, v_sqrt_f32, two fma corrections with compares and selects, and rescaling: both carry every special case of the
// whole float range.  On the operands of a contact (a guarded range of normal numbers, a divisor that is one of two
// constants) one Newton / Markstein step on the hardware seed rounds the same way.  Each function takes its seed as an
// argument: the forms are proven for EVERY float within the documented error of the seed instruction (1 ulp for
// v_rcp_f32, v_rsq_f32 and v_sqrt_f32), not for one chip's table.  The fused multiply-adds are explicit; the translation
// units are compiled with -ffp-contract=off, so nothing else fuses.
#pragma once

#if defined(__HIPCC__)
#define KB_XF __host__ __device__ inline
#else
#define KB_XF inline
#endif

namespace kb {

// Range of dd = dx * dx + dy * dy in which the square-root and the reciprocal form are used (the wave-uniform guard of the
// position sweep).  Every form is invariant under scaling by a power of four as long as no intermediate leaves the normal
// range: with dd in [2^-40, 2^40] the smallest one, the residual dd - s0 * s0, stays above 2^-90.  len = sqrt(dd) is then in
// [2^-20, 2^20], far from B2_EPSILON: the branch for coincident centres is never taken inside the guard.
constexpr unsigned KB_EXACT_DD_MIN_BITS = 0x2B800000u;          // 2^-40 <= dd
constexpr unsigned KB_EXACT_DD_MAX_BITS = 0x53800000u;          // dd < 2^40 (negative numbers, NaN and 0 fall outside as unsigned)
// ... without the four largest mantissas of a binade: sqrt(dd) then rounds to a len whose mantissa is all ones, the one
// operand on which a Newton step may land on a tie (Markstein's exception: 1 / (2 - 2^-23) from the seed 0.5), and on
// dd = 4 - 2^-22 itself the square root lies within 2^-25 ulp of a rounding boundary.  tests/test_exact_forms_cpu.py
// enumerates both statements.
constexpr unsigned KB_EXACT_MANT_MAX = 0x7FFFFCu;
KB_XF bool kb_exact_guard(float dd) {
    const unsigned u = __builtin_bit_cast(unsigned, dd);
    return u - KB_EXACT_DD_MIN_BITS < KB_EXACT_DD_MAX_BITS - KB_EXACT_DD_MIN_BITS && (u & 0x7FFFFFu) < KB_EXACT_MANT_MAX;
}
// the same guard seen from len = sqrtf(dd): every len the reciprocal form is given lies inside (the host test enumerates it)
KB_XF bool kb_exact_len_guard(float len) {
    const unsigned u = __builtin_bit_cast(unsigned, len);
    return u - 0x35800000u < 0x49800000u - 0x35800000u && (u & 0x7FFFFFu) != 0x7FFFFFu;      // 2^-20 <= len < 2^20, mantissa not all ones
}
// |C| of a position constraint is 0 or in [2^-34, 0.2] (kb_clampf(B2_BAUMGARTE * (sep + B2_LINEAR_SLOP), -0.2, 0)): the
// exponents of the dividend that the check of the constant division covers
constexpr int KB_EXACT_C_EXP_MIN = -34, KB_EXACT_C_EXP_MAX = -3;

// a / K for a constant K with y = RN(1 / K) evaluated once on the host: Markstein's final step.  q is a faithful quotient,
// r = a - K * q is exact, q + r * y rounds to RN(a / K).  r == 0: q is the exact quotient, and it alone carries the sign of a
// zero (-0 / K = -0, where the fma would return +0); the select sits beside the last fma, not behind it.
KB_XF float kb_div_const(float a, float K, float y) {
    const float q = a * y;
    const float r = __builtin_fmaf(-K, q, a);
    const float q1 = __builtin_fmaf(r, y, q);
    return r == 0.0f ? q : q1;
}

// sqrt(dd) from s0 ~ sqrt(dd) (v_sqrt_f32) and y0 ~ 1 / sqrt(dd) (v_rsq_f32), both issued on dd, so neither waits for the
// other: the residual dd - s0 * s0 is exact, half of y0 turns it into the correction of s0.
KB_XF float kb_sqrt_refine(float dd, float s0, float y0) {
    const float r = __builtin_fmaf(-s0, s0, dd);
    return __builtin_fmaf(r, 0.5f * y0, s0);
}

// 1 / len from y0 ~ 1 / len (v_rcp_f32): one Newton step, e = 1 - len * y0 is exact.
KB_XF float kb_rcp_refine(float len, float y0) {
    const float e = __builtin_fmaf(-len, y0, 1.0f);
    return __builtin_fmaf(e, y0, y0);
}

}  // namespace kb
