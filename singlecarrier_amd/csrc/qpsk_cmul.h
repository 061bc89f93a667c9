// qpsk_cmul.h -- the complex product of the equalizer, as the reference's
// compiler computes it (included by the receive kernels and by
// tests/kernels/cmul_check.hip).
#pragma once

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

// (re, im) pairs as 2-wide vectors: a complex add / complex*real product is one
// packed fp32 instruction (v_pk_add_f32 / v_pk_mul_f32: IEEE per lane, no
// fusion), and the halves never need repacking.
typedef float f2 __attribute__((ext_vector_type(2)));

// Complex values are f2 = (re, im).  cmul(A, C) = (ac - bd, ad + bc) with every
// product and the final sum/difference rounded once, exactly as gcc expands
// the reference's complex products inline: two packed multiplies and one
// packed add (neg on the low half), no fusion.  This is the whole product
// unless both parts come out NaN (cmul_g below).
// (a.x - b.x, a.y + b.y) as ONE v_pk_add_f32 with the low half of b negated
// (LLVM builds it from two packed adds plus moves otherwise); a + (-b) == a - b.
__device__ __forceinline__ f2 addsub(f2 a, f2 b) {
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// The two products, each ONE v_pk_mul_f32 with the broadcast/swap done by
// op_sel (written out: LLVM otherwise copies the high half to a new register
// before broadcasting it).
__device__ __forceinline__ f2 mul_xx(f2 A, f2 C) {   // (A.x * C.x, A.x * C.y)
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(A), "v"(C));
    return r;
}
__device__ __forceinline__ f2 mul_yy_swap(f2 A, f2 C) {   // (A.y * C.y, A.y * C.x)
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(A), "v"(C));
    return r;
}
__device__ __forceinline__ f2 cmul(f2 A, f2 C) {
    const f2 t1 = mul_xx(A, C);        // (ac, ad)
    const f2 t2 = mul_yy_swap(A, C);   // (bd, bc)
    return addsub(t1, t2);             // (ac - bd, ad + bc)
}
// A * conj(C) as the reference rounds it: (a*c - b*(-d), a*(-d) + b*c).  Since
// b*(-d) == -(b*d) and a*(-d) == -(a*d) exactly, that is (ac + bd, -(ad) + bc):
// the same two packed products and ONE packed add with the high half of t1 negated.
__device__ __forceinline__ f2 cmulc(f2 A, f2 C) {
    const f2 t1 = mul_xx(A, C);        // (ac, ad)
    const f2 t2 = mul_yy_swap(A, C);   // (bd, bc)
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[1,0]" : "=v"(r) : "v"(t1), "v"(t2));
    return r;
}

// The reference's products are C99 `complex float` products built by gcc
// without -ffast-math: the form above inline and, when BOTH parts come out NaN,
// the recovery of ISO C99 Annex G (G.5.1): an infinite operand counts as
// (+-1 or +-0) * inf with its NaN partner as +-0, a product that overflowed from
// finite operands likewise, and the result is inf * (the product of those),
// i.e. infinities where the plain form said NaN.  It matters once the
// equalizer state has left fp32 range (full-scale tones do that), never before.
// Out of line: only the exact path calls it (qpsk_rx_back.h).
__device__ __attribute__((noinline)) f2 cmul_recover(float a, float b, float c, float d) {
    const float ac = a * c, bd = b * d, ad = a * d, bc = b * c;
    f2 r = {ac - bd, ad + bc};
    bool recalc = false;
    if (__builtin_isinf(a) || __builtin_isinf(b)) {   // (a + bi) is infinite
        a = __builtin_copysignf(__builtin_isinf(a) ? 1.0f : 0.0f, a);
        b = __builtin_copysignf(__builtin_isinf(b) ? 1.0f : 0.0f, b);
        if (c != c) c = __builtin_copysignf(0.0f, c);
        if (d != d) d = __builtin_copysignf(0.0f, d);
        recalc = true;
    }
    if (__builtin_isinf(c) || __builtin_isinf(d)) {   // (c + di) is infinite
        c = __builtin_copysignf(__builtin_isinf(c) ? 1.0f : 0.0f, c);
        d = __builtin_copysignf(__builtin_isinf(d) ? 1.0f : 0.0f, d);
        if (a != a) a = __builtin_copysignf(0.0f, a);
        if (b != b) b = __builtin_copysignf(0.0f, b);
        recalc = true;
    }
    if (!recalc && (__builtin_isinf(ac) || __builtin_isinf(bd) || __builtin_isinf(ad) ||
                    __builtin_isinf(bc))) {           // overflow from finite operands
        if (a != a) a = __builtin_copysignf(0.0f, a);
        if (b != b) b = __builtin_copysignf(0.0f, b);
        if (c != c) c = __builtin_copysignf(0.0f, c);
        if (d != d) d = __builtin_copysignf(0.0f, d);
        recalc = true;
    }
    if (recalc) {
        const float inf = __builtin_inff();
        r = f2{inf * (a * c - b * d), inf * (a * d + b * c)};
    }
    return r;
}

// the reference's whole product: A * C and A * conj(C)
__device__ __forceinline__ f2 cmul_g(f2 A, f2 C) {
    f2 r = cmul(A, C);
    if (__builtin_expect(r.x != r.x && r.y != r.y, 0)) r = cmul_recover(A.x, A.y, C.x, C.y);
    return r;
}
__device__ __forceinline__ f2 cmulc_g(f2 A, f2 C) {
    f2 r = cmulc(A, C);
    if (__builtin_expect(r.x != r.x && r.y != r.y, 0)) r = cmul_recover(A.x, A.y, C.x, -C.y);
    return r;
}
// EXACT = false: the inline form alone, for frames whose equalizer state stays
// finite (the callers prove that per frame and otherwise redo it with EXACT)
template <bool EXACT>
__device__ __forceinline__ f2 cmul_t(f2 A, f2 C) { return EXACT ? cmul_g(A, C) : cmul(A, C); }
template <bool EXACT>
__device__ __forceinline__ f2 cmulc_t(f2 A, f2 C) { return EXACT ? cmulc_g(A, C) : cmulc(A, C); }

}  // namespace
