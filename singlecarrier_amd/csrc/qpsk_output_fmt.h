/* qpsk_output_fmt.h -- what the host twin (qpsk_output_host.c) and the device
 * code (qpsk_output.hip) of include/qpsk_output.h share: the argument checks
 * and the G.711 compression.  The format word's fields and its element size
 * are qpsk_input_fmt.h's.  Plain C; internal to the library. */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_input_fmt.h"
#include "qpsk_output.h"

/* index of the highest set bit of v > 0 */
QPSK_IN_FN int qpsk_msb(unsigned v) { return 31 - __builtin_clz(v); }

/* 16-bit linear -> ITU-T G.711 mu-law code (G.191 ulaw_compress) */
QPSK_IN_FN unsigned qpsk_ulaw_encode(int x) {
    const unsigned m = (unsigned)(x < 0 ? ~x : x) >> 2;
    const unsigned a = m + 33u < 0x1fffu ? m + 33u : 0x1fffu;
    const int s = qpsk_msb(a) - 4;   /* a >= 33: 1 .. 8 */
    const unsigned code = ((unsigned)(8 - s) << 4) | (15u - ((a >> s) & 15u));
    return x >= 0 ? code | 0x80u : code;
}

/* 16-bit linear -> ITU-T G.711 A-law code (G.191 alaw_compress) */
QPSK_IN_FN unsigned qpsk_alaw_encode(int x) {
    const unsigned m = (unsigned)(x < 0 ? ~x : x) >> 4;
    unsigned v = m;
    if (m >= 16u) {
        const int e = qpsk_msb(m) - 3;   /* 1 .. 7 */
        v = (m >> (e - 1)) - 16u + ((unsigned)e << 4);
    }
    if (x >= 0) v |= 0x80u;
    return v ^ 0x55u;
}

/* the checks every entry point shares (pointers apart): QPSK_OK or QPSK_EINVAL */
QPSK_IN_FN int qpsk_output_check(int fmt, int nch, long n, long src_ld, long ld) {
    if (qpsk_input_esize(fmt) == 0 || nch < 1 || n < 0 || src_ld < n) return QPSK_EINVAL;
    if (n != 0 && (long long)nch > ((1LL << 28) * QK_FRAME - 1) / n) return QPSK_EINVAL;   /* nch * n >= 2^28 * 1880 */
    if (ld < (QPSK_IN_LAYOUT(fmt) == QPSK_IN_INTERLEAVED ? (long)nch : n)) return QPSK_EINVAL;
    return QPSK_OK;
}

/* elements from the first to the last of a block (n > 0, checked) */
QPSK_IN_FN size_t qpsk_output_elems(int fmt, int nch, long n, long ld) {
    return QPSK_IN_LAYOUT(fmt) == QPSK_IN_INTERLEAVED ? (size_t)(n - 1) * (size_t)ld + (size_t)nch
                                                      : (size_t)(nch - 1) * (size_t)ld + (size_t)n;
}
