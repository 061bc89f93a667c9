/* qpsk_fmt.h -- the G.711 and timeslot-interleaved formats of
 * include/qpsk_input.h and include/qpsk_output.h, as the host twins
 * (qpsk_input_host.c, qpsk_output_host.c) and the device code (qpsk_input.hip,
 * qpsk_output.hip, qpsk_tx.hip) share them: the format word's fields and
 * element size, the G.711 expansion and compression, and each direction's
 * argument checks and element counts.  Plain C; internal to the library. */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_consts.h"
#include "qpsk_input.h"
#include "qpsk_output.h"

#if defined(__HIPCC__)
#define QPSK_FMT_FN static __host__ __device__ inline
#else
#define QPSK_FMT_FN static inline
#endif

/* A format word is the same in both directions (QPSK_OUT_* == QPSK_IN_*): the
 * names for code that serves both. */
enum { QPSK_FMT_S16 = QPSK_IN_S16, QPSK_FMT_ALAW = QPSK_IN_ALAW, QPSK_FMT_ULAW = QPSK_IN_ULAW };
enum { QPSK_FMT_PLANAR = QPSK_IN_PLANAR, QPSK_FMT_INTERLEAVED = QPSK_IN_INTERLEAVED };
#define QPSK_FMT_ENC(fmt) ((fmt) & 0x0f)
#define QPSK_FMT_LAYOUT(fmt) ((fmt) & ~0x0f)

/* bytes of an element, or 0 for an unknown format word */
QPSK_FMT_FN int qpsk_fmt_esize(int fmt) {
    const int enc = QPSK_FMT_ENC(fmt), lay = QPSK_FMT_LAYOUT(fmt);
    if (fmt < 0 || (lay != QPSK_FMT_PLANAR && lay != QPSK_FMT_INTERLEAVED)) return 0;
    return enc == QPSK_FMT_S16 ? 2 : (enc == QPSK_FMT_ALAW || enc == QPSK_FMT_ULAW) ? 1 : 0;
}

/* ITU-T G.711 mu-law code -> 16-bit linear */
QPSK_FMT_FN int qpsk_ulaw_decode(unsigned code) {
    const unsigned u = ~code & 0xffu;
    const int t = (int)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u));
    return (u & 0x80u) ? 0x84 - t : t - 0x84;
}

/* ITU-T G.711 A-law code -> 16-bit linear */
QPSK_FMT_FN int qpsk_alaw_decode(unsigned code) {
    const unsigned a = (code ^ 0x55u) & 0xffu;
    const int m = (int)((a & 15u) << 4);
    const int s = (int)((a >> 4) & 7u);
    const int v = s == 0 ? m + 8 : s == 1 ? m + 0x108 : (m + 0x108) << (s - 1);
    return (a & 0x80u) ? v : -v;
}

/* index of the highest set bit of v > 0 */
QPSK_FMT_FN int qpsk_msb(unsigned v) { return 31 - __builtin_clz(v); }

/* 16-bit linear -> ITU-T G.711 mu-law code (G.191 ulaw_compress) */
QPSK_FMT_FN unsigned qpsk_ulaw_encode(int x) {
    const unsigned m = (unsigned)(x < 0 ? ~x : x) >> 2;
    const unsigned a = m + 33u < 0x1fffu ? m + 33u : 0x1fffu;
    const int s = qpsk_msb(a) - 4;   /* a >= 33: 1 .. 8 */
    const unsigned code = ((unsigned)(8 - s) << 4) | (15u - ((a >> s) & 15u));
    return x >= 0 ? code | 0x80u : code;
}

/* 16-bit linear -> ITU-T G.711 A-law code (G.191 alaw_compress) */
QPSK_FMT_FN unsigned qpsk_alaw_encode(int x) {
    const unsigned m = (unsigned)(x < 0 ? ~x : x) >> 4;
    unsigned v = m;
    if (m >= 16u) {
        const int e = qpsk_msb(m) - 3;   /* 1 .. 7 */
        v = (m >> (e - 1)) - 16u + ((unsigned)e << 4);
    }
    if (x >= 0) v |= 0x80u;
    return v ^ 0x55u;
}

/* Input: the checks every entry point shares (pointers apart), QPSK_OK or QPSK_EINVAL */
QPSK_FMT_FN int qpsk_input_check(int fmt, int nch, int nframes, long ld) {
    if (qpsk_fmt_esize(fmt) == 0 || nch < 1 || nframes < 0) return QPSK_EINVAL;
    if ((long long)nch * nframes >= (1LL << 28)) return QPSK_EINVAL;
    if (QPSK_FMT_LAYOUT(fmt) == QPSK_IN_INTERLEAVED && ld < (long)nch) return QPSK_EINVAL;
    return QPSK_OK;
}

/* elements from the first to the last of a source block (nframes > 0, checked) */
QPSK_FMT_FN size_t qpsk_input_elems(int fmt, int nch, int nframes, long ld) {
    const size_t T = (size_t)nframes * QK_FRAME;
    return QPSK_FMT_LAYOUT(fmt) == QPSK_IN_INTERLEAVED ? (T - 1) * (size_t)ld + (size_t)nch
                                                       : (size_t)nch * T;
}

/* The time tiles of the interleaved conversion (128 samples, qpsk_fmt_dev.h) a
 * frame can span: 1880 samples from an offset of up to 120 end inside the 16th */
#define QPSK_IN_LEVEL_FRAME_TILES 16

/* bytes of qpsk_input_convert_level_device's work area: the partial levels of
 * an interleaved block, [nframes][16][nch] of 16 bytes; 0 for a planar block,
 * for nframes == 0 and for arguments the conversions refuse */
QPSK_FMT_FN size_t qpsk_input_level_work(int fmt, int nch, int nframes, long ld) {
    if (qpsk_input_check(fmt, nch, nframes, ld) != QPSK_OK) return 0;
    if (QPSK_FMT_LAYOUT(fmt) != QPSK_IN_INTERLEAVED) return 0;
    return (size_t)nframes * QPSK_IN_LEVEL_FRAME_TILES * (size_t)nch * sizeof(qpsk_frame_level);
}

/* Output: the same for a block of nch channels x n samples */
QPSK_FMT_FN int qpsk_output_check(int fmt, int nch, long n, long src_ld, long ld) {
    if (qpsk_fmt_esize(fmt) == 0 || nch < 1 || n < 0 || src_ld < n) return QPSK_EINVAL;
    if (n != 0 && (long long)nch > ((1LL << 28) * QK_FRAME - 1) / n) return QPSK_EINVAL;   /* nch * n >= 2^28 * 1880 */
    if (ld < (QPSK_FMT_LAYOUT(fmt) == QPSK_OUT_INTERLEAVED ? (long)nch : n)) return QPSK_EINVAL;
    return QPSK_OK;
}

/* elements from the first to the last of a block (n > 0, checked) */
QPSK_FMT_FN size_t qpsk_output_elems(int fmt, int nch, long n, long ld) {
    return QPSK_FMT_LAYOUT(fmt) == QPSK_OUT_INTERLEAVED ? (size_t)(n - 1) * (size_t)ld + (size_t)nch
                                                        : (size_t)(nch - 1) * (size_t)ld + (size_t)n;
}
