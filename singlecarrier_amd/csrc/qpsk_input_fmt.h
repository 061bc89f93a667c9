/* qpsk_input_fmt.h -- what the host twin (qpsk_input_host.c) and the device
 * code (qpsk_input.hip) of include/qpsk_input.h share: the format word's
 * fields, the argument checks and the G.711 expansion.  Plain C; internal to
 * the library. */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_consts.h"
#include "qpsk_input.h"

#if defined(__HIPCC__)
#define QPSK_IN_FN static __host__ __device__ inline
#else
#define QPSK_IN_FN static inline
#endif

#define QPSK_IN_ENC(fmt) ((fmt) & 0x0f)
#define QPSK_IN_LAYOUT(fmt) ((fmt) & ~0x0f)

/* ITU-T G.711 mu-law code -> 16-bit linear */
QPSK_IN_FN int qpsk_ulaw_decode(unsigned code) {
    const unsigned u = ~code & 0xffu;
    const int t = (int)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u));
    return (u & 0x80u) ? 0x84 - t : t - 0x84;
}

/* ITU-T G.711 A-law code -> 16-bit linear */
QPSK_IN_FN int qpsk_alaw_decode(unsigned code) {
    const unsigned a = (code ^ 0x55u) & 0xffu;
    const int m = (int)((a & 15u) << 4);
    const int s = (int)((a >> 4) & 7u);
    const int v = s == 0 ? m + 8 : s == 1 ? m + 0x108 : (m + 0x108) << (s - 1);
    return (a & 0x80u) ? v : -v;
}

/* bytes of a source element, or 0 for an unknown format word */
QPSK_IN_FN int qpsk_input_esize(int fmt) {
    const int enc = QPSK_IN_ENC(fmt), lay = QPSK_IN_LAYOUT(fmt);
    if (fmt < 0 || (lay != QPSK_IN_PLANAR && lay != QPSK_IN_INTERLEAVED)) return 0;
    return enc == QPSK_IN_S16 ? 2 : (enc == QPSK_IN_ALAW || enc == QPSK_IN_ULAW) ? 1 : 0;
}

/* the checks every entry point shares (pointers apart): QPSK_OK or QPSK_EINVAL */
QPSK_IN_FN int qpsk_input_check(int fmt, int nch, int nframes, long ld) {
    if (qpsk_input_esize(fmt) == 0 || nch < 1 || nframes < 0) return QPSK_EINVAL;
    if ((long long)nch * nframes >= (1LL << 28)) return QPSK_EINVAL;
    if (QPSK_IN_LAYOUT(fmt) == QPSK_IN_INTERLEAVED && ld < (long)nch) return QPSK_EINVAL;
    return QPSK_OK;
}

/* elements from the first to the last of a source block (nframes > 0, checked) */
QPSK_IN_FN size_t qpsk_input_elems(int fmt, int nch, int nframes, long ld) {
    const size_t T = (size_t)nframes * QK_FRAME;
    return QPSK_IN_LAYOUT(fmt) == QPSK_IN_INTERLEAVED ? (T - 1) * (size_t)ld + (size_t)nch
                                                      : (size_t)nch * T;
}
