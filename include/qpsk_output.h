/*
 * qpsk_output.h -- output formats of the transmit path: 8-bit G.711 codes
 * (A-law, mu-law) and timeslot-interleaved blocks, made on the GPU from the
 * planar int16 rows qpsk_tx_batch() writes.  The mirror of qpsk_input.h: a
 * trunk the library fills is one it can also read, with one byte per sample on
 * the bus in either direction.
 *
 * A format word is  encoding | layout  with the numeric values of QPSK_IN_*,
 * so a block's word can be handed to qpsk_rx_batch_fmt() as it is.
 *   encoding  QPSK_OUT_S16   int16 linear samples (little endian)
 *             QPSK_OUT_ALAW  8-bit G.711 A-law codes
 *             QPSK_OUT_ULAW  8-bit G.711 mu-law codes
 *   layout    QPSK_OUT_PLANAR       element (c, p) is dst[c * ld + p]; ld >= n
 *             QPSK_OUT_INTERLEAVED  element (p, c) is dst[p * ld + c]; ld >= nch
 * A block is nch channels x n samples; n is any count (a transmitter row is
 * npackets * (1880 + gap)).  ld counts elements.
 *
 * G.711 encoding is the truncating integer compression of ITU-T G.191
 * (alaw_compress, ulaw_compress) applied to the 16-bit sample x, the inverse of
 * qpsk_input.h's expansion on every code value (it is not "the nearest table
 * value").  msb(v) = index of the highest set bit.
 *   mu-law  m = x < 0 ? (~x) >> 2 : x >> 2;  a = min(m + 33, 0x1FFF);
 *           s = msb(a) - 4  (1 .. 8);
 *           code = ((8 - s) << 4) | (15 - ((a >> s) & 15));
 *           code |= 0x80 when x >= 0
 *   A-law   m = x < 0 ? (~x) >> 4 : x >> 4;
 *           v = m when m < 16; otherwise e = msb(m) - 3,
 *           v = (m >> (e - 1)) - 16 + (e << 4);
 *           v |= 0x80 when x >= 0;  code = v ^ 0x55
 * (0 -> 0xFF / 0xD5, -1 -> 0x7F / 0x55, 32767 -> 0x80 / 0xAA, -32768 -> 0x00 /
 * 0x2A for mu-law / A-law.  compress(expand(k)) == k for every code but mu-law
 * 0x7F, which expands to 0 and so comes back as 0xFF.)
 *
 * Errors are those of qpsk_batch.h.  Every argument check runs before any HIP
 * call.  QPSK_EINVAL: an unknown format word, ld < nch (interleaved) or ld < n
 * (planar), src_ld < n, a NULL pointer with n > 0, nch < 1, n < 0,
 * nch * n >= 2^28 * 1880, and for the tx calls everything qpsk_tx_batch()
 * refuses.  n == 0 is a no-op returning 0.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_batch.h"
#include "qpsk_input.h"
#include "qpsk_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    QPSK_OUT_S16 = QPSK_IN_S16,
    QPSK_OUT_ALAW = QPSK_IN_ALAW,
    QPSK_OUT_ULAW = QPSK_IN_ULAW,
    QPSK_OUT_PLANAR = QPSK_IN_PLANAR,
    QPSK_OUT_INTERLEAVED = QPSK_IN_INTERLEAVED,
};

/* Bytes of a block from its first element to its last: (nch - 1) * ld + n
 * elements planar, (n - 1) * ld + nch interleaved; 0 for n == 0 and for
 * arguments the conversions refuse. */
size_t qpsk_output_bytes(int fmt, int nch, long n, long ld);

/* The conversion on the host (plain C, `nthreads` threads over channels): the
 * contract of qpsk_output_convert_device, and what a caller without a GPU at
 * hand compands with.  src is planar int16 [nch][src_ld], src_ld >= n. */
int qpsk_output_convert_host(int fmt, const int16_t *src, long src_ld, int nch, long n,
                             void *dst, long ld, int nthreads);

/* The conversion on the device, enqueued on `stream` (a hipStream_t, NULL =
 * default stream) without synchronising.  d_src is planar int16
 * [nch][src_ld], 2-byte aligned, any src_ld >= n.  d_dst may have any
 * alignment its element size allows (odd addresses for 8-bit codes) and must
 * not overlap d_src.  Writes exactly the block's nch * n elements and stores
 * to no byte outside them: planar row tails [n, ld), interleaved columns
 * [nch, ld) of every row and the bytes around the block keep their contents,
 * and no wider word that reaches outside the block is read, modified and
 * written back, so another context may write the neighbouring timeslots of the
 * same trunk at the same time. */
int qpsk_output_convert_device(int fmt, const int16_t *d_src, long src_ld, int nch, long n,
                               void *d_dst, long ld, void *stream);

/* qpsk_tx_batch() with the written block in format `fmt`: n = npackets *
 * (1880 + gap).  Only the block's bytes come back over PCIe; for an
 * interleaved `out` with ld > nch the other columns of the caller's trunk are
 * not written. */
int qpsk_tx_batch_fmt(qpsk_tx_ctx *ctx, const uint8_t *bits, int npackets, void *out, int fmt,
                      long ld);

/* qpsk_tx_batch_device() with the written block in format `fmt`.  Planar
 * G.711 comes out of the modulator's own store pass.  For the interleaved
 * formats the modulator writes int16 into a device buffer the context owns,
 * which only grows (a call larger than every earlier one waits for the device
 * before it reallocates), and the conversion follows on the same stream;
 * qpsk_tx_sync() waits for it too.  The carried state advances exactly as in
 * the plain call.  For QPSK_OUT_S16 | QPSK_OUT_PLANAR both calls are the plain
 * ones: no buffer, no extra kernel. */
int qpsk_tx_batch_device_fmt(qpsk_tx_ctx *ctx, const uint8_t *d_bits, int npackets, void *d_out,
                             int fmt, long ld, void *stream);

/* qpsk_tx_batch_masked() and qpsk_tx_batch_masked_device() (qpsk_tx.h,
 * "Channels that come and go") with the written block in format `fmt`, every
 * format of the two calls above and by the same routes.  An idle slot holds
 * the encoded zero, as the gap does.  active / d_active NULL: the calls above. */
int qpsk_tx_batch_masked_fmt(qpsk_tx_ctx *ctx, const uint8_t *bits, const uint8_t *active,
                             int npackets, void *out, int fmt, long ld);
int qpsk_tx_batch_masked_device_fmt(qpsk_tx_ctx *ctx, const uint8_t *d_bits, const uint8_t *d_active,
                                    int npackets, void *d_out, int fmt, long ld, void *stream);

#ifdef __cplusplus
}
#endif
