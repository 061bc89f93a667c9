/*
 * qpsk_input.h -- input formats of the receive path: 8-bit G.711 codes (A-law,
 * mu-law) and timeslot-interleaved blocks, converted on the GPU to the layout
 * qpsk_rx_batch() takes.  Many 8 kHz channels reach a host as G.711 codes, one
 * sample of every channel after another; converting on the device halves the
 * bytes that cross PCIe and removes the host's expand-and-transpose pass.
 *
 * A format word is  encoding | layout.
 *   encoding  QPSK_IN_S16   int16 linear samples (little endian)
 *             QPSK_IN_ALAW  8-bit G.711 A-law codes
 *             QPSK_IN_ULAW  8-bit G.711 mu-law codes
 *   layout    QPSK_IN_PLANAR       [nch][T]: channel c's samples are contiguous
 *             QPSK_IN_INTERLEAVED  element (t, c) is src[t * ld + c]; ld >= nch
 *                                  counts elements, so a channel range of a
 *                                  wider trunk is a pointer and its ld
 * with T = nframes * 1880.  For planar input ld is ignored.  The output is
 * always int16 [nch][nframes][1880].
 *
 * G.711 decoding is the exact integer expansion of ITU-T G.711 to 16 bits:
 *   mu-law  u = ~code;  t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7);
 *           value = (u & 0x80) ? 0x84 - t : t - 0x84
 *   A-law   a = code ^ 0x55;  m = (a & 15) << 4;  s = (a >> 4) & 7;
 *           v = s == 0 ? m + 8 : s == 1 ? m + 0x108 : (m + 0x108) << (s - 1);
 *           value = (a & 0x80) ? v : -v
 * (mu-law 0x00 -> -32124, 0x80 -> 32124, 0x7F and 0xFF -> 0; A-law 0x55 -> -8,
 * 0xD5 -> 8, 0x2A -> -32256, 0xAA -> 32256).
 *
 * Errors are those of qpsk_batch.h.  Every argument check runs before any HIP
 * call.  QPSK_EINVAL: an unknown format word, ld < nch with interleaved
 * layout, a NULL pointer with nframes > 0, nch < 1, nframes < 0,
 * nch * nframes >= 2^28.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_batch.h"
#include "qpsk_level.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    QPSK_IN_S16 = 0,
    QPSK_IN_ALAW = 1,
    QPSK_IN_ULAW = 2,
    QPSK_IN_PLANAR = 0,
    QPSK_IN_INTERLEAVED = 0x10,
};

/* Bytes of a source block from its first element to its last: nch * T elements
 * planar, (T - 1) * ld + nch interleaved; 0 for nframes == 0 and for arguments
 * the conversions refuse. */
size_t qpsk_input_bytes(int fmt, int nch, int nframes, long ld);

/* The conversion on the host (plain C, `nthreads` threads over channels): the
 * contract of qpsk_input_convert_device, and what a caller without a GPU at
 * hand expands with. */
int qpsk_input_convert_host(int fmt, const void *src, long ld, int nch, int nframes,
                            int16_t *out, int nthreads);

/* The conversion on the device, enqueued on `stream` (a hipStream_t, NULL =
 * default stream) without synchronising.  Writes exactly nch * T int16 to
 * d_out and nothing else.  d_out is 16-byte aligned; d_src may have any
 * alignment its element size allows (odd addresses for 8-bit codes) and must
 * not overlap d_out.  Both are device pointers of the current device. */
int qpsk_input_convert_device(int fmt, const void *d_src, long ld, int nch, int nframes,
                              int16_t *d_out, void *stream);

/*
 * The conversion with the level meter (qpsk_level.h) in its pass: d_out is
 * exactly what qpsk_input_convert_device writes, and level[c * nframes + f] is
 * exactly qpsk_level_host of row (c, f) of that output -- integer arithmetic,
 * bit for bit.  The samples are metered while the conversion has them in
 * registers: the source is read once, d_out is written once and is not read.
 *
 *   planar G.711   one launch: a wave converts one frame and stores its level.
 *                  No work area (qpsk_input_level_work_bytes is 0).
 *   interleaved    the tiled conversion stores one partial level per channel
 *                  and per part of a frame inside a tile of 128 samples to
 *                  d_work; a second small launch in stream order folds the 15
 *                  or 16 partials of a frame.  16 partials of 16 bytes a
 *                  channel-frame.
 *   planar int16   has no conversion pass: the copy, then qpsk_level_device on
 *                  d_out in stream order.  No work area.
 *
 * Every element of d_level is written once, with a plain store, into memory
 * the caller need not have cleared; there are no atomics, and no workgroup
 * waits for another.  d_work (at least qpsk_input_level_work_bytes bytes,
 * 16-byte aligned; may be NULL where that is 0) holds nothing between calls.
 *
 * Errors: those of qpsk_input_convert_device, and QPSK_EINVAL for a NULL
 * d_level, a d_level that is not 8-byte aligned, a work area that is too small
 * (or NULL where one is needed) or not 16-byte aligned; all checked before any
 * HIP call.  nframes == 0 does nothing and is QPSK_OK.
 */
size_t qpsk_input_level_work_bytes(int fmt, int nch, int nframes, long ld);
int qpsk_input_convert_level_device(int fmt, const void *d_src, long ld, int nch, int nframes,
                                    int16_t *d_out, qpsk_frame_level *d_level,
                                    void *d_work, size_t work_bytes, void *stream);
/* The host twin: qpsk_input_convert_host followed by qpsk_level_host, and what
 * every GPU result is compared with. */
int qpsk_input_convert_level_host(int fmt, const void *src, long ld, int nch, int nframes,
                                  int16_t *out, qpsk_frame_level *level, int nthreads);

/* qpsk_rx_batch() for input in format `fmt`: copies the source block as it is
 * over PCIe, converts it on the device and receives.  Returns what
 * qpsk_rx_batch() returns. */
int qpsk_rx_batch_fmt(qpsk_ctx *ctx, const void *in, int fmt, long ld, int nframes,
                      uint8_t *bits, uint8_t *valid, int32_t *trace, float *soft);

/* qpsk_rx_batch_device() for device input in format `fmt`: the conversion and
 * the receive are enqueued on `stream`.  The converted block lives in a device
 * buffer the context owns, which only grows: like qpsk_rx_batch_device it
 * returns without synchronising, except that a call larger than every earlier
 * one on the context waits for the whole device before it reallocates.  For
 * QPSK_IN_S16 | QPSK_IN_PLANAR both calls are the plain ones: no copy, no
 * buffer.
 *
 * Pointer rules of the device receive calls (qpsk_rx_batch_device of
 * qpsk_batch.h, this call, and the device record calls of qpsk_compact.h).
 * The kernels load and store wider than the element types, so a device
 * pointer needs more than its element's alignment:
 *
 *   d_in     16 bytes   (int4 loads; planar int16 only: a source block in
 *                        another format follows qpsk_input_convert_device)
 *   d_trace  16 bytes   (a frame's row is one 16-byte store)
 *   d_soft    8 bytes   (a symbol is one 8-byte store)
 *   d_bits    2 bytes   (a symbol's two bits are one 2-byte store)
 *   d_valid  any
 *
 * A view that starts at a channel's row keeps these alignments: a frame of
 * input is 3760 bytes, a channel-frame's rows are 62 (bits), 16 (trace) and
 * 248 (soft) bytes.  A call with any other pointer returns QPSK_EINVAL before
 * it touches the context or the device: nothing is launched, and
 * qpsk_rx_frames() stays.  Host pointers (qpsk_rx_batch, qpsk_rx_batch_fmt)
 * need no alignment.
 *
 * What a call writes: every byte of bits [nch][nframes][62] and valid
 * [nch][nframes], and of trace [nch][nframes][4] and soft [nch][nframes][31][2]
 * when given -- the zeros of invalid frames included, so the arrays need no
 * clearing in front of a call -- and nothing else.  d_in is only read.
 * (tests/test_gpu_rx_writeset.py holds both statements.) */
int qpsk_rx_batch_device_fmt(qpsk_ctx *ctx, const void *d_in, int fmt, long ld, int nframes,
                             uint8_t *d_bits, uint8_t *d_valid, int32_t *d_trace,
                             float *d_soft, void *stream);

#ifdef __cplusplus
}
#endif
