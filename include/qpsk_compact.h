/*
 * qpsk_compact.h -- the format layer of the receive output: packed bits and
 * records of the valid frames only, made on the GPU behind the receive.
 *
 * The receive path (qpsk_batch.h) writes dense arrays over every channel-frame:
 * bits uint8 [nch][nframes][62] (one byte per bit, zero rows for invalid
 * frames), valid uint8 [nch][nframes], optionally trace int32 [..][4] and soft
 * float [..][31][2].  On the modem's own signal a fifth of the frames is valid.
 * This layer turns those arrays into the list of the frames that were received,
 * in a stated order, so that nothing else has to cross PCIe.
 *
 * The record (16 bytes, little endian):
 *   channel   the channel, 0 .. nch-1
 *   frame     the frame's position inside the call, 0 .. nframes-1.  A caller
 *             that wants the channel's own 64-bit frame index adds what
 *             qpsk_rx_channel_frames (qpsk_batch.h) gave before the call.
 *   bits      bit i (bit 0 = LSB) is set iff bits[i] == 1, the transmitter's
 *             rule (qpsk_tx.h): bit 2s = Q and bit 2s+1 = I of data symbol s.
 *             Bytes other than 1 give a zero bit.  Bits 62 and 63 are zero.
 *
 * Orders:
 *   QPSK_REC_BY_CHANNEL   records sorted by (channel, frame): the flat order
 *                         of `valid`; a group is one channel, G = nch groups
 *   QPSK_REC_BY_FRAME     records sorted by (frame, channel): time order; a
 *                         group is one frame, G = nframes groups
 * The output is a function of the inputs alone: a record's rank is the number
 * of valid items in front of it in the order (valid[] != 0 is valid).
 *
 * Outputs (each may be NULL except count):
 *   rec        qpsk_frame_rec [cap]
 *   rec_trace  int32 [cap][4], rec_soft float [cap][31][2]: the rows of the
 *              dense arrays at the same rank; NULL (or ignored) when the dense
 *              source is NULL
 *   groups     uint32 [G + 1]: the exclusive prefix of valid frames per group
 *              (records groups[g] .. groups[g+1]-1 are group g's), groups[G] ==
 *              count
 *   count      uint32: the number of valid frames, whatever cap is
 * Capacity: ranks >= cap are not written, and nothing is written past
 * min(count, cap) rows of any array (snprintf semantics); groups and count
 * always describe the whole list.  cap == 0 with NULL record pointers is a
 * pure count.
 *
 * Errors: QPSK_EINVAL for an unknown order, negative sizes, nch * nframes >=
 * 2^28, NULL bits, valid or count (with nch * nframes > 0 for the first two),
 * NULL rec with cap > 0, a work area that is too small or not 4-byte aligned;
 * all checked before any HIP call.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_batch.h"
#include "qpsk_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t channel;
    uint32_t frame;
    uint64_t bits;
} qpsk_frame_rec;

enum {
    QPSK_REC_BY_CHANNEL = 0,
    QPSK_REC_BY_FRAME = 1,
};

/* The dense form: uint8 [n][62] <-> uint64 [n] by the rule above (an invalid
 * frame's zero row gives 0).  Unpacking writes 0/1 bytes.  The device call is
 * asynchronous on `stream` (a hipStream_t); d_words is 8-byte aligned. */
int qpsk_bits_pack_host(const uint8_t *bits, size_t n, uint64_t *words);
int qpsk_bits_unpack_host(const uint64_t *words, size_t n, uint8_t *bits);
int qpsk_bits_pack_device(const uint8_t *d_bits, size_t n, uint64_t *d_words, void *stream);

/* The host twin: plain C, what every GPU result is compared with and the path
 * of a machine without a GPU. */
int qpsk_compact_host(const uint8_t *bits, const uint8_t *valid, const int32_t *trace,
                      const float *soft, int nch, int nframes, int order, size_t cap,
                      qpsk_frame_rec *rec, int32_t *rec_trace, float *rec_soft,
                      uint32_t *groups, uint32_t *count);

/* Bytes of the work area of qpsk_compact_device for these sizes (0 for sizes
 * it refuses). */
size_t qpsk_compact_work_bytes(int nch, int nframes);
/* The tiling of the device call, for tests that choose shapes at its edges:
 * the items one wave ranks (one count of the work area), the items of one
 * workgroup, and the counts the scan's workgroup takes per trip of its loop. */
void qpsk_compact_tiling(int *run_items, int *block_items, int *scan_trip);

/* The conversion alone, device to device, asynchronous on `stream`: three
 * launches that depend on each other in stream order only (counts per run of
 * items, a scan of those counts by one workgroup, the scatter).  d_work: the
 * caller's work area of work_bytes >= qpsk_compact_work_bytes(nch, nframes),
 * 4-byte aligned; its contents before the call do not matter.  d_rec is
 * 8-byte aligned, d_rec_trace, d_rec_soft, d_trace and d_soft 4-byte. */
int qpsk_compact_device(const uint8_t *d_bits, const uint8_t *d_valid, const int32_t *d_trace,
                        const float *d_soft, int nch, int nframes, int order, size_t cap,
                        qpsk_frame_rec *d_rec, int32_t *d_rec_trace, float *d_rec_soft,
                        uint32_t *d_groups, uint32_t *d_count, void *d_work, size_t work_bytes,
                        void *stream);

/* qpsk_rx_batch whose output is records: host memory in, records out.  The
 * dense outputs never leave the device: count, groups and min(count, cap)
 * rows of rec / rec_trace / rec_soft are copied back (a NULL rec_trace or
 * rec_soft is not computed).  Returns qpsk_rx_sync()'s verdict, as
 * qpsk_rx_batch does. */
int qpsk_rx_batch_records(qpsk_ctx *ctx, const int16_t *in, int nframes, int order, size_t cap,
                          qpsk_frame_rec *rec, int32_t *rec_trace, float *rec_soft,
                          uint32_t *groups, uint32_t *count);
/* the same with the input as qpsk_rx_batch_fmt takes it (qpsk_input.h) */
int qpsk_rx_batch_records_fmt(qpsk_ctx *ctx, const void *in, int fmt, long ld, int nframes,
                              int order, size_t cap, qpsk_frame_rec *rec, int32_t *rec_trace,
                              float *rec_soft, uint32_t *groups, uint32_t *count);
/* The asynchronous device form: all pointers are device pointers, the receive
 * and the compaction are enqueued on `stream`; check with qpsk_rx_sync, which
 * waits for the compaction too.  The dense intermediates and the work area are
 * grow-only buffers of the context: like qpsk_rx_batch_device the call returns
 * without synchronising, except that a call larger than every earlier one on
 * the context waits for the whole device before it reallocates them. */
int qpsk_rx_batch_records_device(qpsk_ctx *ctx, const int16_t *d_in, int nframes, int order,
                                 size_t cap, qpsk_frame_rec *d_rec, int32_t *d_rec_trace,
                                 float *d_rec_soft, uint32_t *d_groups, uint32_t *d_count,
                                 void *stream);

/* A stream (qpsk_stream.h) whose chunks come back as records in `order`, at
 * most cap of them per chunk; fmt as in qpsk_stream_create_fmt.  A chunk
 * copies back count, groups and at most min(count, cap) records, never the
 * dense arrays. */
qpsk_stream *qpsk_stream_create_records(int device, int nch, int frames, int nslot, int mode,
                                        int fmt, int order, size_t cap, int *err);
/* qpsk_stream_retrieve's contract for such a stream: *rec (min(*count, cap)
 * records), *count and *groups (uint32 [G + 1]) point into the slot's pinned
 * memory and stay good until the slot is acquired again; QPSK_ESTALL and the
 * epoch rules are qpsk_stream_retrieve's, and the chunk counts as retrieved
 * either way.  Retrieving in the wrong way is QPSK_EINVAL: this call on a
 * plain stream, qpsk_stream_retrieve on a record stream. */
int qpsk_stream_retrieve_records(qpsk_stream *s, const qpsk_frame_rec **rec, uint32_t *count,
                                 const uint32_t **groups);

#ifdef __cplusplus
}
#endif
