/*
 * qpsk_level.h -- the input level meter and the squelch: a measure of the
 * signal the receiver is fed, and a gate behind the receive that keeps idle
 * channels out of the records.
 *
 * The receive path (qpsk_batch.h) is bit-identical to the reference, and the
 * reference calls silence a valid frame: on all-zero input every frame comes
 * back valid, with the descrambler's keystream as its bits.  What `valid`
 * means does not change.  This is a layer behind the receive, of the kind of
 * qpsk_input.h in front of it and qpsk_compact.h behind it: a meter pass over
 * the int16 samples, a squelch pass over the dense outputs, and record calls
 * that run receive, meter, squelch and compaction in stream order.
 *
 * The level of a frame (16 bytes, little endian), over the frame's 1880
 * samples x:
 *   sumsq    sum of x * x, at most 1880 * 2^30 (a frame of -32768)
 *   sum      sum of x (the DC term), |sum| <= 1880 * 32768
 *   peak     max |x|, 0 .. 32768
 *   clipped  the samples equal to 32767 or -32768, 0 .. 1880
 * All of it is integer arithmetic: the result is exact and the same whatever
 * the order of the reduction.  `clipped` counts the int16 rails only: expanded
 * G.711 (qpsk_input.h) never reaches them (its largest magnitudes are 32256
 * for A-law and 32124 for mu-law), so a G.711 line that clips shows in `peak`
 * and `sumsq`, never in `clipped`.
 *
 * The meter works on planar int16 [nrows][1880], the block the receive reads;
 * for G.711 and interleaved input that is the block behind
 * qpsk_input_convert_device.  nrows is nch * nframes of the call it
 * accompanies, and row c * nframes + f is frame f of channel c.
 *
 * Errors of the meter calls: QPSK_EINVAL for nrows >= 2^28, a NULL pointer
 * with nrows > 0, and for the device call a d_in that is not 16-byte aligned
 * (the receive's own rule) or a d_out that is not 8-byte aligned; all checked
 * before any HIP call.  nrows == 0 does nothing and is QPSK_OK.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_batch.h"
#include "qpsk_compact.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t sumsq;
    int32_t sum;
    uint16_t peak;
    uint16_t clipped;
} qpsk_frame_level;

/* The host twin: plain C, what every GPU result is compared with. */
int qpsk_level_host(const int16_t *in, size_t nrows, qpsk_frame_level *out);
/* The device pass, asynchronous on `stream` (a hipStream_t): one launch, no
 * atomics, no workgroup waits for another; one 16-byte store per row. */
int qpsk_level_device(const int16_t *d_in, size_t nrows, qpsk_frame_level *d_out, void *stream);
/* The tiling of the device pass, for tests that choose shapes at its edges:
 * the rows one workgroup takes. */
void qpsk_level_tiling(int *rows_per_block);

/* Host helpers, in double.  The level in dB relative to full scale,
 * 10 * log10(sumsq / (1880 * 2^30)): 0 for a frame of -32768, -INFINITY for
 * sumsq == 0. */
double qpsk_level_dbfs(const qpsk_frame_level *level);
/* The smallest sumsq whose qpsk_level_dbfs is at least db: 0 for -INFINITY
 * (and for a NaN), 1880 * 2^30 for every db >= 0. */
uint64_t qpsk_level_sumsq_of_dbfs(double db);

/*
 * The squelch.  level is [nch][nframes], valid_in / valid_out uint8
 * [nch][nframes], bits uint8 [nch][nframes][62], soft float
 * [nch][nframes][31][2], prev and last [nch].
 *
 * The gate, by definition: a frame decision of the receiver lies in a window
 * of decimated symbols taken from the previous input frame and the current one.
 *   w[c][f] = max(level[c][f].sumsq, p)
 *   p       = level[c][f-1].sumsq for f > 0, prev[c].sumsq for f == 0, and 0
 *             when prev is NULL: the start of a stream, where the receiver's
 *             history is zeros
 *   valid_out[c][f] = w[c][f] >= min_sumsq ? valid_in[c][f] : 0
 * It is a conservative gate, not a claim about which samples a decision read.
 * Flags are passed on as they are (2 stays 2).  min_sumsq == 0 squelches
 * nothing.
 *
 * What else is written:
 *   bits, soft  (each may be NULL) the row of a frame that was valid and is
 *               squelched is zeroed: the dense contract, "all zero for invalid
 *               frames".  Rows of frames that stay valid and of frames that
 *               were invalid already are not written.
 *   last        (may be NULL) last[c] = level[c][nframes-1]; prev[c] when
 *               nframes == 0, and zero when prev is NULL too.
 * A trace array of the caller is not touched: trace[2] stays the receiver's
 * verdict.
 *
 * valid_out may be valid_in, and last may be prev (prev[c] is read before
 * last[c] is written).  No other overlap.
 *
 * Errors: QPSK_EINVAL for negative sizes, nch * nframes >= 2^28, NULL level,
 * valid_in or valid_out with nch * nframes > 0, and for the device call a
 * level, prev, last or soft that is not 8-byte aligned or bits that is not
 * 2-byte aligned; all checked before any HIP call.  The device call is
 * asynchronous on `stream`: two launches in stream order.
 */
int qpsk_squelch_host(const qpsk_frame_level *level, const qpsk_frame_level *prev, int nch, int nframes,
                      uint64_t min_sumsq, const uint8_t *valid_in, uint8_t *valid_out, uint8_t *bits,
                      float *soft, qpsk_frame_level *last);
int qpsk_squelch_device(const qpsk_frame_level *d_level, const qpsk_frame_level *d_prev, int nch, int nframes,
                        uint64_t min_sumsq, const uint8_t *d_valid_in, uint8_t *d_valid_out, uint8_t *d_bits,
                        float *d_soft, qpsk_frame_level *d_last, void *stream);

/*
 * Records with squelch: qpsk_rx_batch_records and qpsk_rx_batch_records_device
 * (qpsk_compact.h) in every respect, except that
 *   - the compaction ranks by the squelched `valid` (a squelched frame gives
 *     no record and no row of rec_trace / rec_soft);
 *   - prev_io, [nch] and nullable, is read as `prev` and written as `last`.
 *     It is the caller's: after qpsk_rx_reset_channels, and after a join of a
 *     channel that starts fresh, the caller zeroes those entries.  Nothing of
 *     it is kept in the context, whose snapshots stay as they are;
 *   - level, [nch][nframes] and nullable, receives the meter's output.
 * In the device form prev_io and level are device pointers, 8-byte aligned.
 */
int qpsk_rx_batch_records_squelch(qpsk_ctx *ctx, const int16_t *in, int nframes, uint64_t min_sumsq,
                                  qpsk_frame_level *prev_io, int order, size_t cap, qpsk_frame_rec *rec,
                                  int32_t *rec_trace, float *rec_soft, uint32_t *groups, uint32_t *count,
                                  qpsk_frame_level *level);
int qpsk_rx_batch_records_squelch_device(qpsk_ctx *ctx, const int16_t *d_in, int nframes, uint64_t min_sumsq,
                                         qpsk_frame_level *d_prev_io, int order, size_t cap,
                                         qpsk_frame_rec *d_rec, int32_t *d_rec_trace, float *d_rec_soft,
                                         uint32_t *d_groups, uint32_t *d_count, qpsk_frame_level *d_level,
                                         void *stream);

/*
 * The same two calls for input in format `fmt` (qpsk_input.h), taken as
 * qpsk_rx_batch_records_fmt and qpsk_rx_batch_device_fmt take it: the host
 * form copies the source block over PCIe as it is.  QPSK_IN_S16 |
 * QPSK_IN_PLANAR forwards to the calls above.  For every other format the
 * levels are taken by the conversion itself, while it has the samples in
 * registers (qpsk_input_convert_level_device): the meter does not read the
 * converted block again, and `level` is the level of the decoded samples.
 */
int qpsk_rx_batch_records_squelch_fmt(qpsk_ctx *ctx, const void *in, int fmt, long ld, int nframes,
                                      uint64_t min_sumsq, qpsk_frame_level *prev_io, int order, size_t cap,
                                      qpsk_frame_rec *rec, int32_t *rec_trace, float *rec_soft, uint32_t *groups,
                                      uint32_t *count, qpsk_frame_level *level);
int qpsk_rx_batch_records_squelch_device_fmt(qpsk_ctx *ctx, const void *d_in, int fmt, long ld, int nframes,
                                             uint64_t min_sumsq, qpsk_frame_level *d_prev_io, int order, size_t cap,
                                             qpsk_frame_rec *d_rec, int32_t *d_rec_trace, float *d_rec_soft,
                                             uint32_t *d_groups, uint32_t *d_count, qpsk_frame_level *d_level,
                                             void *stream);

/*
 * Record streams with squelch: qpsk_stream_create_records (qpsk_compact.h)
 * whose chunks pass the meter and the squelch between the receive and the
 * compaction.  The stream owns the carried levels, a device array [nch]: zero
 * at creation -- the start of a stream, where the receiver's history is zeros
 * -- and read as `prev` and written as `last` by each chunk in submit order.
 * A chunk's levels come from the conversion's pass for converted formats and
 * from qpsk_level_device on the slot's input for planar int16.  They stay on
 * the device unless `level` (nullable) is given: then they are copied to the
 * slot's pinned memory on retrieval, as the records are, [nch][frames], good
 * until the slot is acquired again.  qpsk_stream_retrieve_records works on
 * such a stream as on any record stream; qpsk_stream_retrieve is QPSK_EINVAL.
 * With a non-NULL `level` on a record stream without squelch: QPSK_EINVAL.
 */
qpsk_stream *qpsk_stream_create_records_squelch(int device, int nch, int frames, int nslot, int mode, int fmt,
                                                int order, size_t cap, uint64_t min_sumsq, int *err);
int qpsk_stream_retrieve_records_squelch(qpsk_stream *s, const qpsk_frame_rec **rec, uint32_t *count,
                                         const uint32_t **groups, const qpsk_frame_level **level);

#ifdef __cplusplus
}
#endif
