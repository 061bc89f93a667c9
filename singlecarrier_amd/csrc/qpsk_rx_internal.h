// qpsk_rx_internal.h -- entry points shared inside libqpsk_hip.so (not part of
// the C-ABI in include/).
#pragma once

#include <hip/hip_runtime.h>

#include "qpsk_batch.h"

// qpsk_rx_batch_device() with the device error word the call's progress waits
// report stalls to (nullptr: the context's own, which qpsk_rx_sync() takes).
// qpsk_stream.hip gives each stream slot its own word, so a stall is reported
// by qpsk_stream_retrieve() for the chunk it happened in.
// err_to (nullable): where rx_data_kernel stores the context's error word,
// taken in one atomic exchange once rx_kernel is done (host calls).
int qpsk_rx_launch(qpsk_ctx* c, const int16_t* d_in, int F, uint8_t* d_bits, uint8_t* d_valid,
                   int32_t* d_trace, float* d_soft, hipStream_t s, int* d_err, int* err_to = nullptr);

// The context's own device error word (qpsk_rx_sync() takes it): a stream
// slot's stall is OR-ed into it too, so the context sees every stall.
int* qpsk_rx_err_word(qpsk_ctx* c);
// Bumped by every qpsk_rx_reset(): a stream keeps reporting a stall for every
// later chunk until the per-channel state it corrupted has been reset.
uint64_t qpsk_rx_epoch(const qpsk_ctx* c);
// A stream chunk of epoch `epoch` stalled: if no reset has run since, the
// context's per-channel state is undefined (qpsk_rx_state_save refuses it).
void qpsk_rx_mark_stalled(qpsk_ctx* c, uint64_t epoch);

// Input in another format than planar int16 (include/qpsk_input.h).  The
// receive path and the streams know nothing of formats: qpsk_input.hip, which
// has the conversions, builds the format entry points on the three hooks below,
// and neither qpsk_rx_host.hip nor qpsk_stream.hip refers to a symbol of it.
//
// qpsk_rx_batch() whose input is made on the device: after the staging block
// is ready, `feed` enqueues on s whatever writes int16 [nch][F][1880] to d_in
// (the block's input), in place of the copy of a host array.
typedef int (*qpsk_rx_feed_fn)(void* arg, int16_t* d_in, hipStream_t s);
int qpsk_rx_batch_fed(qpsk_ctx* c, qpsk_rx_feed_fn feed, void* arg, int F, uint8_t* bits, uint8_t* valid,
                      int32_t* trace, float* soft);
// Grow-only device buffers of the context: the source block of a host call as
// it crossed PCIe (the caller has synchronised its previous use: every host
// call does), and the converted block of device calls (a call larger than
// every earlier one waits for the device before the buffer is reallocated).
int qpsk_rx_fmt_raw(qpsk_ctx* c, size_t bytes, char** p);
int qpsk_rx_fmt_conv(qpsk_ctx* c, size_t n, int16_t** p);
// qpsk_stream_create_mode() for chunks that are source blocks of raw_bytes
// bytes in format fmt: a slot's pinned input is such a block, and submit runs
// `convert` (the signature of qpsk_input_convert_device, ld = nch) on the
// receive stream in front of the receive.  convert == nullptr: a plain stream.
typedef int (*qpsk_convert_fn)(int fmt, const void* d_src, long ld, int nch, int nframes, int16_t* d_out,
                               void* stream);
struct qpsk_stream;
qpsk_stream* qpsk_stream_create_raw(int device, int nch, int frames, int nslot, int mode, int fmt,
                                    size_t raw_bytes, qpsk_convert_fn convert, int* err);

// Records in place of the dense outputs (include/qpsk_compact.h).  As with the
// input formats, the receive path and the streams know nothing of records:
// qpsk_compact.hip, which has the compaction, builds the record entry points on
// the hooks below, and neither qpsk_rx_host.hip nor qpsk_stream.hip refers to
// a symbol of it.
//
// Grow-only device buffers of the context for a record call of cf
// channel-frames: the dense intermediates (trace / soft only when asked for),
// the compaction's work area, and for host calls the block the results are
// made in before they are copied back (out_bytes, 0 for none; 16-byte
// aligned).  A call larger than every earlier one waits for the device before
// a buffer is reallocated.
struct qpsk_rec_bufs {
    uint8_t *bits, *valid;
    int32_t* trace;
    float* soft;
    void* work;
    char* out;
};
int qpsk_rx_rec_bufs(qpsk_ctx* c, size_t cf, bool trace, bool soft, size_t work_bytes, size_t out_bytes,
                     qpsk_rec_bufs* b);
// the context's own stream (what its host calls run on)
hipStream_t qpsk_rx_stream(qpsk_ctx* c);
// What qpsk_rx_sync(), the reset and state calls and the host-memory calls
// wait for moves behind the work enqueued on s so far: the compaction that
// follows a record call's receive and still reads the context's buffers.
int qpsk_rx_mark(qpsk_ctx* c, hipStream_t s);
// Waits for the context's latest device call if it went to a caller's stream:
// every host-memory entry point that runs on the context's own stream calls
// this before it touches the per-channel state or a buffer of the context
// (qpsk_rx_batch and qpsk_rx_batch_fed do so themselves).
int qpsk_rx_wait_pending(qpsk_ctx* c);
// A stream whose chunks come back through a post-receive pass: submit runs
// `compact` on the receive stream behind the receive, on the slot's dense
// bits / valid, and copies back the count and the groups (uint32 [1 + ngroups
// + 1] in one block) instead of the dense arrays; qpsk_stream_retrieve_post
// then copies min(count, cap) records of rec_bytes each.
struct qpsk_stream_post {
    int order = 0;
    size_t cap = 0, rec_bytes = 0, ngroups = 0, work_bytes = 0;
    int (*compact)(const uint8_t* d_bits, const uint8_t* d_valid, int nch, int nframes, int order, size_t cap,
                   void* d_rec, uint32_t* d_groups, uint32_t* d_count, void* d_work, size_t work_bytes,
                   void* stream) = nullptr;
    // A pass that also takes the level of every input frame (level_bytes > 0:
    // the bytes of one level).  The slot keeps the chunk's levels [nch][frames]
    // on the device, the stream a carried array [nch] of them, zero at
    // creation, which every chunk's pass reads and writes in submit order.
    // convert_level (nullptr for planar int16 chunks) runs in place of the
    // stream's convert and writes the levels too, with a work area of
    // level_work_bytes; compact_level runs in place of compact, with the
    // slot's input (have_level == false: the levels are still to be made from
    // it), the levels, the carried array and `arg`, and may change d_valid.
    size_t level_bytes = 0, level_work_bytes = 0;
    uint64_t arg = 0;
    int (*convert_level)(int fmt, const void* d_src, long ld, int nch, int nframes, int16_t* d_out, void* d_level,
                         void* d_work, size_t work_bytes, void* stream) = nullptr;
    int (*compact_level)(const int16_t* d_in, bool have_level, void* d_level, void* d_carry, uint64_t arg,
                         const uint8_t* d_bits, uint8_t* d_valid, int nch, int nframes, int order, size_t cap,
                         void* d_rec, uint32_t* d_groups, uint32_t* d_count, void* d_work, size_t work_bytes,
                         void* stream) = nullptr;
};
struct qpsk_stream;
// qpsk_stream_create_raw (convert may be nullptr: planar int16 chunks) with a
// post-receive pass (post == nullptr: none)
qpsk_stream* qpsk_stream_create_post(int device, int nch, int frames, int nslot, int mode, int fmt,
                                     size_t raw_bytes, qpsk_convert_fn convert, const qpsk_stream_post* post,
                                     int* err);
// qpsk_stream_retrieve for such a stream (QPSK_EINVAL on any other)
int qpsk_stream_retrieve_post(qpsk_stream* s, const void** rec, uint32_t* count, const uint32_t** groups);
// The same, and the chunk's levels (level != nullptr; QPSK_EINVAL on a stream
// whose pass takes none): copied to the slot's pinned memory on retrieval, as
// the records are, and good until the slot is acquired again.
int qpsk_stream_retrieve_post_level(qpsk_stream* s, const void** rec, uint32_t* count, const uint32_t** groups,
                                    const void** level);

// The stream that owns a context (qpsk_stream_create_mode): qpsk_rx_reset()
// and qpsk_rx_state_load() refuse with QPSK_EBUSY while it has chunks pending.
struct qpsk_stream;
void qpsk_rx_set_owner(qpsk_ctx* c, const qpsk_stream* s);
extern "C" int qpsk_stream_pending(const qpsk_stream* s);
