// qpsk_stream.hip -- streaming ingest (include/qpsk_stream.h): host chunks in
// pinned slots, H2D / receive / D2H on three HIP streams so consecutive chunks
// overlap.  Host code only; the receive is qpsk_rx_batch_device().
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <stdint.h>
#include <string.h>

#include "qpsk_batch.h"
#include "qpsk_consts.h"
#include "qpsk_hip_host.h"
#include "qpsk_rx_internal.h"
#include "qpsk_stream.h"

namespace {

constexpr int kMaxSlots = 4;

struct Slot {
    qhip::PinBuf<int16_t> h_in;
    qhip::DevBuf<int16_t> d_in;
    // a stream of another input format (qpsk_stream_create_fmt): the source
    // block, pinned and on the device, in place of h_in; d_in is converted from it
    qhip::PinBuf<char> h_raw;
    qhip::DevBuf<char> d_raw;
    qhip::DevBuf<uint8_t> d_bits, d_valid;
    qhip::PinBuf<uint8_t> h_bits, h_valid;
    qhip::DevBuf<int> d_err;     // the chunk's device error word (progress-wait stalls)
    qhip::PinBuf<int> h_err;     // pinned copy, read by qpsk_stream_retrieve
    // a stream with a post-receive pass (qpsk_stream_create_post): the records
    // on the device and pinned, and the count with the groups (one block) in
    // place of h_bits / h_valid
    qhip::DevBuf<char> d_rec;
    qhip::PinBuf<char> h_rec;
    qhip::DevBuf<uint32_t> d_hdr;
    qhip::PinBuf<uint32_t> h_hdr;
    // a post stream whose pass takes the input's levels: the chunk's, on the
    // device and (copied on retrieval, when asked for) pinned
    qhip::DevBuf<char> d_level;
    qhip::PinBuf<char> h_level;
    qhip::Event copied, received, done;
    uint64_t epoch = 0;          // qpsk_rx_epoch() when the chunk was submitted
};

// a slot's stall also goes into the context's own error word (qpsk_rx_sync)
__global__ void err_merge_kernel(int* ctx_err, const int* slot_err) {
    if (threadIdx.x == 0 && *slot_err != 0) atomicOr(ctx_err, *slot_err);
}

}  // namespace

struct qpsk_stream {
    int device = 0, nch = 0, frames = 0, nslot = 0;
    // chunks in another input format than planar int16 (qpsk_stream_create_raw):
    // the format word, the bytes of a chunk's source block and the conversion
    int fmt = 0;
    size_t raw_bytes = 0;
    qpsk_convert_fn convert = nullptr;
    bool plain() const { return convert == nullptr; }
    // chunks that come back through a post-receive pass (qpsk_stream_create_post)
    bool has_post = false;
    qpsk_stream_post post;
    qhip::DevBuf<char> work;   // the pass's work area: one, the passes run in order on s_rx
    // a pass with levels: the conversion's work area, and the levels carried
    // from chunk to chunk [nch], zero at creation
    bool has_level() const { return has_post && post.level_bytes != 0; }
    qhip::DevBuf<char> level_work, carry;
    // released in reverse order: the slots, the streams, then the receiver
    struct RxDestroy {
        void operator()(qpsk_ctx* c) const { qpsk_rx_destroy(c); }
    };
    std::unique_ptr<qpsk_ctx, RxDestroy> rx;
    qhip::Stream s_h2d, s_rx, s_d2h;
    qhip::Stream s_rec;   // a post stream's copy of a retrieved chunk's records
    Slot slot[kMaxSlots];
    uint64_t acquired = 0, submitted = 0, retrieved = 0;
    // A stalled chunk leaves every channel's carried state (rx_timing, windows,
    // history) undefined, so every later chunk of the same epoch (submitted
    // before the next qpsk_rx_reset() on the stream's context) is reported
    // QPSK_ESTALL too.  Chunks are retrieved in submission order, so when a
    // chunk is retrieved every earlier chunk's stall is known.
    bool stalled = false;
    uint64_t stall_epoch = 0;
};

static int stream_alloc(qpsk_stream* s) {
    HCHECK(hipSetDevice(s->device));
    HCHECK(s->s_h2d.create());
    HCHECK(s->s_rx.create());
    HCHECK(s->s_d2h.create());
    if (s->has_post) {
        HCHECK(s->s_rec.create());
        HCHECK(s->work.reserve(s->post.work_bytes));
    }
    if (s->has_level()) {
        HCHECK(s->level_work.reserve(s->post.level_work_bytes));
        HCHECK(s->carry.reserve((size_t)s->nch * s->post.level_bytes));
        // the start of a stream; on s_rx, in front of every pass that reads it
        HCHECK(hipMemsetAsync(s->carry, 0, (size_t)s->nch * s->post.level_bytes, s->s_rx));
    }
    const size_t cf = (size_t)s->nch * (size_t)s->frames;
    for (int i = 0; i < s->nslot; i++) {
        Slot& q = s->slot[i];
        if (s->plain()) {
            HCHECK(q.h_in.reserve(cf * QK_FRAME));
        } else {
            HCHECK(q.h_raw.reserve(s->raw_bytes));
            HCHECK(q.d_raw.reserve(s->raw_bytes));
        }
        if (s->has_post) {
            HCHECK(q.h_rec.reserve(s->post.cap * s->post.rec_bytes));
            HCHECK(q.d_rec.reserve(s->post.cap * s->post.rec_bytes));
            HCHECK(q.d_hdr.reserve(s->post.ngroups + 2));
            HCHECK(q.h_hdr.reserve(s->post.ngroups + 2));
            if (s->has_level()) {
                HCHECK(q.d_level.reserve(cf * s->post.level_bytes));
                HCHECK(q.h_level.reserve(cf * s->post.level_bytes));
            }
        } else {
            HCHECK(q.h_bits.reserve(cf * QK_NBITS));
            HCHECK(q.h_valid.reserve(cf));
        }
        HCHECK(q.d_in.reserve(cf * QK_FRAME));
        HCHECK(q.d_bits.reserve(cf * QK_NBITS));
        HCHECK(q.d_valid.reserve(cf));
        HCHECK(q.d_err.reserve(1));
        HCHECK(q.h_err.reserve(1));
        HCHECK(q.copied.create(hipEventDisableTiming));
        HCHECK(q.received.create(hipEventDisableTiming));
        HCHECK(q.done.create(hipEventDisableTiming));
    }
    return QPSK_OK;
}

extern "C" qpsk_stream* qpsk_stream_create(int device, int nch, int frames, int nslot, int* err) {
    return qpsk_stream_create_mode(device, nch, frames, nslot, QPSK_MODE_REFERENCE, err);
}

extern "C" qpsk_stream* qpsk_stream_create_mode(int device, int nch, int frames, int nslot,
                                                int mode, int* err) {
    return qpsk_stream_create_raw(device, nch, frames, nslot, mode, 0, 0, nullptr, err);
}

qpsk_stream* qpsk_stream_create_raw(int device, int nch, int frames, int nslot, int mode, int fmt,
                                    size_t raw_bytes, qpsk_convert_fn convert, int* err) {
    return qpsk_stream_create_post(device, nch, frames, nslot, mode, fmt, raw_bytes, convert, nullptr, err);
}

qpsk_stream* qpsk_stream_create_post(int device, int nch, int frames, int nslot, int mode, int fmt,
                                     size_t raw_bytes, qpsk_convert_fn convert, const qpsk_stream_post* post,
                                     int* err) {
    if (nch < 1 || frames < 1 || nslot < 1 || nslot > kMaxSlots) return qhip::fail(err, QPSK_EINVAL);
    if (convert && raw_bytes == 0) return qhip::fail(err, QPSK_EINVAL);
    if (post && ((post->level_bytes ? !post->compact_level : !post->compact) || post->rec_bytes == 0))
        return qhip::fail(err, QPSK_EINVAL);
    // (a pass with levels converts with its own hook wherever the stream converts)
    if (post && post->level_bytes && (convert != nullptr) != (post->convert_level != nullptr))
        return qhip::fail(err, QPSK_EINVAL);
    qpsk_stream* s = new (std::nothrow) qpsk_stream();
    if (!s) return qhip::fail(err, QPSK_ENOMEM);
    s->device = device;
    s->nch = nch;
    s->frames = frames;
    s->nslot = nslot;
    s->fmt = fmt;
    s->raw_bytes = raw_bytes;
    s->convert = convert;
    if (post) {
        s->has_post = true;
        s->post = *post;
    }
    int r = QPSK_OK;
    s->rx.reset(qpsk_rx_create_mode(device, nch, mode, &r));
    if (s->rx) {
        qpsk_rx_set_owner(s->rx.get(), s);
        r = stream_alloc(s);
    }
    if (r != QPSK_OK) {
        delete s;
        return qhip::fail(err, r);
    }
    qhip::set_err(err, QPSK_OK);
    return s;
}

extern "C" void qpsk_stream_destroy(qpsk_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->s_h2d);
    (void)hipStreamSynchronize(s->s_rx);
    (void)hipStreamSynchronize(s->s_d2h);
    if (s->has_post) (void)hipStreamSynchronize(s->s_rec);
    delete s;
}

// the slot of the next chunk, or nullptr (*err = QPSK_EBUSY)
static Slot* acquire_slot(qpsk_stream* s, int* err) {
    if (s->acquired != s->submitted) {   // acquired twice without a submit
        qhip::set_err(err, QPSK_OK);
        return &s->slot[s->acquired % (uint64_t)s->nslot];
    }
    // the slot's previous chunk must have been retrieved (its outputs and its
    // input buffer are the caller's until then)
    if (s->acquired - s->retrieved >= (uint64_t)s->nslot) return qhip::fail(err, QPSK_EBUSY);
    qhip::set_err(err, QPSK_OK);
    return &s->slot[s->acquired++ % (uint64_t)s->nslot];
}

extern "C" int16_t* qpsk_stream_acquire(qpsk_stream* s, int* err) {
    if (!s || !s->plain()) return qhip::fail(err, QPSK_EINVAL);
    Slot* q = acquire_slot(s, err);
    return q ? q->h_in.get() : nullptr;
}

extern "C" void* qpsk_stream_acquire_raw(qpsk_stream* s, int* err) {
    if (!s) return qhip::fail(err, QPSK_EINVAL);
    Slot* q = acquire_slot(s, err);
    if (!q) return nullptr;
    return s->plain() ? static_cast<void*>(q->h_in.get()) : static_cast<void*>(q->h_raw.get());
}

extern "C" int qpsk_stream_submit(qpsk_stream* s) {
    if (!s || s->submitted == s->acquired) return QPSK_EINVAL;
    Slot& q = s->slot[s->submitted % (uint64_t)s->nslot];
    const size_t cf = (size_t)s->nch * (size_t)s->frames;
    HCHECK(hipSetDevice(s->device));
    if (s->plain())
        HCHECK(hipMemcpyAsync(q.d_in, q.h_in, sizeof(int16_t) * cf * QK_FRAME, hipMemcpyHostToDevice,
                              s->s_h2d));
    else
        HCHECK(hipMemcpyAsync(q.d_raw, q.h_raw, s->raw_bytes, hipMemcpyHostToDevice, s->s_h2d));
    HCHECK(hipEventRecord(q.copied, s->s_h2d));
    HCHECK(hipStreamWaitEvent(s->s_rx, q.copied, 0));
    if (!s->plain()) {   // the narrow block -> int16 [nch][frames][1880], in front of the receive
        const int cr = s->has_level()
                           ? s->post.convert_level(s->fmt, q.d_raw, s->nch, s->nch, s->frames, q.d_in, q.d_level,
                                                   s->level_work, s->post.level_work_bytes, s->s_rx)
                           : s->convert(s->fmt, q.d_raw, s->nch, s->nch, s->frames, q.d_in, s->s_rx);
        if (cr != QPSK_OK) return cr;
    }
    HCHECK(hipMemsetAsync(q.d_err, 0, sizeof(int), s->s_rx));
    const int r = qpsk_rx_launch(s->rx.get(), q.d_in, s->frames, q.d_bits, q.d_valid, nullptr, nullptr,
                                 s->s_rx, q.d_err);
    if (r != QPSK_OK) return r;
    hipLaunchKernelGGL(err_merge_kernel, dim3(1), dim3(64), 0, s->s_rx, qpsk_rx_err_word(s->rx.get()), q.d_err);
    HCHECK(hipGetLastError());
    if (s->has_post) {   // the dense outputs -> records, count and groups, behind the receive
        const qpsk_stream_post& p = s->post;
        const int pr = s->has_level()
                           ? p.compact_level(q.d_in, !s->plain(), q.d_level, s->carry, p.arg, q.d_bits, q.d_valid,
                                             s->nch, s->frames, p.order, p.cap, q.d_rec, q.d_hdr + 1, q.d_hdr,
                                             s->work, p.work_bytes, s->s_rx)
                           : p.compact(q.d_bits, q.d_valid, s->nch, s->frames, p.order, p.cap, q.d_rec, q.d_hdr + 1,
                                       q.d_hdr, s->work, p.work_bytes, s->s_rx);
        if (pr != QPSK_OK) return pr;
    }
    HCHECK(hipEventRecord(q.received, s->s_rx));
    HCHECK(hipStreamWaitEvent(s->s_d2h, q.received, 0));
    if (s->has_post) {
        HCHECK(hipMemcpyAsync(q.h_hdr, q.d_hdr, sizeof(uint32_t) * (s->post.ngroups + 2), hipMemcpyDeviceToHost,
                              s->s_d2h));
    } else {
        HCHECK(hipMemcpyAsync(q.h_bits, q.d_bits, cf * QK_NBITS, hipMemcpyDeviceToHost, s->s_d2h));
        HCHECK(hipMemcpyAsync(q.h_valid, q.d_valid, cf, hipMemcpyDeviceToHost, s->s_d2h));
    }
    HCHECK(hipMemcpyAsync(q.h_err, q.d_err, sizeof(int), hipMemcpyDeviceToHost, s->s_d2h));
    HCHECK(hipEventRecord(q.done, s->s_d2h));
    q.epoch = qpsk_rx_epoch(s->rx.get());
    s->submitted++;
    return QPSK_OK;
}

extern "C" int qpsk_stream_pending(const qpsk_stream* s) {
    return s ? (int)(s->submitted - s->retrieved) : 0;
}

// the verdict of the chunk in slot q, which has just been retrieved
static int retrieved_verdict(qpsk_stream* s, Slot& q) {
    s->retrieved++;
    // a progress wait of this chunk's receive ran out: its bits are undefined,
    // and so are those of every later chunk of its epoch, which start from the
    // state it left (the slot is released all the same).  The epoch is the
    // chunk's own, taken at submit: a chunk submitted before a reset that ran
    // on the stalled state stays ESTALL, one submitted after it is clean.
    if (*q.h_err != 0) {
        s->stalled = true;
        s->stall_epoch = q.epoch;
        qpsk_rx_mark_stalled(s->rx.get(), q.epoch);   // the context's state too (qpsk_rx_state_save)
    }
    return (s->stalled && q.epoch == s->stall_epoch) ? QPSK_ESTALL : QPSK_OK;
}

extern "C" int qpsk_stream_retrieve(qpsk_stream* s, const uint8_t** bits, const uint8_t** valid) {
    if (!s || s->has_post || !bits || !valid || s->retrieved == s->submitted) return QPSK_EINVAL;
    Slot& q = s->slot[s->retrieved % (uint64_t)s->nslot];
    HCHECK(hipSetDevice(s->device));
    HCHECK(hipEventSynchronize(q.done));
    *bits = q.h_bits;
    *valid = q.h_valid;
    return retrieved_verdict(s, q);
}

int qpsk_stream_retrieve_post(qpsk_stream* s, const void** rec, uint32_t* count, const uint32_t** groups) {
    return qpsk_stream_retrieve_post_level(s, rec, count, groups, nullptr);
}

int qpsk_stream_retrieve_post_level(qpsk_stream* s, const void** rec, uint32_t* count, const uint32_t** groups,
                                    const void** level) {
    if (!s || !s->has_post || !rec || !count || !groups || s->retrieved == s->submitted) return QPSK_EINVAL;
    if (level && !s->has_level()) return QPSK_EINVAL;
    Slot& q = s->slot[s->retrieved % (uint64_t)s->nslot];
    HCHECK(hipSetDevice(s->device));
    HCHECK(hipEventSynchronize(q.done));
    *count = q.h_hdr[0];
    *groups = q.h_hdr + 1;
    *rec = q.h_rec;
    // the count is known: that many records, at most cap, and nothing else
    const size_t m = *count < s->post.cap ? (size_t)*count : s->post.cap;
    if (m > 0) HCHECK(hipMemcpyAsync(q.h_rec, q.d_rec, m * s->post.rec_bytes, hipMemcpyDeviceToHost, s->s_rec));
    if (level) {
        HCHECK(hipMemcpyAsync(q.h_level, q.d_level, (size_t)s->nch * (size_t)s->frames * s->post.level_bytes,
                              hipMemcpyDeviceToHost, s->s_rec));
        *level = q.h_level;
    }
    if (m > 0 || level) HCHECK(hipStreamSynchronize(s->s_rec));
    return retrieved_verdict(s, q);
}

extern "C" qpsk_ctx* qpsk_stream_ctx(qpsk_stream* s) { return s ? s->rx.get() : nullptr; }

// qpsk_records(): host C, qpsk_records.c
