// qpsk_rx_host.hip -- the host side of the receive path (include/qpsk_batch.h,
// qpsk_rx_internal.h): the context and its parts, its creation, reset and
// state snapshots, a call's bookkeeping around its launches, and the
// host-memory entry point with its staging.  No device code: the kernels
// and their launches are qpsk_rx.hip's (qpsk_rx_launch_kernels), and all the
// two files share is qpsk_rx_shared.h, so an edit here neither rebuilds the
// kernels nor changes their hash (qpsk_kernel_hash()).  The choice of a kernel
// shape and the staging layout are qpsk_rx_plan.h's; every buffer, event and
// stream is an owning handle of qpsk_hip_host.h.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "qpsk_fft.h"
#include "qpsk_fft_tables.h"
#include "qpsk_hip_host.h"
#include "qpsk_rx_internal.h"
#include "qpsk_rx_plan.h"
#include "qpsk_stream.h"

#pragma clang fp contract(off)

extern "C" long qpsk_hip_live_handles(void) { return qhip::g_live.load(); }

static float bits2f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// The receiver's constant tables, built once per process on first use (a C++11
// function-local static: its initialisation is thread-safe, and contexts
// created from several host threads at once share the one read-only copy).
struct RxTables {
    float2 ptab[QK_FRAME];                 // P[t] * 2^-14
    unsigned long long ksf[QK_KS_FRAMES];  // keystream bits of frame f, 62 per word
};

static RxTables* make_rx_tables() {
    RxTables* t = new RxTables();
    // P[t] = R^(t+1): fbb_rx_phase *= fbb_rx_rect (src/qpsk.c:139), fp32, host
    const float rr = bits2f(QK_RX_RECT_RE_BITS), ri = bits2f(QK_RX_RECT_IM_BITS);
    volatile float pr = 1.0f, pi = 0.0f;  // volatile: keep every op a rounded fp32 op
    for (int k = 0; k < QK_FRAME; k++) {
        const float a = pr * rr - pi * ri;
        const float b = pr * ri + pi * rr;
        pr = a;
        pi = b;
        t->ptab[k] = make_float2(a * 0x1p-14f, b * 0x1p-14f);  // exact power-of-two scale
    }
    // keystream of the RX descrambler (src/scramble.c:57-69), 62 bits per frame
    std::vector<uint8_t> ks(QK_KS_PERIOD);
    uint16_t m = QK_SEED;
    for (int k = 0; k < QK_KS_PERIOD; k++) {
        const uint16_t o = (uint16_t)(((m & 2) >> 1) ^ (m & 1));
        ks[k] = (uint8_t)o;
        m = (uint16_t)((m >> 1) | (o << 14));
    }
    for (int f = 0; f < QK_KS_FRAMES; f++) {
        unsigned long long w = 0;
        for (int b = 0; b < QK_NBITS; b++)
            w |= (unsigned long long)ks[(62 * f + b) % QK_KS_PERIOD] << b;
        t->ksf[f] = w;
    }
    return t;
}

static const RxTables& rx_tables() {
    static const RxTables* const t = make_rx_tables();   // never freed: process lifetime
    return *t;
}

// ---------------------------------------------------------------- a context's parts
namespace {

// The state the kernels carry from one call to the next, per channel slot (ns
// of them, rx_nslot), and the constant tables beside it.  For frame index G
// (the next frame): the history int16 [2][1880] (frames G-2, G-1:
// carry_block), window G's row float2 [168] with mi_G, and rt_G, the last
// three in the arrays of parity G & 1 (rx_kernel reads mi_of / rt_of / win_of
// (g0) at a call's start and writes parity g0 + F at its end).  koff: what
// the channel's own frame index is ahead of the context's, mod 1057 (rx_koff,
// qpsk_rx_plan.h); rx_data_kernel descrambles with it.
struct ChanState {
    size_t ns = 0;
    qhip::DevBuf<float2> ptab;
    qhip::DevBuf<unsigned long long> ks;
    qhip::DevBuf<float> fft;   // FFT-hunt tables (kFftHT floats), QPSK_MODE_FFT_HUNT
    qhip::DevBuf<int16_t> hist;
    qhip::DevBuf<float2> win[2];
    qhip::DevBuf<int> mi[2], rt[2];
    qhip::DevBuf<unsigned> koff;

    // every channel as before its first frame, counting with the context; the
    // memsets are left on s
    int reset(hipStream_t s) {
        HCHECK(hipMemsetAsync(koff, 0, sizeof(unsigned) * ns, s));
        return reset_slots(0, ns, s);
    }

    // slots [c0, c0 + n) as before their first frame (koff is the caller's);
    // the memsets are left on s
    int reset_slots(size_t c0, size_t n, hipStream_t s) {
        HCHECK(hipMemsetAsync(hist + c0 * 2 * QK_FRAME, 0, sizeof(int16_t) * n * 2 * QK_FRAME, s));
        for (int p = 0; p < 2; p++) {
            HCHECK(hipMemsetAsync(win[p] + c0 * kWinStride, 0, sizeof(float2) * n * kWinStride, s));
            HCHECK(hipMemsetAsync(mi[p] + c0, 0, sizeof(int) * n, s));
        }
        int* rt0 = (int*)malloc(sizeof(int) * n);
        if (!rt0) return QPSK_ENOMEM;
        for (size_t i = 0; i < n; i++) rt0[i] = QK_RT0;
        hipError_t e = hipMemcpy(rt[0] + c0, rt0, sizeof(int) * n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(rt[1] + c0, rt0, sizeof(int) * n, hipMemcpyHostToDevice);
        free(rt0);
        return herr(e);
    }

    // koff of channels [c0, c0 + n) = v, on s (synchronised before it returns:
    // the source is pageable)
    int set_koff(size_t c0, size_t n, unsigned v, hipStream_t s) {
        if (v == 0) {
            HCHECK(hipMemsetAsync(koff + c0, 0, sizeof(unsigned) * n, s));
            return QPSK_OK;
        }
        std::vector<unsigned> h(n, v);
        HCHECK(hipMemcpyAsync(koff + c0, h.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice, s));
        HCHECK(hipStreamSynchronize(s));
        return QPSK_OK;
    }

    // A snapshot's body (qpsk_rx_plan.h: the four fields channel-major, each
    // one block) of channels [c0, c0 + n) at parity p, to the host (kind
    // hipMemcpyDeviceToHost) or from it, on s; to the device, the window rows
    // may come from another host block (win_from, n rows)
    int copy(char* host, int c0, size_t n, int p, hipMemcpyKind kind, hipStream_t s,
             const char* win_from = nullptr) {
        auto field = [&](void* dev, size_t bytes) {
            const bool out = kind == hipMemcpyDeviceToHost;
            const hipError_t e = hipMemcpyAsync(out ? (void*)host : dev, out ? dev : (void*)host, bytes, kind, s);
            host += bytes;
            return e;
        };
        HCHECK(field(hist + (size_t)c0 * 2 * QK_FRAME, n * kHistB));
        if (win_from) {
            HCHECK(hipMemcpyAsync(win[p] + (size_t)c0 * kWinStride, win_from, n * kWinB, kind, s));
            host += n * kWinB;
        } else {
            HCHECK(field(win[p] + (size_t)c0 * kWinStride, n * kWinB));
        }
        HCHECK(field(mi[p] + c0, n * sizeof(int)));
        HCHECK(field(rt[p] + c0, n * sizeof(int)));
        return QPSK_OK;
    }
};
static_assert(kWinB == sizeof(float2) * kWinStride, "window row");

// data-symbol jobs of valid frames (rx_kernel -> rx_data_kernel) and the head
// pre-pass outputs, both sized by the largest call
struct JobQueue {
    qhip::DevBuf<float4> jobs;      // kJobF4 words per channel-frame
    qhip::DevBuf<unsigned> njobs;   // [2] counters, alternating by call
    qhip::DevBuf<float2> heads;     // [nch][F][102], QPSK_HEADPASS only
    size_t cap() const { return jobs.cap() / kJobF4; }   // channel-frames

    int reserve(size_t need, bool headpass) {
        if (need > cap()) {
            HCHECK(hipDeviceSynchronize());   // an earlier call may still use the queue
            HCHECK(jobs.reserve(kJobF4 * need));
        }
        if (headpass && kHeadOut * need > heads.cap()) {
            HCHECK(hipDeviceSynchronize());   // an earlier call may still read the heads
            HCHECK(heads.reserve(kHeadOut * need));
        }
        return QPSK_OK;
    }
};

// staging for the host-memory entry point (qpsk_rx_batch): one device block
// (stage_of, qpsk_rx_plan.h) and, for small calls, a pinned host image of it,
// so a call is one H2D and one D2H of pinned memory (the per-frame drop-in
// qpsk_rx_frame is such a call)
struct Staging {
    qhip::DevBuf<char> dev;
    qhip::PinBuf<char> pin;   // same layout; only while small
    size_t frames = 0;

    // (the caller's previous call on the block has been synchronised)
    int grow(int nch, size_t F) {
        if (F <= frames) return QPSK_OK;
        (void)dev.release();
        (void)pin.release();
        frames = 0;
        const Stage g = stage_of((size_t)nch * F);
        HCHECK(dev.reserve(g.end));
        if (g.bits <= kPinnedStage) HCHECK(pin.reserve(g.end));
        frames = F;
        return QPSK_OK;
    }
};

// input in another format than planar int16 (include/qpsk_input.h, built in
// qpsk_input.hip on qpsk_rx_fmt_raw / qpsk_rx_fmt_conv): the source block as
// it crossed PCIe (qpsk_rx_batch_fmt) and the converted block of device calls
// (qpsk_rx_batch_device_fmt).  Empty until such a call.
struct FmtInput {
    qhip::DevBuf<char> raw;
    qhip::DevBuf<int16_t> conv;
};

// a record call's buffers (include/qpsk_compact.h, built in qpsk_compact.hip on
// qpsk_rx_rec_bufs): the dense outputs that stay on the device, the
// compaction's work area and a host call's result block.  Empty until such a call.
struct RecBufs {
    qhip::DevBuf<uint8_t> bits, valid;
    qhip::DevBuf<int32_t> trace;
    qhip::DevBuf<float> soft;
    qhip::DevBuf<char> work, out;
};

// kernel-span accounting: events before rx_kernel, between the kernels, after
// rx_data_kernel, from a pool that is folded into running sums when it is full
struct SpanTimer {
    static constexpr int kEv = 64;
    int device = 0;
    qhip::Event ev[kEv][3];
    int ev_frames[kEv] = {};
    int ev_n = 0;
    bool on = false;
    float pend_ms[2] = {0.0f, 0.0f};
    int pend_frames = 0;

    // a call of F frames starts on s: its slot, or -1 when not timing
    int begin(hipStream_t s, int F, int* slot) {
        *slot = -1;
        if (!on) return QPSK_OK;
        if (ev_n == kEv) {   // pool full: fold pending spans into the totals
            float ms[2];
            int nf;
            const int r = collect(&ms[0], &ms[1], &nf);
            if (r != QPSK_OK) return r;
            pend_ms[0] += ms[0];
            pend_ms[1] += ms[1];
            pend_frames += nf;
        }
        *slot = ev_n++;
        for (int j = 0; j < 3; j++)
            if (!ev[*slot][j]) HCHECK(ev[*slot][j].create());
        HCHECK(hipEventRecord(ev[*slot][0], s));
        ev_frames[*slot] = F;
        return QPSK_OK;
    }

    // waits for the pending spans; their sums since the last collect
    int collect(float* ms_rx, float* ms_data, int* frames) {
        HCHECK(hipSetDevice(device));
        float tot[2] = {pend_ms[0], pend_ms[1]};
        int nf = pend_frames;
        for (int i = 0; i < ev_n; i++) {
            HCHECK(hipEventSynchronize(ev[i][2]));
            for (int k = 0; k < 2; k++) {
                float t = 0.0f;
                HCHECK(hipEventElapsedTime(&t, ev[i][k], ev[i][k + 1]));
                tot[k] += t;
            }
            nf += ev_frames[i];
        }
        ev_n = 0;
        pend_ms[0] = pend_ms[1] = 0.0f;
        pend_frames = 0;
        *ms_rx = tot[0];
        *ms_data = tot[1];
        *frames = nf;
        return QPSK_OK;
    }
};

// qpsk_rx_state_load of a channel range into a fresh context (frame 0) from a
// snapshot at frame G != 0: the context takes frame index G, so every channel
// must be loaded before it may receive (left channels to go; cover marks the
// loaded ones)
struct Assembly {
    std::vector<uint8_t> cover;
    int left = 0;
};

}  // namespace

struct qpsk_ctx {
    int device = 0, nch = 0;
    int mode = QPSK_MODE_REFERENCE;   // receiver semantics, fixed at creation
    int ncu = 256;                    // compute units of the device
    qhip::Stream stream;              // the first handle: released last
    ChanState st;
    JobQueue q;
    Staging stage;
    FmtInput fmt;
    RecBufs rec;
    SpanTimer spans;
    RxKnobs knobs;
    Assembly assembly;
    // per channel: its own frame index minus `frames`, wrapped (rx_index_lead,
    // qpsk_rx_plan.h); all zero unless qpsk_rx_reset_channels / qpsk_rx_state_join
    std::vector<uint64_t> lead;
    qhip::DevBuf<int> d_err;    // [0] device error word (kErrStall), taken by qpsk_rx_sync;
                                // [1] the value it took
    qhip::Event done;           // recorded after the latest call's kernels, on its stream
    bool called = false;        // `done` has been recorded
    // `done` was last recorded on a caller's stream: a host-memory call, which
    // runs on the context's own, waits for it first (qpsk_rx_wait_pending).
    // Host calls synchronise their stream before they return, so after one of
    // them there is nothing left to wait for.
    bool pending = false;
    RxLaunch base{};            // a call's launches, all that never changes filled in
    uint64_t frames = 0;
    uint64_t calls = 0;
    uint64_t epoch = 0;         // qpsk_rx_reset() count (qpsk_rx_epoch)
    uint64_t launches = 0;      // calls launched over the context's life (qpsk_rx_reset keeps it)
    const qpsk_stream* owner = nullptr;   // the stream this context belongs to, if any
    // a call reported QPSK_ESTALL since the last reset: the per-channel state
    // is undefined, and qpsk_rx_state_save refuses to export it
    bool stalled = false;
};

extern "C" int qpsk_rx_reset(qpsk_ctx* c) {
    if (!c) return QPSK_EINVAL;
    // a stream's chunks in flight run on the state cleared here (and one that
    // stalled must keep its epoch): refuse until the stream is drained
    if (c->owner && qpsk_stream_pending(c->owner) > 0) return QPSK_EBUSY;
    HCHECK(hipSetDevice(c->device));
    // calls in flight on other streams read and write the state cleared here
    if (c->called) HCHECK(hipEventSynchronize(c->done));
    HCHECK(hipMemsetAsync(c->q.njobs, 0, sizeof(unsigned) * 2, c->stream));
    HCHECK(hipMemsetAsync(c->d_err, 0, 2 * sizeof(int), c->stream));
    const int r = c->st.reset(c->stream);
    if (r != QPSK_OK) return r;
    HCHECK(hipStreamSynchronize(c->stream));
    c->frames = 0;
    c->calls = 0;
    c->epoch++;
    c->stalled = false;
    c->assembly = Assembly{};
    c->lead.assign((size_t)c->nch, 0);
    return QPSK_OK;
}

int* qpsk_rx_err_word(qpsk_ctx* c) { return c ? c->d_err.get() : nullptr; }
void qpsk_rx_set_owner(qpsk_ctx* c, const qpsk_stream* s) { if (c) c->owner = s; }
uint64_t qpsk_rx_epoch(const qpsk_ctx* c) { return c ? c->epoch : 0; }
void qpsk_rx_mark_stalled(qpsk_ctx* c, uint64_t epoch) {
    if (c && epoch == c->epoch) c->stalled = true;
}

// The FFT hunt's LDS image (fft_hunt()): twiddles of fft_alloc(256, 0/1)
// (src/fft.c:67-74, host C: qpsk_fft_host.c), Q = conj(fft(c)) with
// c[i] = conj(preambletable[i]) for i < 128 (computed by the GPU FFT itself),
// and kf_work's input permutation.
static int fft_hunt_tables(qpsk_ctx* c) {
    float tab[kFftHT];
    qpsk_fft_twiddle_table(256, 0, tab);
    qpsk_fft_twiddle_table(256, 1, tab + 512);
    qpsk_fft_perm_table(256, reinterpret_cast<int*>(tab + 1536));
    float cq[512] = {};
    for (int i = 0; i < QK_NPRE; i++) {
        cq[2 * i] = (float)QK_PRE[i];
        cq[2 * i + 1] = -(float)QK_PRE[i];
    }
    int r = QPSK_OK;
    qpsk_fft_plan* plan = qpsk_fft_alloc(c->device, 256, 0, &r);
    if (!plan) return r;
    r = qpsk_fft(plan, cq, cq, 1);
    qpsk_fft_free(plan);
    if (r != QPSK_OK) return r;
    for (int k = 0; k < 256; k++) {
        tab[1024 + 2 * k] = cq[2 * k];
        tab[1024 + 2 * k + 1] = -cq[2 * k + 1];
    }
    HCHECK(c->st.fft.reserve(kFftHT));
    HCHECK(hipMemcpy(c->st.fft, tab, sizeof tab, hipMemcpyHostToDevice));
    return QPSK_OK;
}

// The environment's test, profiling and A/B settings of a new context of `mode`
static RxKnobs ctx_read_env(int mode) {
    RxKnobs k;
    if (const char* ab = getenv("QPSK_ABLATE")) {   // timing experiments; output invalid
        if (!strcmp(ab, "front")) k.roles = roles_with_served(k.roles, kRoleFront);
        else if (!strcmp(ab, "back")) k.roles = roles_with_served(k.roles, kRoleBack);
        else if (!strcmp(ab, "frontidle")) k.roles |= kFrontIdle;
    }
    if (getenv("QPSK_FORCE_EXACT")) k.roles |= kForceExact;   // tests: exact-division path
    if (const char* ds = getenv("QPSK_DEBUG_STALL")) {          // tests: the QPSK_ESTALL path
        k.roles |= kDebugStall;
        if (!strcmp(ds, "first")) k.stall_calls = 1;           // only the context's first call
    }
    if (getenv("QPSK_DEBUG_BLOCK")) k.short_block = 64;          // tests: rx_kernel's launch-shape guard
    if (const char* w = getenv("QPSK_WIDTH")) {
        const int v = atoi(w);
        k.width = (v == 16 || v == 32 || v == 64) ? v : 0;
    }
    if (const char* hv = getenv("QPSK_HEADPASS")) k.headpass = atoi(hv) != 0 && mode == QPSK_MODE_REFERENCE;
    if (const char* sv = getenv("QPSK_STAGGER")) {   // A/B: the 4x2 fronts' stagger, 512-cycle units
        const int v = atoi(sv);
        if (v >= 0 && v < 256) k.roles = roles_with_stagger(k.roles, v);
    }
    if (const char* pv = getenv("QPSK_PRIO"))
        k.prio = !strcmp(pv, "none") ? kPrioNone : !strcmp(pv, "front") ? kPrioFront : !strcmp(pv, "back") ? kPrioBack : -1;
    if (const char* sh = getenv("QPSK_SHAPE")) {
        k.shape = !strcmp(sh, "4x2") ? Shape::k4x2
                : !strcmp(sh, "2x4d") ? Shape::k2x4d
                : !strcmp(sh, "1x8") ? Shape::k1x8d64 : -1;
    }
    return k;
}

// The buffers a context has from creation, in the order they have always been
// allocated: it decides where the large state arrays land in device memory,
// and every recorded measurement was taken with this one (profiles/host_layer.txt).
static int ctx_alloc(qpsk_ctx* c) {
    ChanState& st = c->st;
    st.ns = rx_nslot(c->nch);
    HCHECK(st.ptab.reserve(QK_FRAME));
    HCHECK(st.ks.reserve(QK_KS_FRAMES));
    HCHECK(st.hist.reserve(st.ns * 2 * QK_FRAME));
    HCHECK(c->q.njobs.reserve(2));
    HCHECK(c->d_err.reserve(2));
    HCHECK(c->done.create(hipEventDisableTiming));
    for (int p = 0; p < 2; p++) {
        HCHECK(st.win[p].reserve(st.ns * kWinStride));
        HCHECK(st.mi[p].reserve(st.ns));
        HCHECK(st.rt[p].reserve(st.ns));
    }
    HCHECK(st.koff.reserve(st.ns));   // (after the arrays above: they stay where they were)
    const RxTables& t = rx_tables();
    HCHECK(hipMemcpy(st.ptab, t.ptab, sizeof t.ptab, hipMemcpyHostToDevice));
    HCHECK(hipMemcpy(st.ks, t.ksf, sizeof t.ksf, hipMemcpyHostToDevice));
    return QPSK_OK;
}

// stream, buffers, tables and the first reset of a new context (device, nch,
// mode and knobs are set)
static int ctx_init(qpsk_ctx* c) {
    HCHECK(hipSetDevice(c->device));
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && n > 0)
        c->ncu = n;
    HCHECK(c->stream.create());
    int r = ctx_alloc(c);
    if (r != QPSK_OK) return r;
    if (c->mode & QPSK_MODE_FFT_HUNT) {
        r = fft_hunt_tables(c);
        if (r != QPSK_OK) return r;
    }
    // what every call's launches share (qpsk_rx_launch sets the rest)
    RxLaunch& l = c->base;
    l.mode = c->mode;
    l.hp = c->knobs.headpass;
    l.short_block = c->knobs.short_block;
    l.hist = c->st.hist;
    l.ptab = c->st.ptab;
    l.ks = c->st.ks;
    l.koff = c->st.koff;
    for (int p = 0; p < 2; p++) {
        l.win[p] = c->st.win[p];
        l.mi[p] = c->st.mi[p];
        l.rt[p] = c->st.rt[p];
    }
    l.njobs = c->q.njobs;
    l.nch = c->nch;
    l.fft_tab = c->st.fft;
    l.ctx_err = c->d_err;
    return qpsk_rx_reset(c);
}

extern "C" qpsk_ctx* qpsk_rx_create(int device, int nch, int* err) {
    return qpsk_rx_create_mode(device, nch, QPSK_MODE_REFERENCE, err);
}

extern "C" qpsk_ctx* qpsk_rx_create_mode(int device, int nch, int mode, int* err) {
    if (nch < 1 || mode < 0 || mode > (QPSK_MODE_DEC752 | QPSK_MODE_FFT_HUNT)) return qhip::fail(err, QPSK_EINVAL);
    if (!qhip::device_ok(device)) return qhip::fail(err, QPSK_ENODEV);
    qpsk_ctx* c = new (std::nothrow) qpsk_ctx();
    if (!c) return qhip::fail(err, QPSK_ENOMEM);
    c->device = c->spans.device = device;
    c->nch = nch;
    c->mode = mode;
    c->knobs = ctx_read_env(mode);
    const int r = ctx_init(c);
    if (r != QPSK_OK) {
        delete c;
        return qhip::fail(err, r);
    }
    qhip::set_err(err, QPSK_OK);
    return c;
}

// ---------------------------------------------------------------- state snapshots
// qpsk_batch.h qpsk_rx_state_*: the per-channel state of ChanState for the
// context's frame index G (the next frame), in the layout of qpsk_rx_plan.h.
extern "C" size_t qpsk_rx_state_size(int n) { return rx_state_size(n); }

// the checks both directions share; waits for the context's calls in flight
static int state_begin(qpsk_ctx* c, int c0, int n, const void* buf, size_t size) {
    if (!c || !buf || n < 1 || c0 < 0 || c0 > c->nch - n || size < rx_state_size(n)) return QPSK_EINVAL;
    if (c->owner && qpsk_stream_pending(c->owner) > 0) return QPSK_EBUSY;
    HCHECK(hipSetDevice(c->device));
    if (c->called) HCHECK(hipEventSynchronize(c->done));
    return QPSK_OK;
}

// A stall (reported, or still in the error word: peeked, not taken, so
// qpsk_rx_sync still reports it) leaves every channel's state undefined:
// QPSK_ESTALL then.  (The context's calls in flight have been waited for.)
static int state_defined(qpsk_ctx* c) {
    if (!c->stalled) {
        int e = 0;
        HCHECK(hipMemcpyAsync(&e, c->d_err, sizeof e, hipMemcpyDeviceToHost, c->stream));
        HCHECK(hipStreamSynchronize(c->stream));
        if (e != 0) return QPSK_ESTALL;
    }
    return c->stalled ? QPSK_ESTALL : QPSK_OK;
}

// n window rows (kWinB bytes each) negated in place: what the rows of a
// channel are in a context whose frame index differs from the channel's own by
// an odd number (rx_lead_odd, qpsk_rx_plan.h).  Zeros keep their sign: sums of
// the FIR that cancel exactly are +0 under either mixer sign.
static void negate_windows(char* w, size_t n) {
    for (size_t i = 0; i < n; i++) {
        uint32_t* f = reinterpret_cast<uint32_t*>(w + i * kWinB);
        for (int k = 0; k < 2 * kWinObs; k++)
            if ((f[k] & 0x7fffffffu) != 0) f[k] ^= 0x80000000u;
    }
}

extern "C" int qpsk_rx_state_save(qpsk_ctx* c, int c0, int n, void* buf, size_t size) {
    int r = state_begin(c, c0, n, buf, size);
    if (r != QPSK_OK) return r;
    // channels still to be loaded (qpsk_rx_state_load) hold no state of frame G
    if (c->assembly.left > 0) return QPSK_EINVAL;
    r = state_defined(c);
    if (r != QPSK_OK) return r;
    // a snapshot has one frame index: the range's own
    const uint64_t lead = c->lead[(size_t)c0];
    for (int i = c0; i < c0 + n; i++)
        if (c->lead[(size_t)i] != lead) return QPSK_EINVAL;
    const uint64_t own = rx_own_index(c->frames, lead);
    StateHdr h{};
    memcpy(h.magic, kStateMagic, sizeof h.magic);
    h.version = 1;
    h.hdr_bytes = sizeof h;
    h.mode = c->mode;
    h.n = n;
    h.frame = own;
    h.hist_bytes = (uint32_t)kHistB;
    h.win_bytes = (uint32_t)kWinB;
    char* o = static_cast<char*>(buf);
    memcpy(o, &h, sizeof h);
    o += sizeof h;
    const size_t nn = (size_t)n;
    r = c->st.copy(o, c0, nn, (int)(c->frames & 1u), hipMemcpyDeviceToHost, c->stream);
    if (r != QPSK_OK) return r;
    HCHECK(hipStreamSynchronize(c->stream));
    // window slots past dec[mi+162] (the last data symbol's taps, SURVEY.md
    // A.6) are never read; the fronts leave whatever their dec buffer held
    // there (the split FIR skips dec[255..289] when mi < 93).  Zeroed, so a
    // snapshot is a function of the channel's state alone.
    char* w = o + nn * kHistB;
    for (size_t i = 0; i < nn; i++)
        memset(w + i * kWinB + kWinObs * sizeof(float2), 0, (kWinStride - kWinObs) * sizeof(float2));
    if (rx_lead_odd(own, c->frames)) negate_windows(w, nn);   // the channels' own convention
    return QPSK_OK;
}

// a snapshot's header, checked against the context and the range it goes to
static int state_header(const qpsk_ctx* c, int n, const void* buf, StateHdr* h) {
    memcpy(h, buf, sizeof *h);
    if (memcmp(h->magic, kStateMagic, sizeof h->magic) != 0 || h->version != 1 || h->hdr_bytes != sizeof *h ||
        h->n != n || h->mode != c->mode || h->hist_bytes != kHistB || h->win_bytes != kWinB)
        return QPSK_EINVAL;
    return QPSK_OK;
}

extern "C" int qpsk_rx_state_load(qpsk_ctx* c, int c0, int n, const void* buf, size_t size) {
    int r = state_begin(c, c0, n, buf, size);
    if (r != QPSK_OK) return r;
    StateHdr h;
    r = state_header(c, n, buf, &h);
    if (r != QPSK_OK) return r;
    // the context's index or a fresh context (qpsk_rx_state_join takes any)
    if (c->frames != h.frame && c->frames != 0) return QPSK_EINVAL;
    // a channel range at frame G != 0 into a fresh context moves the context's
    // frame index to G for every channel: the others must be loaded too
    // (from this or other snapshots at G) before the context may receive
    const bool assemble = c->assembly.left > 0 || (c->frames == 0 && h.frame != 0 && n < c->nch);
    // (hipMemcpyHostToDevice only reads the buffer)
    char* o = const_cast<char*>(static_cast<const char*>(buf)) + sizeof h;
    r = c->st.copy(o, c0, (size_t)n, (int)(h.frame & 1u), hipMemcpyHostToDevice, c->stream);
    if (r != QPSK_OK) return r;
    HCHECK(hipStreamSynchronize(c->stream));
    if (assemble) {
        Assembly& a = c->assembly;
        if (a.cover.empty()) {
            a.cover.assign((size_t)c->nch, 0);
            a.left = c->nch;
            // every channel moves to the snapshot's index with the context
            c->lead.assign((size_t)c->nch, 0);
            HCHECK(hipMemsetAsync(c->st.koff, 0, sizeof(unsigned) * c->st.ns, c->stream));
            HCHECK(hipStreamSynchronize(c->stream));
        }
        for (int i = c0; i < c0 + n; i++)
            if (!a.cover[(size_t)i]) {
                a.cover[(size_t)i] = 1;
                a.left--;
            }
        if (a.left == 0) a.cover.clear();
    }
    // the loaded channels count with the context
    r = c->st.set_koff((size_t)c0, (size_t)n, 0, c->stream);
    if (r != QPSK_OK) return r;
    HCHECK(hipStreamSynchronize(c->stream));
    for (int i = c0; i < c0 + n; i++) c->lead[(size_t)i] = 0;
    c->frames = h.frame;
    return QPSK_OK;
}

extern "C" int qpsk_rx_state_join(qpsk_ctx* c, int c0, int n, const void* buf, size_t size) {
    int r = state_begin(c, c0, n, buf, size);
    if (r != QPSK_OK) return r;
    // (a context under assembly has no frame index to join at yet)
    if (c->assembly.left > 0) return QPSK_EINVAL;
    StateHdr h;
    r = state_header(c, n, buf, &h);
    if (r != QPSK_OK) return r;
    const char* o = static_cast<const char*>(buf) + sizeof h;
    const size_t nn = (size_t)n;
    // the state of the channels' next frame goes where the context's next
    // frame reads it: its current parity.  The snapshot's rows are in the
    // channels' own convention (qpsk_rx_state_save).
    std::vector<char> win;
    if (rx_lead_odd(h.frame, c->frames)) {
        win.assign(o + nn * kHistB, o + nn * (kHistB + kWinB));
        negate_windows(win.data(), nn);
    }
    r = c->st.copy(const_cast<char*>(o), c0, nn, (int)(c->frames & 1u), hipMemcpyHostToDevice, c->stream,
                   win.empty() ? nullptr : win.data());
    if (r != QPSK_OK) return r;
    r = c->st.set_koff((size_t)c0, nn, rx_koff(h.frame, c->frames), c->stream);
    if (r != QPSK_OK) return r;
    HCHECK(hipStreamSynchronize(c->stream));
    for (int i = c0; i < c0 + n; i++) c->lead[(size_t)i] = rx_index_lead(h.frame, c->frames);
    return QPSK_OK;
}

extern "C" int qpsk_rx_reset_channels(qpsk_ctx* c, int c0, int n) {
    if (!c || n < 1 || c0 < 0 || c0 > c->nch - n) return QPSK_EINVAL;
    if (c->owner && qpsk_stream_pending(c->owner) > 0) return QPSK_EBUSY;
    // channels of a context under assembly hold no state to go on beside
    if (c->assembly.left > 0) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    // calls in flight read and write the state cleared here
    if (c->called) HCHECK(hipEventSynchronize(c->done));
    // a stall leaves every channel undefined and the context's epoch open:
    // only qpsk_rx_reset recovers it
    int r = state_defined(c);
    if (r != QPSK_OK) return r;
    r = c->st.reset_slots((size_t)c0, (size_t)n, c->stream);
    if (r != QPSK_OK) return r;
    r = c->st.set_koff((size_t)c0, (size_t)n, rx_koff(0, c->frames), c->stream);
    if (r != QPSK_OK) return r;
    HCHECK(hipStreamSynchronize(c->stream));
    for (int i = c0; i < c0 + n; i++) c->lead[(size_t)i] = rx_index_lead(0, c->frames);
    return QPSK_OK;
}

extern "C" int qpsk_rx_channel_frames(const qpsk_ctx* c, int c0, int n, uint64_t* out) {
    if (!c || !out || n < 1 || c0 < 0 || c0 > c->nch - n) return QPSK_EINVAL;
    for (int i = 0; i < n; i++) out[i] = rx_own_index(c->frames, c->lead[(size_t)(c0 + i)]);
    return QPSK_OK;
}

extern "C" void qpsk_rx_destroy(qpsk_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
}

// Internal, not part of the C-ABI in include/ (tests: a context made under
// QPSK_SHAPE / QPSK_WIDTH / QPSK_HEADPASS launches what the knobs name): the
// rx_kernel shape of the context's calls, "+head" with the head pre-pass.
extern "C" const char* qpsk_rx_plan_name(const qpsk_ctx* c) {
    if (!c) return "";
    static const char* const names[2][5] = {{"4x2", "2x4d", "1x8d64", "1x8q16", "1x8q32"},
                                            {"4x2+head", "2x4d+head", "1x8d64+head", "1x8q16+head", "1x8q32+head"}};
    static_assert(Shape::k4x2 == 0 && Shape::k2x4d == 1 && Shape::k1x8d64 == 2 && Shape::k1x8q16 == 3 &&
                  Shape::k1x8q32 == 4, "names follow Shape::Kind");
    const int kind = pick_shape(c->knobs, c->nch, c->ncu).kind;
    return kind >= 0 && kind < 5 ? names[c->knobs.headpass ? 1 : 0][kind] : "";
}

extern "C" int qpsk_rx_channels(const qpsk_ctx* c) { return c ? c->nch : 0; }
extern "C" int qpsk_rx_mode(const qpsk_ctx* c) { return c ? c->mode : QPSK_EINVAL; }
extern "C" uint64_t qpsk_rx_frames(const qpsk_ctx* c) { return c ? c->frames : 0; }

// A call's launches (qpsk_rx_batch_device) and the bookkeeping around them; the
// launches themselves are qpsk_rx.hip's (qpsk_rx_launch_kernels).  d_err: the device error word
// the call's progress waits report to: the context's (qpsk_rx_sync takes it),
// or a caller's own (qpsk_stream.hip: one per stream slot, so a stall is
// reported with the chunk it belongs to).
int qpsk_rx_launch(qpsk_ctx* c, const int16_t* d_in, int F, uint8_t* d_bits, uint8_t* d_valid,
                   int32_t* d_trace, float* d_soft, hipStream_t s, int* d_err, int* err_to) {
    if (!c || F < 0 || (F > 0 && (!d_in || !d_bits || !d_valid))) return QPSK_EINVAL;
    if (c->assembly.left > 0) return QPSK_EINVAL;   // channels not yet loaded (qpsk_rx_state_load)
    if (F == 0) return QPSK_OK;
    // the kernels' loads and stores are wider than the elements (qpsk_rx_plan.h);
    // refused before anything of the context or the device is touched
    if (!rx_ptrs_aligned(d_in, d_bits, d_valid, d_trace, d_soft)) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    const size_t need = (size_t)c->nch * (size_t)F;   // every frame valid, at most
    // job slots are addressed with 32-bit byte offsets (slot * 16); 2^28 channel-
    // frames would be 1 TB of input, beyond any device's memory
    if (need >= ((size_t)1 << 28)) return QPSK_EINVAL;
    int r = c->q.reserve(need, c->knobs.headpass);
    if (r != QPSK_OK) return r;
    int slot;
    r = c->spans.begin(s, F, &slot);
    if (r != QPSK_OK) return r;
    Shape sh = pick_shape(c->knobs, c->nch, c->ncu);
    if (c->knobs.stall_calls >= 0 && c->launches >= (uint64_t)c->knobs.stall_calls) sh.roles &= ~kDebugStall;
    RxLaunch l = c->base;
    l.s = s;
    l.kind = sh.kind;
    l.roles = sh.roles;
    l.F = F;
    // the kernels use the frame index only as g & 1 (mixer sign, state parity)
    // and g % QK_KS_FRAMES (descrambler word): its residue mod 2 * 1057 is
    // right for any 64-bit c->frames, and g0 + F stays far below 2^32
    l.g0 = (unsigned)(c->frames % (uint64_t)(2 * QK_KS_FRAMES));
    l.parity = (int)(c->calls & 1u);
    l.in = d_in;
    l.bits = d_bits;
    l.valid = d_valid;
    l.trace = d_trace;
    l.soft = d_soft;
    l.jobs = c->q.jobs;
    l.jobs_cap = c->q.cap();
    l.heads = c->q.heads;
    l.err = d_err ? d_err : c->d_err.get();
    l.err_to = err_to;
    l.ev_mid = slot >= 0 ? (hipEvent_t)c->spans.ev[slot][1] : nullptr;
    l.ev_end = slot >= 0 ? (hipEvent_t)c->spans.ev[slot][2] : nullptr;
    const int lr = qpsk_rx_launch_kernels(l);
    if (lr != QPSK_OK) return lr;
    HCHECK(hipEventRecord(c->done, s));
    c->called = true;
    c->pending = s != (hipStream_t)c->stream;
    c->frames += (uint64_t)F;
    c->calls++;
    c->launches++;
    return QPSK_OK;
}

extern "C" int qpsk_rx_batch_device(qpsk_ctx* c, const int16_t* d_in, int F, uint8_t* d_bits,
                                    uint8_t* d_valid, int32_t* d_trace, float* d_soft,
                                    void* stream) {
    return qpsk_rx_launch(c, d_in, F, d_bits, d_valid, d_trace, d_soft, (hipStream_t)stream,
                          nullptr, nullptr);
}

// qpsk_rx_internal.h: what follows a call's kernels on s and still uses the
// context's buffers (a record call's compaction) is covered by `done` too
int qpsk_rx_mark(qpsk_ctx* c, hipStream_t s) {
    if (!c) return QPSK_EINVAL;
    HCHECK(hipEventRecord(c->done, s));
    c->called = true;
    c->pending = s != (hipStream_t)c->stream;
    return QPSK_OK;
}

// qpsk_rx_internal.h: a device call still pending on a caller's stream writes
// the per-channel state, the job queue and the context's format and record
// buffers, which a host-memory call on the context's own stream is about to use
int qpsk_rx_wait_pending(qpsk_ctx* c) {
    if (!c) return QPSK_EINVAL;
    if (!c->pending) return QPSK_OK;
    HCHECK(hipSetDevice(c->device));
    HCHECK(hipEventSynchronize(c->done));
    c->pending = false;
    return QPSK_OK;
}

// Waits for the context's latest call (an event recorded on its stream, so the
// stream may since have been destroyed) and reports a device-side failure of
// any call since the previous check.  Calls on one context depend on each
// other through the per-channel state, so they are ordered (one stream, or
// streams the caller chains); the latest call's completion covers them all.
extern "C" int qpsk_rx_sync(qpsk_ctx* c) {
    if (!c) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    if (c->called) HCHECK(hipEventSynchronize(c->done));
    const int r = qpsk_rx_take_err(c->d_err, c->stream);
    if (r != QPSK_OK) return r;
    int e = 0;
    HCHECK(hipMemcpyAsync(&e, c->d_err + 1, sizeof e, hipMemcpyDeviceToHost, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    if (e != 0) c->stalled = true;
    return e == 0 ? QPSK_OK : QPSK_ESTALL;
}

extern "C" int qpsk_rx_timing_enable(qpsk_ctx* c, int on) {
    if (!c) return QPSK_EINVAL;
    c->spans.on = on != 0;
    return QPSK_OK;
}

extern "C" int qpsk_rx_timing_split(qpsk_ctx* c, float* ms_rx, float* ms_data, int* frames) {
    if (!c || !ms_rx || !ms_data || !frames) return QPSK_EINVAL;
    return c->spans.collect(ms_rx, ms_data, frames);
}

extern "C" int qpsk_rx_timing_collect(qpsk_ctx* c, float* ms, int* frames) {
    if (!ms) return QPSK_EINVAL;
    float a = 0.0f, b = 0.0f;
    const int r = qpsk_rx_timing_split(c, &a, &b, frames);
    if (r == QPSK_OK) *ms = a + b;
    return r;
}

// qpsk_rx_batch (feed == nullptr: `in` goes to the staging block as it is) and
// qpsk_rx_batch_fed (`feed` fills the staging block's input on the context's
// stream, qpsk_rx_internal.h)
static int rx_batch_host(qpsk_ctx* c, const int16_t* in, qpsk_rx_feed_fn feed, void* arg, int F, uint8_t* bits,
                         uint8_t* valid, int32_t* trace, float* soft) {
    const bool plain = feed == nullptr;
    if (!c || F < 0 || (F > 0 && ((plain && !in) || !bits || !valid))) return QPSK_EINVAL;
    if (c->assembly.left > 0) return QPSK_EINVAL;   // channels not yet loaded (qpsk_rx_state_load)
    if (F == 0) return QPSK_OK;
    HCHECK(hipSetDevice(c->device));
    // a device call still pending on a caller's stream: this call continues
    // from the state it leaves
    int r = qpsk_rx_wait_pending(c);
    if (r != QPSK_OK) return r;
    r = c->stage.grow(c->nch, (size_t)F);
    if (r != QPSK_OK) return r;
    const size_t cf = (size_t)c->nch * F;
    const Stage g = stage_of(cf);
    const bool pin = c->stage.pin && g.bits <= kPinnedStage;
    // pinned: the caller's input is copied into the pinned image (a host memcpy)
    // and moves in one DMA, outputs come back in one; pageable otherwise
    const StageView d{c->stage.dev, g}, h{pin ? c->stage.pin.get() : nullptr, g};
    const size_t nin = sizeof(int16_t) * cf * QK_FRAME;
    const size_t ntr = sizeof(int32_t) * cf * 4, nso = sizeof(float) * cf * QK_NDSYM * 2;
    // the kernels of this call on the block v; the error word comes back with
    // the outputs (rx_data_kernel's err_to) when the block is, or has, a pinned image
    auto launch = [&](const StageView& v) {
        return qpsk_rx_launch(c, v.in(), F, v.bits(), v.valid(), trace ? v.trace() : nullptr,
                              soft ? v.soft() : nullptr, c->stream, nullptr, pin ? v.err() : nullptr);
    };
    // the results that came back through the pinned image: copied out to the
    // caller, with the error word that rx_data_kernel took beside them
    auto finish = [&] {
        memcpy(bits, h.bits(), cf * QK_NBITS);
        memcpy(valid, h.valid(), cf);
        if (trace) memcpy(trace, h.trace(), ntr);
        if (soft) memcpy(soft, h.soft(), nso);
        if (*h.err() != 0) c->stalled = true;
        return *h.err() != 0 ? QPSK_ESTALL : QPSK_OK;
    };
    if (pin && plain) memcpy(h.in(), in, nin);
    if (pin && plain && cf <= kZeroCopyCF) {
        // tiny calls: the kernels read the input from and write the outputs to
        // the pinned block directly (device-accessible host memory); the
        // per-frame latency is then two launches and one synchronisation, not
        // two copies besides (the kernels touch these few KB once)
        r = launch(h);
        if (r != QPSK_OK) return r;
        HCHECK(hipStreamSynchronize(c->stream));
        return finish();
    }
    if (plain) {
        HCHECK(hipMemcpyAsync(d.in(), pin ? (const void*)h.in() : (const void*)in, nin, hipMemcpyHostToDevice, c->stream));
    } else {
        r = feed(arg, d.in(), c->stream);
        if (r != QPSK_OK) return r;
    }
    // pinned: the error word is taken by rx_data_kernel (err_to) into the
    // staging block right after the valid flags, so bits, flags and error word
    // come back in one copy; pageable: qpsk_rx_sync() takes it
    r = launch(d);
    if (r != QPSK_OK) return r;
    if (!pin) {
        HCHECK(hipMemcpyAsync(bits, d.bits(), cf * QK_NBITS, hipMemcpyDeviceToHost, c->stream));
        HCHECK(hipMemcpyAsync(valid, d.valid(), cf, hipMemcpyDeviceToHost, c->stream));
        if (trace) HCHECK(hipMemcpyAsync(trace, d.trace(), ntr, hipMemcpyDeviceToHost, c->stream));
        if (soft) HCHECK(hipMemcpyAsync(soft, d.soft(), nso, hipMemcpyDeviceToHost, c->stream));
        return qpsk_rx_sync(c);
    }
    // (the error word was taken in one atomic exchange behind rx_kernel, as
    // qpsk_rx_sync does: a stream on this context, qpsk_stream_ctx, ORs its
    // slots' stalls into the same word from another HIP stream, and a read
    // followed by a separate clear could lose one merged in between)
    HCHECK(hipMemcpyAsync(h.bits(), d.bits(), g.err + sizeof(int) - g.bits, hipMemcpyDeviceToHost, c->stream));
    if (trace) HCHECK(hipMemcpyAsync(h.trace(), d.trace(), ntr, hipMemcpyDeviceToHost, c->stream));
    if (soft) HCHECK(hipMemcpyAsync(h.soft(), d.soft(), nso, hipMemcpyDeviceToHost, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    return finish();
}

extern "C" int qpsk_rx_batch(qpsk_ctx* c, const int16_t* in, int F, uint8_t* bits, uint8_t* valid,
                             int32_t* trace, float* soft) {
    return rx_batch_host(c, in, nullptr, nullptr, F, bits, valid, trace, soft);
}

int qpsk_rx_batch_fed(qpsk_ctx* c, qpsk_rx_feed_fn feed, void* arg, int F, uint8_t* bits, uint8_t* valid,
                      int32_t* trace, float* soft) {
    if (!feed) return QPSK_EINVAL;
    return rx_batch_host(c, nullptr, feed, arg, F, bits, valid, trace, soft);
}

int qpsk_rx_fmt_raw(qpsk_ctx* c, size_t bytes, char** p) {
    if (!c || !p) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    HCHECK(c->fmt.raw.reserve(bytes));
    *p = c->fmt.raw;
    return QPSK_OK;
}

int qpsk_rx_fmt_conv(qpsk_ctx* c, size_t n, int16_t** p) {
    if (!c || !p) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    if (n > c->fmt.conv.cap()) {
        HCHECK(hipDeviceSynchronize());   // an earlier call may still read the block
        HCHECK(c->fmt.conv.reserve(n));
    }
    *p = c->fmt.conv;
    return QPSK_OK;
}

int qpsk_rx_rec_bufs(qpsk_ctx* c, size_t cf, bool trace, bool soft, size_t work_bytes, size_t out_bytes,
                     qpsk_rec_bufs* b) {
    if (!c || !b) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    RecBufs& r = c->rec;
    const size_t ntr = trace ? cf * 4 : 0, nso = soft ? cf * QK_NDSYM * 2 : 0;
    if (cf * QK_NBITS > r.bits.cap() || cf > r.valid.cap() || ntr > r.trace.cap() || nso > r.soft.cap() ||
        work_bytes > r.work.cap() || out_bytes > r.out.cap())
        HCHECK(hipDeviceSynchronize());   // an earlier call may still use the buffers
    HCHECK(r.bits.reserve(cf * QK_NBITS));
    HCHECK(r.valid.reserve(cf));
    HCHECK(r.trace.reserve(ntr));
    HCHECK(r.soft.reserve(nso));
    HCHECK(r.work.reserve(work_bytes));
    HCHECK(r.out.reserve(out_bytes));
    *b = qpsk_rec_bufs{r.bits, r.valid, trace ? r.trace.get() : nullptr, soft ? r.soft.get() : nullptr, r.work, r.out};
    return QPSK_OK;
}

hipStream_t qpsk_rx_stream(qpsk_ctx* c) { return c ? (hipStream_t)c->stream : nullptr; }

extern "C" const char* qpsk_strerror(int err) {
    switch (err) {
        case QPSK_OK: return "success";
        case QPSK_EINVAL: return "invalid argument";
        case QPSK_ENOMEM: return "out of memory";
        case QPSK_ENODEV: return "no such HIP device";
        case QPSK_EBUSY: return "every stream slot is in flight (retrieve first)";
        case QPSK_ESTALL: return "a device-side progress wait exceeded its bound; the call's outputs are undefined";
        default: break;
    }
    if (err <= QPSK_EHIP) return hipGetErrorString((hipError_t)(QPSK_EHIP - err));
    return "unknown error";
}
