// qpsk_rx_host.hip -- the host side of the receive path (include/qpsk_batch.h,
// qpsk_rx_internal.h): the context, its creation, reset and state snapshots,
// the choice of a kernel shape, a call's bookkeeping around its launches, and
// the host-memory entry point with its staging.  No device code: the kernels
// and their launches are qpsk_rx.hip's (qpsk_rx_launch_kernels), and all the
// two files share is qpsk_rx_shared.h, so an edit here neither rebuilds the
// kernels nor changes their hash (qpsk_kernel_hash()).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "qpsk_batch.h"
#include "qpsk_consts.h"
#include "qpsk_fft.h"
#include "qpsk_fft_tables.h"
#include "qpsk_rx_internal.h"
#include "qpsk_rx_shared.h"

#pragma clang fp contract(off)

static float bits2f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct qpsk_ctx {
    int device = 0, nch = 0, ngroup = 0;
    int mode = QPSK_MODE_REFERENCE;   // receiver semantics, fixed at creation
    float* d_fft = nullptr;           // FFT-hunt tables (kFftHT floats), QPSK_MODE_FFT_HUNT
    uint64_t frames = 0;
    hipStream_t stream = nullptr;
    float2* d_ptab = nullptr;
    unsigned long long* d_ks = nullptr;
    int16_t* d_hist = nullptr;
    float2* d_win[2] = {nullptr, nullptr};
    int* d_mi[2] = {nullptr, nullptr};
    int* d_rt[2] = {nullptr, nullptr};
    // data-symbol jobs of valid frames (rx_kernel -> rx_data_kernel)
    float4* d_jobs = nullptr;
    size_t jobs_cap = 0;           // jobs (one per channel-frame of the largest call)
    unsigned* d_njobs = nullptr;   // [2] counters, alternating by call
    uint64_t calls = 0;
    // staging for the host-memory entry point (qpsk_rx_batch): one device block
    // [in | bits | valid | trace | soft] (stage_grow) and, for small calls, a
    // pinned host image of it, so a call is one H2D and one D2H of pinned
    // memory (the per-frame drop-in qpsk_rx_frame is such a call)
    char* s_dev = nullptr;
    char* s_pin = nullptr;          // pinned, same layout; only while small
    size_t s_frames = 0;
    // kernel-span accounting: events before rx_kernel, between the kernels, after
    // rx_data_kernel
    static constexpr int kEv = 64;
    hipEvent_t ev[kEv][3] = {};
    int ev_frames[kEv] = {};
    int ev_n = 0;
    bool timing = false;
    // roles + front issue priority + front stagger (0 since round 5; 12 x 512
    // cycles was -0.7% in round 1,
    // profiles/r01_stagger_ab.txt); QPSK_ABLATE (profiling), QPSK_FORCE_EXACT /
    // QPSK_DEBUG_STALL (tests)
    int roles = roles_with_stagger(roles_with_prio(kRoleBack | kRoleFront, kPrioFront), kStagger);
    int ncu = 256;              // compute units of the device
    int shape = -1;             // Shape::Kind forced by QPSK_SHAPE (A/B runs); -1: by batch size
    int width = 0;              // dual-chain group width forced by QPSK_WIDTH; 0: by batch size
    int prio = -1;              // issue priority forced by QPSK_PRIO (a RolePrio); -1: by shape
    bool headpass = false;      // QPSK_HEADPASS: the FIR-head pre-pass (reference mode only)
    float2* d_heads = nullptr;  // its outputs, [nch][F][102] for the largest call
    size_t heads_cap = 0;       // channel-frames d_heads holds
    int* d_err = nullptr;       // [0] device error word (kErrStall), taken by qpsk_rx_sync;
                                // [1] the value it took
    hipEvent_t done = nullptr;  // recorded after the latest call's kernels, on its stream
    bool called = false;        // `done` has been recorded
    float pend_ms[2] = {0.0f, 0.0f};
    int pend_frames = 0;
    uint64_t epoch = 0;         // qpsk_rx_reset() count (qpsk_rx_epoch)
    int stall_calls = -1;       // QPSK_DEBUG_STALL=first: the stall only in the first launch; -1: every call
    int short_block = 0;        // QPSK_DEBUG_BLOCK (tests): rx_kernel launched one wave short
    uint64_t launches = 0;      // calls launched over the context's life (qpsk_rx_reset keeps it)
    const qpsk_stream* owner = nullptr;   // the stream this context belongs to, if any
    // a call reported QPSK_ESTALL since the last reset: the per-channel state
    // is undefined, and qpsk_rx_state_save refuses to export it
    bool stalled = false;
    // qpsk_rx_state_load of a channel range into a fresh context (frame 0) from
    // a snapshot at frame G != 0: the context takes frame index G, so every
    // channel must be loaded before it may receive (asm_left channels to go;
    // asm_cover marks the loaded ones)
    std::vector<uint8_t> asm_cover;
    int asm_left = 0;
};

extern "C" int qpsk_rx_timing_split(qpsk_ctx* c, float* ms_rx, float* ms_data, int* frames);

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

// state arrays cover whole workgroups of the largest shape (kMaxGroups groups)
static size_t nslot(const qpsk_ctx* c) {
    return (size_t)((c->ngroup + kMaxGroups - 1) / kMaxGroups) * kMaxGroups * QK_GROUP;
}

static int ctx_alloc(qpsk_ctx* c) {
    HCHECK(hipMalloc(&c->d_ptab, sizeof(float2) * QK_FRAME));
    HCHECK(hipMalloc(&c->d_ks, sizeof(unsigned long long) * QK_KS_FRAMES));
    HCHECK(hipMalloc(&c->d_hist, sizeof(int16_t) * nslot(c) * 2 * QK_FRAME));
    HCHECK(hipMalloc(&c->d_njobs, sizeof(unsigned) * 2));
    HCHECK(hipMalloc(&c->d_err, 2 * sizeof(int)));
    HCHECK(hipEventCreateWithFlags(&c->done, hipEventDisableTiming));
    for (int p = 0; p < 2; p++) {
        HCHECK(hipMalloc(&c->d_win[p], sizeof(float2) * nslot(c) * kWinStride));
        HCHECK(hipMalloc(&c->d_mi[p], sizeof(int) * nslot(c)));
        HCHECK(hipMalloc(&c->d_rt[p], sizeof(int) * nslot(c)));
    }
    return QPSK_OK;
}

extern "C" int qpsk_rx_reset(qpsk_ctx* c) {
    if (!c) return QPSK_EINVAL;
    // a stream's chunks in flight run on the state cleared here (and one that
    // stalled must keep its epoch): refuse until the stream is drained
    if (c->owner && qpsk_stream_pending(c->owner) > 0) return QPSK_EBUSY;
    HCHECK(hipSetDevice(c->device));
    // calls in flight on other streams read and write the state cleared here
    if (c->called) HCHECK(hipEventSynchronize(c->done));
    const size_t ns = nslot(c);
    HCHECK(hipMemsetAsync(c->d_hist, 0, sizeof(int16_t) * ns * 2 * QK_FRAME, c->stream));
    HCHECK(hipMemsetAsync(c->d_njobs, 0, sizeof(unsigned) * 2, c->stream));
    HCHECK(hipMemsetAsync(c->d_err, 0, 2 * sizeof(int), c->stream));
    for (int p = 0; p < 2; p++) {
        HCHECK(hipMemsetAsync(c->d_win[p], 0, sizeof(float2) * ns * kWinStride, c->stream));
        HCHECK(hipMemsetAsync(c->d_mi[p], 0, sizeof(int) * ns, c->stream));
    }
    int* rt0 = (int*)malloc(sizeof(int) * ns);
    if (!rt0) return QPSK_ENOMEM;
    for (size_t i = 0; i < ns; i++) rt0[i] = QK_RT0;
    hipError_t e = hipMemcpy(c->d_rt[0], rt0, sizeof(int) * ns, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_rt[1], rt0, sizeof(int) * ns, hipMemcpyHostToDevice);
    free(rt0);
    HCHECK(e);
    HCHECK(hipStreamSynchronize(c->stream));
    c->frames = 0;
    c->calls = 0;
    c->epoch++;
    c->stalled = false;
    c->asm_cover.clear();
    c->asm_left = 0;
    return QPSK_OK;
}

int* qpsk_rx_err_word(qpsk_ctx* c) { return c ? c->d_err : nullptr; }
void qpsk_rx_set_owner(qpsk_ctx* c, const qpsk_stream* s) { if (c) c->owner = s; }
uint64_t qpsk_rx_epoch(const qpsk_ctx* c) { return c ? c->epoch : 0; }
void qpsk_rx_mark_stalled(qpsk_ctx* c, uint64_t epoch) {
    if (c && epoch == c->epoch) c->stalled = true;
}

static void ctx_free(qpsk_ctx* c) {
    for (int i = 0; i < qpsk_ctx::kEv; i++)
        for (int j = 0; j < 3; j++)
            if (c->ev[i][j]) (void)hipEventDestroy(c->ev[i][j]);
    (void)hipFree(c->d_ptab);
    (void)hipFree(c->d_err);
    if (c->done) (void)hipEventDestroy(c->done);
    (void)hipFree(c->d_jobs);
    (void)hipFree(c->d_njobs);
    (void)hipFree(c->d_ks);
    (void)hipFree(c->d_hist);
    (void)hipFree(c->d_fft);
    (void)hipFree(c->d_heads);
    for (int p = 0; p < 2; p++) {
        (void)hipFree(c->d_win[p]);
        (void)hipFree(c->d_mi[p]);
        (void)hipFree(c->d_rt[p]);
    }
    (void)hipFree(c->s_dev);
    (void)hipHostFree(c->s_pin);
    if (c->stream) (void)hipStreamDestroy(c->stream);
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
    HCHECK(hipMalloc(&c->d_fft, sizeof tab));
    HCHECK(hipMemcpy(c->d_fft, tab, sizeof tab, hipMemcpyHostToDevice));
    return QPSK_OK;
}

// The environment's test, profiling and A/B settings of a new context (c->mode
// is set)
static void ctx_read_env(qpsk_ctx* c) {
    if (const char* ab = getenv("QPSK_ABLATE")) {   // timing experiments; output invalid
        if (!strcmp(ab, "front")) c->roles = roles_with_served(c->roles, kRoleFront);
        else if (!strcmp(ab, "back")) c->roles = roles_with_served(c->roles, kRoleBack);
        else if (!strcmp(ab, "frontidle")) c->roles |= kFrontIdle;
    }
    if (getenv("QPSK_FORCE_EXACT")) c->roles |= kForceExact;   // tests: exact-division path
    if (const char* ds = getenv("QPSK_DEBUG_STALL")) {          // tests: the QPSK_ESTALL path
        c->roles |= kDebugStall;
        if (!strcmp(ds, "first")) c->stall_calls = 1;           // only the context's first call
    }
    if (getenv("QPSK_DEBUG_BLOCK")) c->short_block = 64;          // tests: rx_kernel's launch-shape guard
    if (const char* w = getenv("QPSK_WIDTH")) {
        const int v = atoi(w);
        c->width = (v == 16 || v == 32 || v == 64) ? v : 0;
    }
    if (const char* hv = getenv("QPSK_HEADPASS")) c->headpass = atoi(hv) != 0 && c->mode == QPSK_MODE_REFERENCE;
    if (const char* sv = getenv("QPSK_STAGGER")) {   // A/B: the 4x2 fronts' stagger, 512-cycle units
        const int v = atoi(sv);
        if (v >= 0 && v < 256) c->roles = roles_with_stagger(c->roles, v);
    }
    if (const char* pv = getenv("QPSK_PRIO"))
        c->prio = !strcmp(pv, "none") ? kPrioNone : !strcmp(pv, "front") ? kPrioFront : !strcmp(pv, "back") ? kPrioBack : -1;
    if (const char* sh = getenv("QPSK_SHAPE")) {
        c->shape = !strcmp(sh, "4x2") ? Shape::k4x2
                 : !strcmp(sh, "2x4d") ? Shape::k2x4d
                 : !strcmp(sh, "1x8") ? Shape::k1x8d64 : -1;
    }
}

extern "C" qpsk_ctx* qpsk_rx_create(int device, int nch, int* err) {
    return qpsk_rx_create_mode(device, nch, QPSK_MODE_REFERENCE, err);
}

extern "C" qpsk_ctx* qpsk_rx_create_mode(int device, int nch, int mode, int* err) {
    int dummy;
    if (!err) err = &dummy;
    if (nch < 1 || mode < 0 || mode > (QPSK_MODE_DEC752 | QPSK_MODE_FFT_HUNT)) {
        *err = QPSK_EINVAL;
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        *err = QPSK_ENODEV;
        return nullptr;
    }
    qpsk_ctx* c = new (std::nothrow) qpsk_ctx();
    if (!c) { *err = QPSK_ENOMEM; return nullptr; }
    c->device = device;
    c->nch = nch;
    c->mode = mode;
    c->ngroup = (nch + QK_GROUP - 1) / QK_GROUP;
    ctx_read_env(c);
    int r = herr(hipSetDevice(device));
    if (r == QPSK_OK) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
            n > 0)
            c->ncu = n;
    }
    if (r == QPSK_OK) r = herr(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (r == QPSK_OK) r = ctx_alloc(c);
    if (r == QPSK_OK) {
        const RxTables& t = rx_tables();
        r = herr(hipMemcpy(c->d_ptab, t.ptab, sizeof t.ptab, hipMemcpyHostToDevice));
        if (r == QPSK_OK) r = herr(hipMemcpy(c->d_ks, t.ksf, sizeof t.ksf, hipMemcpyHostToDevice));
    }
    if (r == QPSK_OK && (mode & QPSK_MODE_FFT_HUNT)) r = fft_hunt_tables(c);
    if (r == QPSK_OK) r = qpsk_rx_reset(c);
    if (r != QPSK_OK) {
        ctx_free(c);
        delete c;
        *err = r;
        return nullptr;
    }
    *err = QPSK_OK;
    return c;
}

// ---------------------------------------------------------------- state snapshots
// qpsk_batch.h qpsk_rx_state_*: the per-channel state the kernels carry from
// one call to the next, for the context's frame index G (the next frame):
// the history int16 [2][1880] (frames G-2, G-1: carry_history), window G's
// row float2 [168] with mi_G, and rt_G, the last three in the arrays of
// parity G & 1 (rx_kernel reads mi_of / rt_of / win_of (g0) at a call's start
// and writes parity g0 + F at its end).  Layout: a 64-byte header, then the
// four fields channel-major, each as one contiguous block.
namespace {
constexpr char kStateMagic[8] = {'Q', 'P', 'S', 'K', 'S', 'T', 'A', '1'};
struct StateHdr {
    char magic[8];
    uint32_t version, hdr_bytes;
    int32_t mode, n;
    uint64_t frame;
    uint32_t hist_bytes, win_bytes;   // per channel
    uint8_t pad[24];
};
static_assert(sizeof(StateHdr) == 64, "state header");
constexpr size_t kHistB = sizeof(int16_t) * 2 * QK_FRAME, kWinB = sizeof(float2) * kWinStride;
constexpr size_t kChanB = kHistB + kWinB + 2 * sizeof(int);
constexpr int kWinObs = QK_NPRE + QK_NDSYM + 5;   // slots 0..163 = dec[mi-1 .. mi+162]
static_assert(kWinObs == 164 && kWinObs <= kWinStride, "window slots");
}  // namespace

extern "C" size_t qpsk_rx_state_size(int n) { return n < 1 ? 0 : sizeof(StateHdr) + (size_t)n * kChanB; }

// the checks both directions share; waits for the context's calls in flight
static int state_begin(qpsk_ctx* c, int c0, int n, const void* buf, size_t size) {
    if (!c || !buf || n < 1 || c0 < 0 || c0 > c->nch - n || size < qpsk_rx_state_size(n)) return QPSK_EINVAL;
    if (c->owner && qpsk_stream_pending(c->owner) > 0) return QPSK_EBUSY;
    HCHECK(hipSetDevice(c->device));
    if (c->called) HCHECK(hipEventSynchronize(c->done));
    return QPSK_OK;
}

extern "C" int qpsk_rx_state_save(qpsk_ctx* c, int c0, int n, void* buf, size_t size) {
    int r = state_begin(c, c0, n, buf, size);
    if (r != QPSK_OK) return r;
    // channels still to be loaded (qpsk_rx_state_load) hold no state of frame G
    if (c->asm_left > 0) return QPSK_EINVAL;
    // a stall (reported, or still in the error word: peeked, not taken, so
    // qpsk_rx_sync still reports it) leaves the state undefined
    if (!c->stalled) {
        int e = 0;
        HCHECK(hipMemcpyAsync(&e, c->d_err, sizeof e, hipMemcpyDeviceToHost, c->stream));
        HCHECK(hipStreamSynchronize(c->stream));
        if (e != 0) return QPSK_ESTALL;
    }
    if (c->stalled) return QPSK_ESTALL;
    StateHdr h{};
    memcpy(h.magic, kStateMagic, sizeof h.magic);
    h.version = 1;
    h.hdr_bytes = sizeof h;
    h.mode = c->mode;
    h.n = n;
    h.frame = c->frames;
    h.hist_bytes = (uint32_t)kHistB;
    h.win_bytes = (uint32_t)kWinB;
    char* o = static_cast<char*>(buf);
    memcpy(o, &h, sizeof h);
    o += sizeof h;
    const int p = (int)(c->frames & 1u);
    const size_t nn = (size_t)n;
    HCHECK(hipMemcpyAsync(o, c->d_hist + (size_t)c0 * 2 * QK_FRAME, nn * kHistB, hipMemcpyDeviceToHost, c->stream));
    o += nn * kHistB;
    char* w = o;
    HCHECK(hipMemcpyAsync(o, c->d_win[p] + (size_t)c0 * kWinStride, nn * kWinB, hipMemcpyDeviceToHost, c->stream));
    o += nn * kWinB;
    HCHECK(hipMemcpyAsync(o, c->d_mi[p] + c0, nn * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    o += nn * sizeof(int);
    HCHECK(hipMemcpyAsync(o, c->d_rt[p] + c0, nn * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    // window slots past dec[mi+162] (the last data symbol's taps, SURVEY.md
    // A.6) are never read; the fronts leave whatever their dec buffer held
    // there (the split FIR skips dec[255..289] when mi < 93).  Zeroed, so a
    // snapshot is a function of the channel's state alone.
    for (size_t i = 0; i < nn; i++)
        memset(w + i * kWinB + kWinObs * sizeof(float2), 0, (kWinStride - kWinObs) * sizeof(float2));
    return QPSK_OK;
}

extern "C" int qpsk_rx_state_load(qpsk_ctx* c, int c0, int n, const void* buf, size_t size) {
    int r = state_begin(c, c0, n, buf, size);
    if (r != QPSK_OK) return r;
    StateHdr h;
    memcpy(&h, buf, sizeof h);
    if (memcmp(h.magic, kStateMagic, sizeof h.magic) != 0 || h.version != 1 || h.hdr_bytes != sizeof h ||
        h.n != n || h.mode != c->mode || h.hist_bytes != kHistB || h.win_bytes != kWinB)
        return QPSK_EINVAL;
    if (c->frames != h.frame && c->frames != 0) return QPSK_EINVAL;   // one frame index per context
    // a channel range at frame G != 0 into a fresh context moves the context's
    // frame index to G for every channel: the others must be loaded too
    // (from this or other snapshots at G) before the context may receive
    const bool assemble = c->asm_left > 0 || (c->frames == 0 && h.frame != 0 && n < c->nch);
    const char* o = static_cast<const char*>(buf) + sizeof h;
    const int p = (int)(h.frame & 1u);
    const size_t nn = (size_t)n;
    HCHECK(hipMemcpyAsync(c->d_hist + (size_t)c0 * 2 * QK_FRAME, o, nn * kHistB, hipMemcpyHostToDevice, c->stream));
    o += nn * kHistB;
    HCHECK(hipMemcpyAsync(c->d_win[p] + (size_t)c0 * kWinStride, o, nn * kWinB, hipMemcpyHostToDevice, c->stream));
    o += nn * kWinB;
    HCHECK(hipMemcpyAsync(c->d_mi[p] + c0, o, nn * sizeof(int), hipMemcpyHostToDevice, c->stream));
    o += nn * sizeof(int);
    HCHECK(hipMemcpyAsync(c->d_rt[p] + c0, o, nn * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    if (assemble) {
        if (c->asm_cover.empty()) {
            c->asm_cover.assign((size_t)c->nch, 0);
            c->asm_left = c->nch;
        }
        for (int i = c0; i < c0 + n; i++)
            if (!c->asm_cover[(size_t)i]) {
                c->asm_cover[(size_t)i] = 1;
                c->asm_left--;
            }
        if (c->asm_left == 0) c->asm_cover.clear();
    }
    c->frames = h.frame;
    return QPSK_OK;
}

extern "C" void qpsk_rx_destroy(qpsk_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    ctx_free(c);
    delete c;
}

extern "C" int qpsk_rx_channels(const qpsk_ctx* c) { return c ? c->nch : 0; }
extern "C" int qpsk_rx_mode(const qpsk_ctx* c) { return c ? c->mode : QPSK_EINVAL; }
extern "C" uint64_t qpsk_rx_frames(const qpsk_ctx* c) { return c ? c->frames : 0; }

// The rx_kernel instantiation for a call (DESIGN.md "Kernels"):
//   > 2 groups per CU (C3's 65,536 channels): 4x2, one back wave per group;
//   2 groups per CU: 2x4 with dual-chain backs (11% faster at 32,768 channels,
//     profiles/r01_dual_ab.txt);
//   1 group per CU: 1x8 dual-chain, at the narrowest group width (16/32/64
//     channels) that still fits the batch in one wave of workgroups: quad
//     backs at W = 16 / 32, lane backs at W = 64 (quad backs there need 16
//     waves, whose 128-VGPR budget spills the front: profiles/r02_quad_ab.txt)
//     with back priority and 2 channels moved off each front wave that
//     shares a SIMD with a back wave (-3%, profiles/r01_split_ab.txt).
// QPSK_SHAPE (4x2 | 2x4d | 1x8) and QPSK_WIDTH force a shape for tests and A/B
// runs.  The result is a Shape::Kind; launch_shape maps it to the kernel whose
// parameters ShapeOf gives that kind.  Measured and dropped (records in
// profiles/, DESIGN.md "Measured and not kept"): 4x1d, 2x4 and 1x8 with single
// back waves, the early-terminated flow kernel (r01_flow_ab.txt), lane backs at
// W = 16 / 32, one front per SIMD (1x4) and the 4x3 C3 shape (round 5 removed
// the last three from the build).
static Shape pick_shape(const qpsk_ctx* c) {
    Shape sh{c->shape, c->roles};
    if (sh.kind < 0)
        sh.kind = c->ngroup <= c->ncu ? Shape::k1x8d64 : c->ngroup <= 2 * c->ncu ? Shape::k2x4d
                                                                                  : Shape::k4x2;
    if (sh.kind == Shape::k1x8d64) {
        const int W = c->width > 0 ? c->width
                    : (size_t)c->nch <= (size_t)16 * c->ncu ? 16
                    : (size_t)c->nch <= (size_t)32 * c->ncu ? 32 : 64;
        if (W == 16) sh.kind = Shape::k1x8q16;
        else if (W == 32) sh.kind = Shape::k1x8q32;
        else sh.roles = roles_with_split(roles_with_prio(sh.roles, kPrioBack), 2);
    }
    if (c->prio >= 0) sh.roles = roles_with_prio(sh.roles, c->prio);
    return sh;
}

// A call's launches (qpsk_rx_batch_device) and the bookkeeping around them; the
// launches themselves are qpsk_rx.hip's (qpsk_rx_launch_kernels).  d_err: the device error word
// the call's progress waits report to: the context's (qpsk_rx_sync takes it),
// or a caller's own (qpsk_stream.hip: one per stream slot, so a stall is
// reported with the chunk it belongs to).
int qpsk_rx_launch(qpsk_ctx* c, const int16_t* d_in, int F, uint8_t* d_bits, uint8_t* d_valid,
                   int32_t* d_trace, float* d_soft, hipStream_t s, int* d_err, int* err_to) {
    if (!c || F < 0 || (F > 0 && (!d_in || !d_bits || !d_valid))) return QPSK_EINVAL;
    if (c->asm_left > 0) return QPSK_EINVAL;   // channels not yet loaded (qpsk_rx_state_load)
    if (F == 0) return QPSK_OK;
    if ((reinterpret_cast<uintptr_t>(d_in) & 15u) != 0) return QPSK_EINVAL;  // int4 loads
    HCHECK(hipSetDevice(c->device));
    if (!d_err) d_err = c->d_err;
    const size_t need = (size_t)c->nch * (size_t)F;   // every frame valid, at most
    // job slots are addressed with 32-bit byte offsets (slot * 16); 2^28 channel-
    // frames would be 1 TB of input, beyond any device's memory
    if (need >= ((size_t)1 << 28)) return QPSK_EINVAL;
    if (need > c->jobs_cap) {
        HCHECK(hipDeviceSynchronize());   // an earlier call may still use the queue
        (void)hipFree(c->d_jobs);
        c->d_jobs = nullptr;
        c->jobs_cap = 0;
        HCHECK(hipMalloc(&c->d_jobs, sizeof(float4) * kJobF4 * need));
        c->jobs_cap = need;
    }
    const bool hp = c->headpass;
    if (hp && need > c->heads_cap) {
        HCHECK(hipDeviceSynchronize());   // an earlier call may still read the heads
        (void)hipFree(c->d_heads);
        c->d_heads = nullptr;
        c->heads_cap = 0;
        HCHECK(hipMalloc(&c->d_heads, sizeof(float2) * kHeadOut * need));
        c->heads_cap = need;
    }
    int slot = -1;
    if (c->timing) {
        if (c->ev_n == qpsk_ctx::kEv) {   // pool full: fold pending spans into the totals
            float ms[2];
            int nf;
            int r = qpsk_rx_timing_split(c, &ms[0], &ms[1], &nf);
            if (r != QPSK_OK) return r;
            c->pend_ms[0] += ms[0];
            c->pend_ms[1] += ms[1];
            c->pend_frames += nf;
        }
        slot = c->ev_n++;
        for (int j = 0; j < 3; j++)
            if (!c->ev[slot][j]) HCHECK(hipEventCreate(&c->ev[slot][j]));
        HCHECK(hipEventRecord(c->ev[slot][0], s));
        c->ev_frames[slot] = F;
    }
    const int parity = (int)(c->calls & 1u);
    // the kernels use the frame index only as g & 1 (mixer sign, state parity)
    // and g % QK_KS_FRAMES (descrambler word): its residue mod 2 * 1057 is
    // right for any 64-bit c->frames, and g0 + F stays far below 2^32
    const unsigned g0 = (unsigned)(c->frames % (uint64_t)(2 * QK_KS_FRAMES));
    Shape sh = pick_shape(c);
    if (c->stall_calls >= 0 && c->launches >= (uint64_t)c->stall_calls) sh.roles &= ~kDebugStall;
    RxLaunch l{};
    l.s = s;
    l.kind = sh.kind;
    l.mode = c->mode;
    l.hp = hp;
    l.short_block = c->short_block;
    l.in = d_in;
    l.hist = c->d_hist;
    l.ptab = c->d_ptab;
    l.ks = c->d_ks;
    for (int p = 0; p < 2; p++) {
        l.win[p] = c->d_win[p];
        l.mi[p] = c->d_mi[p];
        l.rt[p] = c->d_rt[p];
    }
    l.bits = d_bits;
    l.valid = d_valid;
    l.trace = d_trace;
    l.soft = d_soft;
    l.jobs = c->d_jobs;
    l.jobs_cap = c->jobs_cap;
    l.njobs = c->d_njobs;
    l.parity = parity;
    l.nch = c->nch;
    l.F = F;
    l.g0 = g0;
    l.roles = sh.roles;
    l.fft_tab = c->d_fft;
    l.heads = c->d_heads;
    l.err = d_err;
    l.ctx_err = c->d_err;
    l.err_to = err_to;
    l.ev_mid = slot >= 0 ? c->ev[slot][1] : nullptr;
    l.ev_end = slot >= 0 ? c->ev[slot][2] : nullptr;
    const int lr = qpsk_rx_launch_kernels(l);
    if (lr != QPSK_OK) return lr;
    HCHECK(hipEventRecord(c->done, s));
    c->called = true;
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
    c->timing = on != 0;
    return QPSK_OK;
}

extern "C" int qpsk_rx_timing_split(qpsk_ctx* c, float* ms_rx, float* ms_data, int* frames) {
    if (!c || !ms_rx || !ms_data || !frames) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    float tot[2] = {c->pend_ms[0], c->pend_ms[1]};
    int nf = c->pend_frames;
    for (int i = 0; i < c->ev_n; i++) {
        HCHECK(hipEventSynchronize(c->ev[i][2]));
        for (int k = 0; k < 2; k++) {
            float t = 0.0f;
            HCHECK(hipEventElapsedTime(&t, c->ev[i][k], c->ev[i][k + 1]));
            tot[k] += t;
        }
        nf += c->ev_frames[i];
    }
    c->ev_n = 0;
    c->pend_ms[0] = c->pend_ms[1] = 0.0f;
    c->pend_frames = 0;
    *ms_rx = tot[0];
    *ms_data = tot[1];
    *frames = nf;
    return QPSK_OK;
}

extern "C" int qpsk_rx_timing_collect(qpsk_ctx* c, float* ms, int* frames) {
    if (!ms) return QPSK_EINVAL;
    float a = 0.0f, b = 0.0f;
    const int r = qpsk_rx_timing_split(c, &a, &b, frames);
    if (r == QPSK_OK) *ms = a + b;
    return r;
}

// byte offsets of the staging block for cf channel-frames
struct Stage {
    size_t in, bits, valid, err, trace, soft, end;
};
static Stage stage_of(size_t cf) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    Stage g;
    g.in = 0;
    g.bits = up(sizeof(int16_t) * cf * QK_FRAME);
    g.valid = g.bits + cf * QK_NBITS;   // bits, valid and the taken error word
    g.err = (g.valid + cf + 3) & ~(size_t)3;   // adjacent: one D2H
    g.trace = up(g.err + sizeof(int));
    g.soft = up(g.trace + sizeof(int32_t) * cf * 4);
    g.end = up(g.soft + sizeof(float) * cf * QK_NDSYM * 2);
    return g;
}
// calls up to this many input bytes stage through pinned memory
constexpr size_t kPinnedStage = (size_t)8 << 20;
// calls up to this many channel-frames (the drop-in qpsk_rx_frame: one) run
// their kernels on the pinned block itself, no copies
constexpr size_t kZeroCopyCF = 64;

static int stage_grow(qpsk_ctx* c, size_t F) {
    if (F <= c->s_frames) return QPSK_OK;
    (void)hipFree(c->s_dev);
    (void)hipHostFree(c->s_pin);
    c->s_dev = nullptr;
    c->s_pin = nullptr;
    c->s_frames = 0;
    const size_t cf = (size_t)c->nch * F;
    const Stage g = stage_of(cf);
    HCHECK(hipMalloc(&c->s_dev, g.end));
    if (g.bits <= kPinnedStage) HCHECK(hipHostMalloc((void**)&c->s_pin, g.end, hipHostMallocDefault));
    c->s_frames = F;
    return QPSK_OK;
}

// The results of a call that came back through the pinned block h: copied out
// to the caller, with the error word that rx_data_kernel took beside them
static int stage_finish(qpsk_ctx* c, const char* h, const Stage& g, size_t cf, uint8_t* bits,
                        uint8_t* valid, int32_t* trace, float* soft) {
    memcpy(bits, h + g.bits, cf * QK_NBITS);
    memcpy(valid, h + g.valid, cf);
    if (trace) memcpy(trace, h + g.trace, sizeof(int32_t) * cf * 4);
    if (soft) memcpy(soft, h + g.soft, sizeof(float) * cf * QK_NDSYM * 2);
    int e;
    memcpy(&e, h + g.err, sizeof e);
    if (e != 0) c->stalled = true;
    return e != 0 ? QPSK_ESTALL : QPSK_OK;
}

extern "C" int qpsk_rx_batch(qpsk_ctx* c, const int16_t* in, int F, uint8_t* bits, uint8_t* valid,
                             int32_t* trace, float* soft) {
    if (!c || F < 0 || (F > 0 && (!in || !bits || !valid))) return QPSK_EINVAL;
    if (c->asm_left > 0) return QPSK_EINVAL;   // channels not yet loaded (qpsk_rx_state_load)
    if (F == 0) return QPSK_OK;
    HCHECK(hipSetDevice(c->device));
    int r = stage_grow(c, (size_t)F);
    if (r != QPSK_OK) return r;
    const size_t cf = (size_t)c->nch * F;
    const Stage g = stage_of(cf);
    char* d = c->s_dev;
    const bool pin = c->s_pin && g.bits <= kPinnedStage;
    // pinned: the caller's input is copied into the pinned image (a host memcpy)
    // and moves in one DMA, outputs come back in one; pageable otherwise
    char* h = pin ? c->s_pin : nullptr;
    const size_t nin = sizeof(int16_t) * cf * QK_FRAME;
    const size_t ntr = sizeof(int32_t) * cf * 4, nso = sizeof(float) * cf * QK_NDSYM * 2;
    if (pin && cf <= kZeroCopyCF) {
        // tiny calls: the kernels read the input from and write the outputs to
        // the pinned block directly (device-accessible host memory); the
        // per-frame latency is then two launches and one synchronisation, not
        // two copies besides (the kernels touch these few KB once)
        memcpy(h + g.in, in, nin);
        // the error word comes back with the outputs (rx_data_kernel's err_to)
        r = qpsk_rx_launch(c, reinterpret_cast<int16_t*>(h + g.in), F,
                           reinterpret_cast<uint8_t*>(h + g.bits), reinterpret_cast<uint8_t*>(h + g.valid),
                           trace ? reinterpret_cast<int32_t*>(h + g.trace) : nullptr,
                           soft ? reinterpret_cast<float*>(h + g.soft) : nullptr, c->stream, nullptr,
                           reinterpret_cast<int*>(h + g.err));
        if (r != QPSK_OK) return r;
        HCHECK(hipStreamSynchronize(c->stream));
        return stage_finish(c, h, g, cf, bits, valid, trace, soft);
    }
    if (pin) memcpy(h + g.in, in, nin);
    HCHECK(hipMemcpyAsync(d + g.in, pin ? (const void*)(h + g.in) : (const void*)in, nin,
                          hipMemcpyHostToDevice, c->stream));
    // pinned: the error word is taken by rx_data_kernel (err_to) into the
    // staging block right after the valid flags, so bits, flags and error word
    // come back in one copy; pageable: qpsk_rx_sync() takes it
    r = qpsk_rx_launch(c, reinterpret_cast<int16_t*>(d + g.in), F,
                       reinterpret_cast<uint8_t*>(d + g.bits), reinterpret_cast<uint8_t*>(d + g.valid),
                       trace ? reinterpret_cast<int32_t*>(d + g.trace) : nullptr,
                       soft ? reinterpret_cast<float*>(d + g.soft) : nullptr, c->stream, nullptr,
                       pin ? reinterpret_cast<int*>(d + g.err) : nullptr);
    if (r != QPSK_OK) return r;
    if (!pin) {
        HCHECK(hipMemcpyAsync(bits, d + g.bits, cf * QK_NBITS, hipMemcpyDeviceToHost, c->stream));
        HCHECK(hipMemcpyAsync(valid, d + g.valid, cf, hipMemcpyDeviceToHost, c->stream));
        if (trace) HCHECK(hipMemcpyAsync(trace, d + g.trace, ntr, hipMemcpyDeviceToHost, c->stream));
        if (soft) HCHECK(hipMemcpyAsync(soft, d + g.soft, nso, hipMemcpyDeviceToHost, c->stream));
        return qpsk_rx_sync(c);
    }
    // (the error word was taken in one atomic exchange behind rx_kernel, as
    // qpsk_rx_sync does: a stream on this context, qpsk_stream_ctx, ORs its
    // slots' stalls into the same word from another HIP stream, and a read
    // followed by a separate clear could lose one merged in between)
    HCHECK(hipMemcpyAsync(h + g.bits, d + g.bits, g.err + sizeof(int) - g.bits, hipMemcpyDeviceToHost, c->stream));
    if (trace) HCHECK(hipMemcpyAsync(h + g.trace, d + g.trace, ntr, hipMemcpyDeviceToHost, c->stream));
    if (soft) HCHECK(hipMemcpyAsync(h + g.soft, d + g.soft, nso, hipMemcpyDeviceToHost, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    return stage_finish(c, h, g, cf, bits, valid, trace, soft);
}

extern "C" const char* qpsk_strerror(int err) {
    switch (err) {
        case QPSK_OK: return "success";
        case QPSK_EINVAL: return "invalid argument";
        case QPSK_ENOMEM: return "out of memory";
        case QPSK_ENODEV: return "no such HIP device";
        case -4: return "every stream slot is in flight (retrieve first)";
        case QPSK_ESTALL: return "a device-side progress wait exceeded its bound; the call's outputs are undefined";
        default: break;
    }
    if (err <= QPSK_EHIP) return hipGetErrorString((hipError_t)(QPSK_EHIP - err));
    return "unknown error";
}
