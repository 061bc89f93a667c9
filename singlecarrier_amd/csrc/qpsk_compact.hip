// qpsk_compact.hip -- the receive output's format layer on the GPU
// (include/qpsk_compact.h): the dense bits / valid / trace / soft of a receive
// call -> records of the valid frames in a stated order, and the dense bit
// packing.  A stream compaction in three launches that depend on each other in
// stream order only; no workgroup ever waits for another one:
//
//   count_kernel    the order's items (channel-frames) in runs of kRun; a wave
//                   takes one run, 64 items a step, and stores the number of
//                   valid ones: one count per run in the work area.
//   scan_kernel     one workgroup of kScan threads loops over the counts, kScan
//                   a trip, and leaves their exclusive prefix in place; the
//                   total is `count` and the last entry of `groups`.
//   scatter_kernel  the same runs again.  A step ranks its 64 items with one
//                   ballot and mbcnt on top of the run's prefix; an item that
//                   starts a group stores its rank into `groups` (every group
//                   has items, so empty ones come out right).  Then the wave
//                   takes the step's valid items with rank < cap, kGather at a
//                   time: lane i loads byte i of the 62-byte row and the
//                   ballot of (byte == 1) is the record's word, which lane 0
//                   stores with channel and frame; the soft row (62 dwords)
//                   and the trace row (4) are copied a dword a lane, one
//                   contiguous access of the wave each.
//
// By-frame order walks valid[c * F + f] with c fastest: a strided byte read of
// an array that stays in cache (DESIGN.md has the measurement).
// Every offset into bits, rec, soft or trace is 64-bit.  The tiling constants
// are qpsk_compact_tile.h's.  The record entry points of the receive path and
// of the streams are here too, on the hooks of qpsk_rx_internal.h: the receive
// and stream units refer to nothing of this file.
// Not part of the receive kernels' hash (csrc/Makefile KSRC).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <vector>

#include "qpsk_compact.h"
#include "qpsk_compact_tile.h"
#include "qpsk_consts.h"
#include "qpsk_fmt.h"
#include "qpsk_herr.h"
#include "qpsk_rx_internal.h"
#include "qpsk_rx_plan.h"

namespace {

constexpr int kWave = 64;
constexpr unsigned kRun = QPSK_COMPACT_RUN_ITEMS;
constexpr unsigned kSteps = kRun / kWave;
constexpr int kBlock = QPSK_COMPACT_BLOCK_ITEMS / kRun * kWave;
constexpr int kRunsPerBlock = kBlock / kWave;
constexpr int kScan = QPSK_COMPACT_SCAN_TRIP;
constexpr int kGather = 4;           // valid items whose loads a wave has in flight
constexpr unsigned kSoftDw = QK_NDSYM * 2;
constexpr unsigned kMaxPackGrid = 1u << 20;
static_assert(kRun % kWave == 0 && QPSK_COMPACT_BLOCK_ITEMS % kRun == 0 && kBlock <= 1024, "run tiling");
static_assert(kScan % kWave == 0 && kScan <= 1024, "scan tiling");
static_assert(QK_NBITS <= kWave && kSoftDw <= kWave, "a row is one access of a wave");
static_assert(sizeof(qpsk_frame_rec) == 16, "record layout");

// The order: item i of it is channel c, frame f, at src = c * F + f of the
// dense arrays; an item with `first` starts group g.
struct Walk {
    unsigned nch, F, n;
    bool by_frame;
};
struct Item {
    unsigned c, f, src;
};
__device__ __forceinline__ Item item_of(const Walk& w, unsigned i) {
    Item t;
    if (w.by_frame) t.f = i / w.nch, t.c = i - t.f * w.nch;
    else t.c = i / w.F, t.f = i - t.c * w.F;
    t.src = t.c * w.F + t.f;   // < n < 2^28
    return t;
}

__device__ __forceinline__ unsigned lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
// set bits of m below this lane
__device__ __forceinline__ unsigned below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ __launch_bounds__(kBlock) void count_kernel(const uint8_t* __restrict__ valid, Walk w, unsigned nruns,
                                                       unsigned* __restrict__ sums) {
    const unsigned run = blockIdx.x * kRunsPerBlock + threadIdx.x / kWave;
    if (run >= nruns) return;
    const unsigned lane = lane_id();
    unsigned cnt = 0;
#pragma unroll
    for (unsigned k = 0; k < kSteps; k++) {
        const unsigned i = run * kRun + k * kWave + lane;
        const bool v = i < w.n && valid[item_of(w, i).src] != 0;
        cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(v));
    }
    if (lane == 0) sums[run] = cnt;
}

__global__ __launch_bounds__(kScan) void scan_kernel(unsigned* __restrict__ sums, unsigned nruns,
                                                     unsigned* __restrict__ count, unsigned* __restrict__ groups_end) {
    __shared__ unsigned wsum[kScan / kWave];
    const unsigned lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    unsigned carry = 0;   // the same in every thread
    for (unsigned base = 0; base < nruns; base += kScan) {
        const unsigned k = base + threadIdx.x;
        const unsigned v = k < nruns ? sums[k] : 0u;
        unsigned x = v;   // inclusive over the wave
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned y = __shfl_up(x, d, kWave);
            if (lane >= (unsigned)d) x += y;
        }
        if (lane == kWave - 1) wsum[wave] = x;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (unsigned j = 0; j < kScan / kWave; j++) {
            const unsigned t = wsum[j];
            if (j < wave) before += t;
            total += t;
        }
        if (k < nruns) sums[k] = carry + before + x - v;
        carry += total;
        __syncthreads();   // wsum is rewritten by the next trip
    }
    if (threadIdx.x == 0) {
        *count = carry;
        if (groups_end) *groups_end = carry;
    }
}

struct Scatter {
    const uint8_t* bits;
    const uint8_t* valid;
    const unsigned* trace;   // nullptr: no rec_trace
    const unsigned* soft;    // nullptr: no rec_soft
    qpsk_frame_rec* rec;     // nullptr only with cap == 0
    unsigned* rec_trace;
    unsigned* rec_soft;
    unsigned* groups;        // nullable
    size_t cap;
};

__global__ __launch_bounds__(kBlock) void scatter_kernel(Scatter a, Walk w, unsigned nruns,
                                                         const unsigned* __restrict__ prefix) {
    const unsigned run = blockIdx.x * kRunsPerBlock + threadIdx.x / kWave;
    if (run >= nruns) return;
    const unsigned lane = lane_id();
    unsigned base = prefix[run];   // valid items in front of the step
    for (unsigned k = 0; k < kSteps; k++) {
        const unsigned i = run * kRun + k * kWave + lane;
        const bool in = i < w.n;
        Item t{0, 0, 0};
        if (in) t = item_of(w, i);
        const bool v = in && a.valid[t.src] != 0;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(v);
        if (in && a.groups) {
            if (w.by_frame ? t.c == 0 : t.f == 0) a.groups[w.by_frame ? t.f : t.c] = base + below(mask);
        }
        // the step's valid items, kGather at a time; everything below is the
        // same in every lane but `lane` itself
        unsigned long long m = mask;
        unsigned r = base;   // rank of the lowest item still in m
        while (m != 0 && (size_t)r < a.cap) {
            unsigned src[kGather], cc[kGather], ff[kGather];
            bool on[kGather];
#pragma unroll
            for (int u = 0; u < kGather; u++) {
                on[u] = m != 0 && (size_t)(r + u) < a.cap;
                const int j = on[u] ? __builtin_ctzll(m) : 0;
                if (on[u]) m &= m - 1;
                src[u] = __shfl(t.src, j, kWave);
                cc[u] = __shfl(t.c, j, kWave);
                ff[u] = __shfl(t.f, j, kWave);
            }
            unsigned byte[kGather], sw[kGather], tw[kGather];
#pragma unroll
            for (int u = 0; u < kGather; u++) {
                byte[u] = sw[u] = tw[u] = 0;
                if (!on[u]) continue;
                if (lane < QK_NBITS) byte[u] = a.bits[(size_t)src[u] * QK_NBITS + lane];
                if (a.soft && lane < kSoftDw) sw[u] = a.soft[(size_t)src[u] * kSoftDw + lane];
                if (a.trace && lane < 4) tw[u] = a.trace[(size_t)src[u] * 4 + lane];
            }
#pragma unroll
            for (int u = 0; u < kGather; u++) {
                if (!on[u]) continue;
                const size_t rank = (size_t)r + u;
                const unsigned long long word = __builtin_amdgcn_ballot_w64(byte[u] == 1);
                if (lane == 0) a.rec[rank] = qpsk_frame_rec{cc[u], ff[u], word};
                if (a.soft && lane < kSoftDw) a.rec_soft[rank * kSoftDw + lane] = sw[u];
                if (a.trace && lane < 4) a.rec_trace[rank * 4 + lane] = tw[u];
            }
            r += kGather;
        }
        base += (unsigned)__builtin_popcountll(mask);
    }
}

// a wave per row: uint8 [62] -> one word
__global__ __launch_bounds__(kBlock) void pack_kernel(const uint8_t* __restrict__ bits, size_t n,
                                                      unsigned long long* __restrict__ words) {
    const unsigned lane = lane_id();
    for (size_t k = (size_t)blockIdx.x * kRunsPerBlock + threadIdx.x / kWave; k < n;
         k += (size_t)gridDim.x * kRunsPerBlock) {
        const unsigned b = lane < QK_NBITS ? bits[k * QK_NBITS + lane] : 0u;
        const unsigned long long word = __builtin_amdgcn_ballot_w64(b == 1);
        if (lane == 0) words[k] = word;
    }
}

// p (NULL included) is a multiple of a
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int qpsk_bits_pack_device(const uint8_t* d_bits, size_t n, uint64_t* d_words, void* stream) {
    if (n > 0 && (!d_bits || !d_words || !aligned(d_words, 8))) return QPSK_EINVAL;
    if (n == 0) return QPSK_OK;
    const size_t blocks = (n + kRunsPerBlock - 1) / kRunsPerBlock;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)(blocks < kMaxPackGrid ? blocks : kMaxPackGrid)), dim3(kBlock), 0,
                       (hipStream_t)stream, d_bits, n, reinterpret_cast<unsigned long long*>(d_words));
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

extern "C" int qpsk_compact_device(const uint8_t* d_bits, const uint8_t* d_valid, const int32_t* d_trace,
                                   const float* d_soft, int nch, int nframes, int order, size_t cap,
                                   qpsk_frame_rec* d_rec, int32_t* d_rec_trace, float* d_rec_soft,
                                   uint32_t* d_groups, uint32_t* d_count, void* d_work, size_t work_bytes,
                                   void* stream) {
    const int r = qpsk_compact_check(d_bits, d_valid, nch, nframes, order, cap, d_rec, d_count);
    if (r != QPSK_OK) return r;
    const size_t need = qpsk_compact_work_bytes(nch, nframes);
    if (!d_work || work_bytes < need || !aligned(d_work, 4)) return QPSK_EINVAL;
    if (!aligned(d_rec, 8) || !aligned(d_rec_trace, 4) || !aligned(d_rec_soft, 4) || !aligned(d_trace, 4) ||
        !aligned(d_soft, 4) || !aligned(d_groups, 4) || !aligned(d_count, 4))
        return QPSK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool by_frame = order == QPSK_REC_BY_FRAME;
    const size_t G = (size_t)(by_frame ? nframes : nch);
    const unsigned n = (unsigned)nch * (unsigned)nframes;   // < 2^28
    if (n == 0) {   // no items: an empty list, every group empty
        HCHECK(hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
        if (d_groups) HCHECK(hipMemsetAsync(d_groups, 0, sizeof(uint32_t) * (G + 1), s));
        return QPSK_OK;
    }
    const Walk w{(unsigned)nch, (unsigned)nframes, n, by_frame};
    const unsigned nruns = (n + kRun - 1) / kRun;
    const unsigned blocks = (nruns + kRunsPerBlock - 1) / kRunsPerBlock;
    unsigned* sums = static_cast<unsigned*>(d_work);
    hipLaunchKernelGGL(count_kernel, dim3(blocks), dim3(kBlock), 0, s, d_valid, w, nruns, sums);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, sums, nruns, d_count,
                       d_groups ? d_groups + G : nullptr);
    if (cap > 0 || d_groups) {
        Scatter a{};
        a.bits = d_bits;
        a.valid = d_valid;
        a.rec = d_rec;
        a.cap = d_rec ? cap : 0;
        if (d_trace && d_rec_trace) {
            a.trace = reinterpret_cast<const unsigned*>(d_trace);
            a.rec_trace = reinterpret_cast<unsigned*>(d_rec_trace);
        }
        if (d_soft && d_rec_soft) {
            a.soft = reinterpret_cast<const unsigned*>(d_soft);
            a.rec_soft = reinterpret_cast<unsigned*>(d_rec_soft);
        }
        a.groups = d_groups;
        hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(kBlock), 0, s, a, w, nruns, sums);
    }
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

// ---------------------------------------------------------------- the receive path in front of it
namespace {

// nch * F of a record call, checked as qpsk_rx_launch checks it
int rec_call_check(qpsk_ctx* c, int F, int order, size_t cap, const void* rec, const void* count) {
    if (!c) return QPSK_EINVAL;
    // (the dense arrays are the context's own: never NULL)
    return qpsk_compact_check(c, c, qpsk_rx_channels(c), F, order, cap, rec, count);
}

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// the device block a host call's results are made in
struct OutBlock {
    size_t count = 0, groups, rec, trace, soft, end;
    OutBlock(size_t G, size_t m, bool tr, bool so) {
        groups = sizeof(uint32_t);   // count and groups come back in one copy
        rec = up16(groups + sizeof(uint32_t) * (G + 1));
        trace = up16(rec + m * sizeof(qpsk_frame_rec));
        soft = up16(trace + (tr ? m * 4 * sizeof(int32_t) : 0));
        end = up16(soft + (so ? m * kSoftDw * sizeof(float) : 0));
    }
};

// the receive of d_in and its compaction on s; the context's buffers in *b
int records_device(qpsk_ctx* c, const int16_t* d_in, int F, int order, size_t cap, qpsk_frame_rec* d_rec,
                   int32_t* d_rec_trace, float* d_rec_soft, uint32_t* d_groups, uint32_t* d_count,
                   size_t out_bytes, qpsk_rec_bufs* b, hipStream_t s) {
    const int nch = qpsk_rx_channels(c);
    // the receive's own refusal of a misaligned input (qpsk_rx_plan.h), in front of the context's buffers
    if (F > 0 && !rx_ptrs_aligned(d_in, nullptr, nullptr, nullptr, nullptr)) return QPSK_EINVAL;
    const size_t work = qpsk_compact_work_bytes(nch, F);
    int r = qpsk_rx_rec_bufs(c, (size_t)nch * (size_t)F, d_rec_trace != nullptr, d_rec_soft != nullptr, work, out_bytes,
                             b);
    if (r != QPSK_OK) return r;
    r = qpsk_rx_batch_device(c, d_in, F, b->bits, b->valid, b->trace, b->soft, s);
    if (r != QPSK_OK) return r;
    if (out_bytes) {   // a host call: the results are made in the context's block
        const OutBlock o((size_t)(order == QPSK_REC_BY_FRAME ? F : nch), cap, d_rec_trace != nullptr,
                         d_rec_soft != nullptr);
        d_count = reinterpret_cast<uint32_t*>(b->out + o.count);
        d_groups = reinterpret_cast<uint32_t*>(b->out + o.groups);
        d_rec = cap ? reinterpret_cast<qpsk_frame_rec*>(b->out + o.rec) : nullptr;
        if (d_rec_trace) d_rec_trace = reinterpret_cast<int32_t*>(b->out + o.trace);
        if (d_rec_soft) d_rec_soft = reinterpret_cast<float*>(b->out + o.soft);
    }
    // (F == 0: no receive was launched and the dense buffers may be empty; the
    // compaction of no items reads none of them)
    r = qpsk_compact_device(b->bits, b->valid, b->trace, b->soft, nch, F, order, cap, d_rec,
                            d_rec_trace, d_rec_soft, d_groups, d_count, b->work, work, s);
    if (r != QPSK_OK || F == 0) return r;
    // the compaction reads the context's dense buffers: whoever waits for the
    // context's latest call (qpsk_rx_sync, a host call) waits for it too
    return qpsk_rx_mark(c, s);
}

struct HostIn {
    const void* in;
    int fmt;
    long ld;
};

int records_host(qpsk_ctx* c, const HostIn& hi, int F, int order, size_t cap, qpsk_frame_rec* rec, int32_t* rec_trace,
                 float* rec_soft, uint32_t* groups, uint32_t* count) {
    int r = rec_call_check(c, F, order, cap, rec, count);
    if (r != QPSK_OK) return r;
    const int nch = qpsk_rx_channels(c);
    const bool planar16 = hi.fmt == (QPSK_IN_S16 | QPSK_IN_PLANAR);
    if (!planar16 && qpsk_input_check(hi.fmt, nch, F, hi.ld) != QPSK_OK) return QPSK_EINVAL;
    if (F > 0 && !hi.in) return QPSK_EINVAL;
    const size_t cf = (size_t)nch * (size_t)F;
    const size_t G = (size_t)(order == QPSK_REC_BY_FRAME ? F : nch);
    const size_t m = cap < cf ? cap : cf;   // rows there can be
    hipStream_t s = qpsk_rx_stream(c);
    // a device call still pending on a caller's stream uses the buffers taken
    // below (a call of no frames still compacts in the context's work area)
    r = qpsk_rx_wait_pending(c);
    if (r != QPSK_OK) return r;
    int16_t* d_in = nullptr;
    if (F > 0) {
        r = qpsk_rx_fmt_conv(c, cf * QK_FRAME, &d_in);
        if (r != QPSK_OK) return r;
        if (planar16) {
            HCHECK(hipMemcpyAsync(d_in, hi.in, sizeof(int16_t) * cf * QK_FRAME, hipMemcpyHostToDevice, s));
        } else {   // the source block over PCIe as it is, converted on the device
            const size_t nraw = qpsk_input_bytes(hi.fmt, nch, F, hi.ld);
            char* raw = nullptr;
            r = qpsk_rx_fmt_raw(c, nraw, &raw);
            if (r != QPSK_OK) return r;
            HCHECK(hipMemcpyAsync(raw, hi.in, nraw, hipMemcpyHostToDevice, s));
            r = qpsk_input_convert_device(hi.fmt, raw, hi.ld, nch, F, d_in, s);
            if (r != QPSK_OK) return r;
        }
    }
    const OutBlock o(G, m, rec_trace != nullptr, rec_soft != nullptr);
    qpsk_rec_bufs b{};
    // (the rec_trace / rec_soft passed on only say which rows are wanted)
    r = records_device(c, d_in, F, order, m, rec, rec_trace, rec_soft, nullptr, nullptr, o.end, &b, s);
    if (r != QPSK_OK) return r;
    // count and groups first; then min(count, cap) rows and nothing else
    std::vector<uint32_t> head(G + 2);
    HCHECK(hipMemcpyAsync(head.data(), b.out + o.count, sizeof(uint32_t) * (G + 2), hipMemcpyDeviceToHost, s));
    const int verdict = qpsk_rx_sync(c);   // waits for the call's kernels; the copy is awaited below
    HCHECK(hipStreamSynchronize(s));
    *count = head[0];
    if (groups)
        for (size_t g = 0; g <= G; g++) groups[g] = head[1 + g];
    const size_t rows = *count < m ? (size_t)*count : m;
    if (rows > 0) {
        HCHECK(hipMemcpyAsync(rec, b.out + o.rec, rows * sizeof(qpsk_frame_rec), hipMemcpyDeviceToHost, s));
        if (rec_trace)
            HCHECK(hipMemcpyAsync(rec_trace, b.out + o.trace, rows * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (rec_soft)
            HCHECK(hipMemcpyAsync(rec_soft, b.out + o.soft, rows * kSoftDw * sizeof(float), hipMemcpyDeviceToHost, s));
        HCHECK(hipStreamSynchronize(s));
    }
    return verdict;
}

}  // namespace

extern "C" int qpsk_rx_batch_records(qpsk_ctx* c, const int16_t* in, int F, int order, size_t cap,
                                     qpsk_frame_rec* rec, int32_t* rec_trace, float* rec_soft, uint32_t* groups,
                                     uint32_t* count) {
    return records_host(c, HostIn{in, QPSK_IN_S16 | QPSK_IN_PLANAR, 0}, F, order, cap, rec, rec_trace, rec_soft,
                        groups, count);
}

extern "C" int qpsk_rx_batch_records_fmt(qpsk_ctx* c, const void* in, int fmt, long ld, int F, int order, size_t cap,
                                         qpsk_frame_rec* rec, int32_t* rec_trace, float* rec_soft, uint32_t* groups,
                                         uint32_t* count) {
    return records_host(c, HostIn{in, fmt, ld}, F, order, cap, rec, rec_trace, rec_soft, groups, count);
}

extern "C" int qpsk_rx_batch_records_device(qpsk_ctx* c, const int16_t* d_in, int F, int order, size_t cap,
                                            qpsk_frame_rec* d_rec, int32_t* d_rec_trace, float* d_rec_soft,
                                            uint32_t* d_groups, uint32_t* d_count, void* stream) {
    const int r = rec_call_check(c, F, order, cap, d_rec, d_count);
    if (r != QPSK_OK) return r;
    if (F > 0 && !d_in) return QPSK_EINVAL;
    qpsk_rec_bufs b{};
    return records_device(c, d_in, F, order, cap, d_rec, d_rec_trace, d_rec_soft, d_groups, d_count, 0, &b,
                          (hipStream_t)stream);
}

// ---------------------------------------------------------------- streams of records
namespace {

int stream_compact(const uint8_t* d_bits, const uint8_t* d_valid, int nch, int nframes, int order, size_t cap,
                   void* d_rec, uint32_t* d_groups, uint32_t* d_count, void* d_work, size_t work_bytes,
                   void* stream) {
    return qpsk_compact_device(d_bits, d_valid, nullptr, nullptr, nch, nframes, order, cap,
                               static_cast<qpsk_frame_rec*>(d_rec), nullptr, nullptr, d_groups, d_count, d_work,
                               work_bytes, stream);
}

}  // namespace

extern "C" qpsk_stream* qpsk_stream_create_records(int device, int nch, int frames, int nslot, int mode, int fmt,
                                                   int order, size_t cap, int* err) {
    const bool planar16 = fmt == (QPSK_IN_S16 | QPSK_IN_PLANAR);
    if ((order != QPSK_REC_BY_CHANNEL && order != QPSK_REC_BY_FRAME) || nch < 1 || frames < 1 ||
        (uint64_t)nch * (uint64_t)frames >= QPSK_COMPACT_MAX_ITEMS ||
        (!planar16 && qpsk_input_check(fmt, nch, frames, nch) != QPSK_OK)) {
        if (err) *err = QPSK_EINVAL;
        return nullptr;
    }
    const size_t cf = (size_t)nch * (size_t)frames;
    qpsk_stream_post p;
    p.order = order;
    p.cap = cap < cf ? cap : cf;   // a chunk has no more
    p.rec_bytes = sizeof(qpsk_frame_rec);
    p.ngroups = (size_t)(order == QPSK_REC_BY_FRAME ? frames : nch);
    p.work_bytes = qpsk_compact_work_bytes(nch, frames);
    p.compact = stream_compact;
    return qpsk_stream_create_post(device, nch, frames, nslot, mode, fmt,
                                   planar16 ? 0 : qpsk_input_bytes(fmt, nch, frames, nch),
                                   planar16 ? nullptr : qpsk_input_convert_device, &p, err);
}

extern "C" int qpsk_stream_retrieve_records(qpsk_stream* s, const qpsk_frame_rec** rec, uint32_t* count,
                                            const uint32_t** groups) {
    if (!rec) return QPSK_EINVAL;
    const void* r = nullptr;
    const int v = qpsk_stream_retrieve_post(s, &r, count, groups);
    if (v != QPSK_EINVAL) *rec = static_cast<const qpsk_frame_rec*>(r);
    return v;
}
