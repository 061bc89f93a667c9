// qpsk_level.hip -- the input level meter and the squelch on the GPU
// (include/qpsk_level.h), and the record calls that run them between the
// receive and the compaction.
//
//   level_kernel    a streaming reduction over the int16 block the receive
//                   reads.  A wave takes one row (frame) of 3,760 bytes = 235
//                   16-byte words: lane i loads words i, i + 64, i + 128 and
//                   i + 192 (the last one for 43 lanes), all four in flight
//                   before the first is used, sums its 32 samples, and the wave
//                   reduces with xor shuffles; lane 0 stores the row's 16-byte
//                   level at once.  Integer arithmetic throughout, so the tree
//                   does not matter.  Widths: a lane's sum of squares reaches
//                   32 * 2^30, a row's 1880 * 2^30 > 2^40: 64-bit from the
//                   second square on (two squares of -32768 are 2^31, which an
//                   unsigned word still holds: they are added as a pair).
//                   No atomics, no LDS, no workgroup waits for another.
//   squelch_kernel  one lane per channel-frame: the gate of the header from
//                   the frame's level and the one in front of it, the flag, and
//                   for a frame that was valid and is squelched the zeroing of
//                   its bits row (31 two-byte stores) and soft row (31
//                   eight-byte stores): the rows' own alignments, nothing wider.
//   last_kernel     a second launch, one lane per channel: last[c], which may
//                   be prev[c] that squelch_kernel read.
//
// The record entry points are built on the hooks of qpsk_rx_internal.h as
// qpsk_compact.hip builds its own: the receive, stream and compaction units
// refer to nothing of this file.  For input in another format than planar
// int16 (the _fmt calls, squelch streams) the levels come from the conversion's
// own pass (qpsk_input_convert_level_device, qpsk_input.hip), not from
// level_kernel.  What level_kernel shares with that pass is qpsk_level_dev.h.
// Not part of the receive kernels' hash (csrc/Makefile KSRC).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <vector>

#include "qpsk_compact.h"
#include "qpsk_compact_tile.h"
#include "qpsk_consts.h"
#include "qpsk_fmt.h"
#include "qpsk_herr.h"
#include "qpsk_input.h"
#include "qpsk_level.h"
#include "qpsk_level_dev.h"
#include "qpsk_level_tile.h"
#include "qpsk_rx_internal.h"
#include "qpsk_rx_plan.h"

namespace {

using namespace qlevel;   // kWave, LevelWords, Acc, take2

constexpr int kRows = QPSK_LEVEL_BLOCK_ROWS;
constexpr int kBlock = kRows * kWave;
constexpr int kVec = 8;                                   // samples of a 16-byte word
constexpr int kRowVec = QK_FRAME / kVec;                  // 235 words a row
constexpr int kLoads = (kRowVec + kWave - 1) / kWave;     // 4 words a lane
constexpr int kSqBlock = 256;
constexpr unsigned kSoftQw = QK_NDSYM;                    // a soft row in 8-byte words
constexpr uintptr_t kAlignLevel = 8;
static_assert(QK_FRAME % kVec == 0 && kBlock <= 1024, "meter tiling");
static_assert(QK_NBITS % 2 == 0 && sizeof(float) * 2 * QK_NDSYM == 8 * kSoftQw, "row alignments");

__global__ __launch_bounds__(kBlock) void level_kernel(const int4* __restrict__ in, size_t nrows,
                                                       LevelWords* __restrict__ out) {
    const size_t row = (size_t)blockIdx.x * kRows + threadIdx.x / kWave;
    if (row >= nrows) return;   // (a whole wave: no shuffle below has a lane missing)
    const unsigned lane = threadIdx.x % kWave;
    const int4* p = in + row * kRowVec;
    int4 v[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; k++) {
        const unsigned i = k * kWave + lane;
        v[k] = i < (unsigned)kRowVec ? p[i] : make_int4(0, 0, 0, 0);   // zeros add nothing to any field
    }
    Acc a;
#pragma unroll
    for (int k = 0; k < kLoads; k++) {
        take2(a, v[k].x);
        take2(a, v[k].y);
        take2(a, v[k].z);
        take2(a, v[k].w);
    }
    // (wave_reduce and pack of qpsk_level_dev.h, written out: see there)
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        a.sumsq += __shfl_xor(a.sumsq, d, kWave);
        a.sum += __shfl_xor(a.sum, d, kWave);
        a.peak = max(a.peak, (unsigned)__shfl_xor(a.peak, d, kWave));
        a.clipped += __shfl_xor(a.clipped, d, kWave);
    }
    if (lane == 0)
        out[row] = LevelWords{a.sumsq, (unsigned long long)(unsigned)a.sum | (unsigned long long)a.peak << 32 |
                                           (unsigned long long)a.clipped << 48};
}

struct Squelch {
    const LevelWords* level;
    const LevelWords* prev;   // nullable
    unsigned F, n;
    unsigned long long min_sumsq;
    const uint8_t* valid_in;
    uint8_t* valid_out;
    uint16_t* bits;             // nullable
    unsigned long long* soft;   // nullable
};

__global__ __launch_bounds__(kSqBlock) void squelch_kernel(Squelch a) {
    const unsigned i = blockIdx.x * kSqBlock + threadIdx.x;   // < n < 2^28
    if (i >= a.n) return;
    const unsigned c = i / a.F, f = i - c * a.F;
    const unsigned long long cur = a.level[i].sumsq;
    const unsigned long long p = f > 0 ? a.level[i - 1].sumsq : a.prev ? a.prev[c].sumsq : 0ull;
    const bool keep = (cur > p ? cur : p) >= a.min_sumsq;
    const uint8_t v = a.valid_in[i];
    a.valid_out[i] = keep ? v : (uint8_t)0;
    if (keep || !v) return;
    // (volatile: the compiler merges plain stores into 16-byte ones, past the
    // rows' 2- and 8-byte alignment)
    if (a.bits) {
        volatile uint16_t* row = a.bits + (size_t)i * (QK_NBITS / 2);
#pragma unroll
        for (int k = 0; k < QK_NBITS / 2; k++) row[k] = 0;
    }
    if (a.soft) {
        volatile unsigned long long* row = a.soft + (size_t)i * kSoftQw;
#pragma unroll
        for (unsigned k = 0; k < kSoftQw; k++) row[k] = 0;
    }
}

__global__ __launch_bounds__(kSqBlock) void last_kernel(const LevelWords* level, const LevelWords* prev, unsigned nch,
                                                        unsigned F, LevelWords* last) {
    const unsigned c = blockIdx.x * kSqBlock + threadIdx.x;
    if (c >= nch) return;
    const LevelWords* src = F > 0 ? level + ((size_t)c * F + (F - 1)) : prev ? prev + c : nullptr;
    unsigned long long sumsq = 0, rest = 0;
    if (src) sumsq = src->sumsq, rest = src->rest;
    last[c] = LevelWords{sumsq, rest};
}

// p (NULL included) is a multiple of a
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int qpsk_level_device(const int16_t* d_in, size_t nrows, qpsk_frame_level* d_out, void* stream) {
    const int r = qpsk_level_check(d_in, nrows, d_out);
    if (r != QPSK_OK) return r;
    if (nrows == 0) return QPSK_OK;
    if (!aligned(d_in, kAlignIn) || !aligned(d_out, kAlignLevel)) return QPSK_EINVAL;
    const size_t blocks = (nrows + kRows - 1) / kRows;   // < 2^26
    hipLaunchKernelGGL(level_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4*>(d_in), nrows, reinterpret_cast<LevelWords*>(d_out));
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

extern "C" int qpsk_squelch_device(const qpsk_frame_level* d_level, const qpsk_frame_level* d_prev, int nch,
                                   int nframes, uint64_t min_sumsq, const uint8_t* d_valid_in, uint8_t* d_valid_out,
                                   uint8_t* d_bits, float* d_soft, qpsk_frame_level* d_last, void* stream) {
    const int r = qpsk_squelch_check(d_level, nch, nframes, d_valid_in, d_valid_out);
    if (r != QPSK_OK) return r;
    if (!aligned(d_level, kAlignLevel) || !aligned(d_prev, kAlignLevel) || !aligned(d_last, kAlignLevel) ||
        !aligned(d_bits, kAlignBits) || !aligned(d_soft, kAlignSoft))
        return QPSK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const unsigned n = (unsigned)nch * (unsigned)nframes;   // < 2^28
    const LevelWords* level = reinterpret_cast<const LevelWords*>(d_level);
    const LevelWords* prev = reinterpret_cast<const LevelWords*>(d_prev);
    if (n > 0) {
        const Squelch a{level, prev, (unsigned)nframes, n, min_sumsq, d_valid_in, d_valid_out,
                        reinterpret_cast<uint16_t*>(d_bits), reinterpret_cast<unsigned long long*>(d_soft)};
        hipLaunchKernelGGL(squelch_kernel, dim3((n + kSqBlock - 1) / kSqBlock), dim3(kSqBlock), 0, s, a);
    }
    // (no frames: last[c] = prev[c], nothing to do where they are one array)
    if (d_last && nch > 0 && (nframes > 0 || d_last != d_prev))
        hipLaunchKernelGGL(last_kernel, dim3(((unsigned)nch + kSqBlock - 1) / kSqBlock), dim3(kSqBlock), 0, s, level, prev,
                           (unsigned)nch, (unsigned)nframes, reinterpret_cast<LevelWords*>(d_last));
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

// ---------------------------------------------------------------- the receive path around them
namespace {

constexpr unsigned kSoftDw = QK_NDSYM * 2;

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// the device block a host call's results are made in: qpsk_compact.hip's own
// layout (count and groups side by side: one copy), then the levels carried in
// and out
struct OutBlock {
    size_t count = 0, groups, rec, trace, soft, prev, end;
    OutBlock(size_t G, size_t m, bool tr, bool so, size_t nprev) {
        groups = sizeof(uint32_t);
        rec = up16(groups + sizeof(uint32_t) * (G + 1));
        trace = up16(rec + m * sizeof(qpsk_frame_rec));
        soft = up16(trace + (tr ? m * 4 * sizeof(int32_t) : 0));
        prev = up16(soft + (so ? m * kSoftDw * sizeof(float) : 0));
        end = up16(prev + nprev * sizeof(qpsk_frame_level));
    }
};

struct Call {
    qpsk_ctx* c;
    int F;
    uint64_t min_sumsq;
    int order;
    size_t cap;
};

int call_check(const Call& k, const void* rec, const void* count) {
    if (!k.c) return QPSK_EINVAL;
    // (the dense arrays are the context's own: never NULL)
    return qpsk_compact_check(k.c, k.c, qpsk_rx_channels(k.c), k.F, k.order, k.cap, rec, count);
}

// What a call made on the device, for the host form to copy back
struct Made {
    qpsk_rec_bufs b;
    qpsk_frame_level* level;
};

// The input of a call on the device: a block in format fmt (include/qpsk_input.h)
struct In {
    const void* d;
    int fmt;
    long ld;
    bool planar16() const { return fmt == (QPSK_IN_S16 | QPSK_IN_PLANAR); }
};

// Receive, meter, squelch and compaction of `in` on s.  Planar int16 is
// received where it lies and metered by level_kernel; a block in any other
// format is converted into the context's buffer by the pass that also takes
// the levels (qpsk_input_convert_level_device): no level_kernel launch.  A
// device call gives its own pointers; a host call (out != nullptr) gets the
// results in the context's block, with prev_host copied in behind the buffers'
// growth.  want_trace / want_soft: whether those rows are made.
int enqueue(const Call& k, const In& in, qpsk_frame_level* d_prev_io, qpsk_frame_rec* d_rec,
            int32_t* d_rec_trace, float* d_rec_soft, uint32_t* d_groups, uint32_t* d_count, qpsk_frame_level* d_level,
            bool want_trace, bool want_soft, const OutBlock* out, const qpsk_frame_level* prev_host, Made* made,
            hipStream_t s) {
    const int nch = qpsk_rx_channels(k.c), F = k.F;
    const size_t cf = (size_t)nch * (size_t)F;
    const bool p16 = in.planar16();
    // the receive's own refusal of a misaligned input (qpsk_rx_plan.h), or the
    // conversion's, in front of the context's buffers
    if (F > 0 && (p16 ? !rx_ptrs_aligned(static_cast<const int16_t*>(in.d), nullptr, nullptr, nullptr, nullptr)
                      : !aligned(in.d, (uintptr_t)qpsk_fmt_esize(in.fmt))))
        return QPSK_EINVAL;
    if (!aligned(d_prev_io, kAlignLevel) || !aligned(d_level, kAlignLevel)) return QPSK_EINVAL;
    // the work area: the compaction's counts, then the levels where the caller
    // takes none, then the partial levels of the conversion's pass
    const size_t cwork = qpsk_compact_work_bytes(nch, F), lvl_at = up16(cwork);
    const size_t part_at = up16(lvl_at + (d_level ? 0 : cf * sizeof(qpsk_frame_level)));
    const size_t part_bytes = p16 ? 0 : qpsk_input_level_work(in.fmt, nch, F, in.ld);
    const size_t work = part_at + part_bytes;
    qpsk_rec_bufs& b = made->b;
    int r = qpsk_rx_rec_bufs(k.c, cf, want_trace, want_soft, work, out ? out->end : 0, &b);
    if (r != QPSK_OK) return r;
    if (out) {
        d_count = reinterpret_cast<uint32_t*>(b.out + out->count);
        d_groups = reinterpret_cast<uint32_t*>(b.out + out->groups);
        d_rec = k.cap ? reinterpret_cast<qpsk_frame_rec*>(b.out + out->rec) : nullptr;
        d_rec_trace = want_trace ? reinterpret_cast<int32_t*>(b.out + out->trace) : nullptr;
        d_rec_soft = want_soft ? reinterpret_cast<float*>(b.out + out->soft) : nullptr;
        if (prev_host) {
            d_prev_io = reinterpret_cast<qpsk_frame_level*>(b.out + out->prev);
            if (F > 0) HCHECK(hipMemcpyAsync(d_prev_io, prev_host, sizeof(qpsk_frame_level) * (size_t)nch,
                                             hipMemcpyHostToDevice, s));
        }
    }
    if (!d_level) d_level = reinterpret_cast<qpsk_frame_level*>(static_cast<char*>(b.work) + lvl_at);
    made->level = d_level;
    const int16_t* d_in = static_cast<const int16_t*>(in.d);
    if (!p16 && F > 0) {   // the receive's input and the levels in one pass over the source
        int16_t* conv = nullptr;
        r = qpsk_rx_fmt_conv(k.c, cf * QK_FRAME, &conv);
        if (r != QPSK_OK) return r;
        r = qpsk_input_convert_level_device(in.fmt, in.d, in.ld, nch, F, conv, d_level,
                                            static_cast<char*>(b.work) + part_at, part_bytes, s);
        if (r != QPSK_OK) return r;
        d_in = conv;
    }
    r = qpsk_rx_batch_device(k.c, d_in, F, b.bits, b.valid, b.trace, b.soft, s);
    if (r != QPSK_OK) return r;
    if (F > 0) {
        if (p16) {
            r = qpsk_level_device(d_in, cf, d_level, s);
            if (r != QPSK_OK) return r;
        }
        // the flags in place; the rows of squelched frames stay as they are:
        // the compaction reads the rows of valid frames only
        r = qpsk_squelch_device(d_level, d_prev_io, nch, F, k.min_sumsq, b.valid, b.valid, nullptr, nullptr, d_prev_io, s);
        if (r != QPSK_OK) return r;
    }
    r = qpsk_compact_device(b.bits, b.valid, b.trace, b.soft, nch, F, k.order, k.cap, d_rec, d_rec_trace, d_rec_soft,
                            d_groups, d_count, b.work, cwork, s);
    if (r != QPSK_OK || F == 0) return r;
    // the passes read the context's buffers: whoever waits for the context's
    // latest call (qpsk_rx_sync, a host call) waits for them too
    return qpsk_rx_mark(k.c, s);
}

}  // namespace

extern "C" int qpsk_rx_batch_records_squelch_device_fmt(qpsk_ctx* c, const void* d_in, int fmt, long ld, int F,
                                                        uint64_t min_sumsq, qpsk_frame_level* d_prev_io, int order,
                                                        size_t cap, qpsk_frame_rec* d_rec, int32_t* d_rec_trace,
                                                        float* d_rec_soft, uint32_t* d_groups, uint32_t* d_count,
                                                        qpsk_frame_level* d_level, void* stream) {
    const Call k{c, F, min_sumsq, order, cap};
    const int r = call_check(k, d_rec, d_count);
    if (r != QPSK_OK) return r;
    const In in{d_in, fmt, ld};
    if (!in.planar16() && qpsk_input_check(fmt, qpsk_rx_channels(c), F, ld) != QPSK_OK) return QPSK_EINVAL;
    if (F > 0 && !d_in) return QPSK_EINVAL;
    Made made{};
    return enqueue(k, in, d_prev_io, d_rec, d_rec_trace, d_rec_soft, d_groups, d_count, d_level,
                   d_rec_trace != nullptr, d_rec_soft != nullptr, nullptr, nullptr, &made, (hipStream_t)stream);
}

extern "C" int qpsk_rx_batch_records_squelch_device(qpsk_ctx* c, const int16_t* d_in, int F, uint64_t min_sumsq,
                                                    qpsk_frame_level* d_prev_io, int order, size_t cap,
                                                    qpsk_frame_rec* d_rec, int32_t* d_rec_trace, float* d_rec_soft,
                                                    uint32_t* d_groups, uint32_t* d_count, qpsk_frame_level* d_level,
                                                    void* stream) {
    return qpsk_rx_batch_records_squelch_device_fmt(c, d_in, QPSK_IN_S16 | QPSK_IN_PLANAR, 0, F, min_sumsq, d_prev_io,
                                                    order, cap, d_rec, d_rec_trace, d_rec_soft, d_groups, d_count,
                                                    d_level, stream);
}

extern "C" int qpsk_rx_batch_records_squelch_fmt(qpsk_ctx* c, const void* in, int fmt, long ld, int F,
                                                 uint64_t min_sumsq, qpsk_frame_level* prev_io, int order, size_t cap,
                                                 qpsk_frame_rec* rec, int32_t* rec_trace, float* rec_soft,
                                                 uint32_t* groups, uint32_t* count, qpsk_frame_level* level) {
    Call k{c, F, min_sumsq, order, cap};
    int r = call_check(k, rec, count);
    if (r != QPSK_OK) return r;
    const int nch = qpsk_rx_channels(c);
    const bool p16 = fmt == (QPSK_IN_S16 | QPSK_IN_PLANAR);
    if (!p16 && qpsk_input_check(fmt, nch, F, ld) != QPSK_OK) return QPSK_EINVAL;
    if (F > 0 && !in) return QPSK_EINVAL;
    const size_t cf = (size_t)nch * (size_t)F;
    const size_t G = (size_t)(order == QPSK_REC_BY_FRAME ? F : nch);
    const size_t m = cap < cf ? cap : cf;   // rows there can be
    k.cap = m;
    hipStream_t s = qpsk_rx_stream(c);
    // a device call still pending on a caller's stream uses the buffers taken below
    r = qpsk_rx_wait_pending(c);
    if (r != QPSK_OK) return r;
    In d_in{nullptr, fmt, ld};
    if (F > 0 && p16) {
        int16_t* conv = nullptr;
        r = qpsk_rx_fmt_conv(c, cf * QK_FRAME, &conv);
        if (r != QPSK_OK) return r;
        HCHECK(hipMemcpyAsync(conv, in, sizeof(int16_t) * cf * QK_FRAME, hipMemcpyHostToDevice, s));
        d_in.d = conv;
    } else if (F > 0) {   // the source block over PCIe as it is
        const size_t nraw = qpsk_input_bytes(fmt, nch, F, ld);
        char* raw = nullptr;
        r = qpsk_rx_fmt_raw(c, nraw, &raw);
        if (r != QPSK_OK) return r;
        HCHECK(hipMemcpyAsync(raw, in, nraw, hipMemcpyHostToDevice, s));
        d_in.d = raw;
    }
    const OutBlock o(G, m, rec_trace != nullptr, rec_soft != nullptr, prev_io ? (size_t)nch : 0);
    Made made{};
    r = enqueue(k, d_in, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rec_trace != nullptr,
                rec_soft != nullptr, &o, prev_io, &made, s);
    if (r != QPSK_OK) return r;
    const char* out = made.b.out;
    // count and groups first (with the levels); then min(count, cap) rows and nothing else
    std::vector<uint32_t> head(G + 2);
    HCHECK(hipMemcpyAsync(head.data(), out + o.count, sizeof(uint32_t) * (G + 2), hipMemcpyDeviceToHost, s));
    if (F > 0 && level) HCHECK(hipMemcpyAsync(level, made.level, sizeof(qpsk_frame_level) * cf, hipMemcpyDeviceToHost, s));
    if (F > 0 && prev_io)
        HCHECK(hipMemcpyAsync(prev_io, out + o.prev, sizeof(qpsk_frame_level) * (size_t)nch, hipMemcpyDeviceToHost, s));
    const int verdict = qpsk_rx_sync(c);   // waits for the call's kernels; the copies are awaited below
    HCHECK(hipStreamSynchronize(s));
    *count = head[0];
    if (groups)
        for (size_t g = 0; g <= G; g++) groups[g] = head[1 + g];
    const size_t rows = *count < m ? (size_t)*count : m;
    if (rows > 0) {
        HCHECK(hipMemcpyAsync(rec, out + o.rec, rows * sizeof(qpsk_frame_rec), hipMemcpyDeviceToHost, s));
        if (rec_trace)
            HCHECK(hipMemcpyAsync(rec_trace, out + o.trace, rows * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (rec_soft)
            HCHECK(hipMemcpyAsync(rec_soft, out + o.soft, rows * kSoftDw * sizeof(float), hipMemcpyDeviceToHost, s));
        HCHECK(hipStreamSynchronize(s));
    }
    return verdict;
}

extern "C" int qpsk_rx_batch_records_squelch(qpsk_ctx* c, const int16_t* in, int F, uint64_t min_sumsq,
                                             qpsk_frame_level* prev_io, int order, size_t cap, qpsk_frame_rec* rec,
                                             int32_t* rec_trace, float* rec_soft, uint32_t* groups, uint32_t* count,
                                             qpsk_frame_level* level) {
    return qpsk_rx_batch_records_squelch_fmt(c, in, QPSK_IN_S16 | QPSK_IN_PLANAR, 0, F, min_sumsq, prev_io, order, cap,
                                             rec, rec_trace, rec_soft, groups, count, level);
}

// ---------------------------------------------------------------- streams of records with squelch
namespace {

int stream_convert_level(int fmt, const void* d_src, long ld, int nch, int nframes, int16_t* d_out, void* d_level,
                         void* d_work, size_t work_bytes, void* stream) {
    return qpsk_input_convert_level_device(fmt, d_src, ld, nch, nframes, d_out, static_cast<qpsk_frame_level*>(d_level),
                                           d_work, work_bytes, stream);
}

// the chunk's levels (made here from planar int16 input), the gate with the
// stream's carried levels as prev and last, then the compaction
int stream_squelch_compact(const int16_t* d_in, bool have_level, void* d_level, void* d_carry, uint64_t min_sumsq,
                           const uint8_t* d_bits, uint8_t* d_valid, int nch, int nframes, int order, size_t cap,
                           void* d_rec, uint32_t* d_groups, uint32_t* d_count, void* d_work, size_t work_bytes,
                           void* stream) {
    qpsk_frame_level* level = static_cast<qpsk_frame_level*>(d_level);
    qpsk_frame_level* carry = static_cast<qpsk_frame_level*>(d_carry);
    int r = have_level ? QPSK_OK : qpsk_level_device(d_in, (size_t)nch * (size_t)nframes, level, stream);
    if (r != QPSK_OK) return r;
    r = qpsk_squelch_device(level, carry, nch, nframes, min_sumsq, d_valid, d_valid, nullptr, nullptr, carry, stream);
    if (r != QPSK_OK) return r;
    return qpsk_compact_device(d_bits, d_valid, nullptr, nullptr, nch, nframes, order, cap,
                               static_cast<qpsk_frame_rec*>(d_rec), nullptr, nullptr, d_groups, d_count, d_work,
                               work_bytes, stream);
}

}  // namespace

extern "C" qpsk_stream* qpsk_stream_create_records_squelch(int device, int nch, int frames, int nslot, int mode, int fmt,
                                                           int order, size_t cap, uint64_t min_sumsq, int* err) {
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
    p.level_bytes = sizeof(qpsk_frame_level);
    p.level_work_bytes = planar16 ? 0 : qpsk_input_level_work(fmt, nch, frames, nch);
    p.arg = min_sumsq;
    p.convert_level = planar16 ? nullptr : stream_convert_level;
    p.compact_level = stream_squelch_compact;
    return qpsk_stream_create_post(device, nch, frames, nslot, mode, fmt,
                                   planar16 ? 0 : qpsk_input_bytes(fmt, nch, frames, nch),
                                   planar16 ? nullptr : qpsk_input_convert_device, &p, err);
}

extern "C" int qpsk_stream_retrieve_records_squelch(qpsk_stream* s, const qpsk_frame_rec** rec, uint32_t* count,
                                                    const uint32_t** groups, const qpsk_frame_level** level) {
    if (!rec) return QPSK_EINVAL;
    const void *r = nullptr, *l = nullptr;
    const int v = qpsk_stream_retrieve_post_level(s, &r, count, groups, level ? &l : nullptr);
    if (v != QPSK_EINVAL) {
        *rec = static_cast<const qpsk_frame_rec*>(r);
        if (level) *level = static_cast<const qpsk_frame_level*>(l);
    }
    return v;
}
