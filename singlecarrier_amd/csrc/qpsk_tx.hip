// qpsk_tx.hip -- the batched transmitter of include/qpsk_tx.h on the GPU:
// qpsk_tx_frame (src/qpsk.c:278-322) in the packet order of the reference's
// main() (src/qpsk.c:380-413) for many channels with caller-supplied payload
// bits, bit-identical to the host twin qpsk_tx_batch_host (qpsk_tx_host.c).
//
// What a sample depends on (DESIGN.md "Batched transmitter"):
//   * a channel's row is one flat stream of npackets * P samples, P = 1880 +
//     gap; position p is packet k = p / P, offset r = p % P; r >= 1880 is gap
//     (zero, never filtered: the reference fwrites it), otherwise it is TX
//     sample t = 1880 k + r of the call;
//   * the FIR input is the zero-stuffed symbol stream, so sample t is the sum
//     over the <= 10 symbols S - 9 .. S (S = t / 5) of +-QK_RRC[i], i ascending
//     (one packed fma per tap: see period());
//     symbols before a packet's first are the previous packet's last 9
//     whatever the gap, taken from the payload when that packet is in this
//     call, from the saved per-channel state otherwise, and zero before the
//     context's first packet;
//   * the carrier depends on the transmitter's call sequence only: the host
//     continues the reference's fp32 recurrence from the carried phase and
//     uploads one float2 per TX sample of the call.
//
// Shape.  The arithmetic wants a thread to own one symbol period (5 samples
// whose tap indices are compile-time constants); the stores want a lane to own
// 8 consecutive samples at a 16-byte-aligned address.  P is odd for the
// reference gap and ld and out are the caller's, so the two never line up:
// the block computes into an LDS tile (ds_write_b16) and stores from it
// (ds_read_b128 -> global_store_dwordx4).  A block owns kTile samples of the
// row, cut at 16-byte-aligned addresses, and loops over kLoop channels of one
// alignment class (c mod 8: rows 8 apart differ by 8 ld samples, so they share
// out + c ld mod 16 bytes).  Everything that does not depend on the channel --
// (k, r), the LDS slot, the scale and the 5 carrier values of each period --
// is worked out once and kept in registers over that loop; per channel only
// the payload changes: its bytes are read once per tile, reduced to one sign
// bit per component with ballots, and kept in LDS as two bit strings.  Gap
// positions of the tile are zeroed once and never overwritten, so the same
// store pass writes the gap.  Row heads and tails that do not fill an aligned
// 16 bytes are stored per int16.  The same kernel writes the planar G.711
// formats of include/qpsk_output.h: its store pass compresses a lane's 8
// samples into one aligned 8-byte store (heads and tails per code).
//
// Channels that come and go (qpsk_tx.h).  The above is the *uniform* context:
// every channel at the context's packet count.  Once a channel has an index of
// its own (qpsk_tx_reset_channels, qpsk_tx_state_load, a call with a mask) the
// context is *general* until qpsk_tx_reset: the indices live on the device, a
// pre-pass (tx_plan_kernel) walks each channel's slots once and writes one plan
// word per channel and slot, and tx_mask_kernel, tx_batch_kernel's tiling with
// everything that was per period now per period, channel and slot, modulates
// from the plan.  The carrier needs no recurrence there: from packet 8 on each
// packet's carrier is the exact negation of the one before (DESIGN.md "The
// carrier's period"), so own index p reads row min(p, 8) of a 9-packet table
// uploaded once per context, negated for odd p > 8.
#include <hip/hip_runtime.h>

#include <new>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_consts.h"
#include "qpsk_fmt_dev.h"
#include "qpsk_hip_host.h"
#include "qpsk_tx.h"
#include "qpsk_tx_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTxPacket = QPSK_TX_PACKET;         // qpsk_tx_internal.h
constexpr int kPacketBits = QPSK_TX_PACKET_BITS;
constexpr int kSymPacket = 376;    // 128 + 8*31 symbols per packet
constexpr int kHist = 9;           // earlier symbols a sample's FIR window reaches
constexpr int kThreads = 256;
constexpr int kChunk = 8;                    // samples per 16-byte store
constexpr int kTile = kThreads * kChunk;     // samples of a row per block
constexpr int kMargin = 8;         // LDS slots either side of the tile: a period that straddles
                                   // the tile's edge is written whole, its outside part never read
constexpr int kClasses = 8;        // alignment classes: (out + c*ld) mod 16 bytes repeats every 8 rows
constexpr int kLoop = 16;          // channels of one class a block loops over
constexpr int kRounds = 2;         // periods per thread: kTile/5 + 2 <= kRounds * kThreads
constexpr int kSignBits = kRounds * kThreads;   // sign bits per channel and component, 64 per ballot
constexpr int kSignWords = kSignBits / 32 + 1;  // + one zero word: a window read may touch it
static_assert(kTile / 5 + 2 <= kRounds * kThreads, "a tile's periods must fit the rounds");
static_assert(kTile / 5 + 2 + kHist <= kSignBits, "and their symbols the bit strings");
static_assert(kMargin >= 4 && kMargin % kChunk == 0, "margin keeps the 16-byte LDS reads aligned");

// The plan word of a channel's slot (tx_plan_kernel -> tx_mask_kernel).  The 9
// history dibits ride in the word itself, in the saved state's layout (bit j =
// I sign, bit 16 + j = Q sign), so the modulator never chases where they came
// from: an earlier slot of the call, the saved word, or none (kPlanStart).
constexpr uint32_t kDibits = 0x01ff01ffu;
constexpr uint32_t kPlanActive = 1u << 31;   // the channel sends in this slot
constexpr uint32_t kPlanStart = 1u << 30;    // its first packet: zero filter memory
constexpr uint32_t kPlanNeg = 1u << 29;      // carrier = minus the table row
constexpr int kPlanRowShift = 25;            // carrier row 0 .. 8, 4 bits
constexpr int kCarrierRows = 9;              // packets 0 .. 7 are a transient, 8 repeats negated
constexpr int kPlanSlots = 4;                // slots a tile's periods and their history touch
static_assert((kSymPacket - 1 + kTile / 5 + 2) / kSymPacket + 2 <= kPlanSlots,
              "a tile's last period lies at most 2 slots past its first, and reads the slot after");

// bit u set: preamble symbol u is -1 (both components, src/qpsk.c:361-365)
constexpr unsigned long long pre_neg(int half) {
    unsigned long long m = 0;
    for (int i = 0; i < 64; i++)
        if (QK_PRE[half * 64 + i] < 0) m |= 1ull << i;
    return m;
}

__host__ __device__ inline long lmin(long a, long b) { return a < b ? a : b; }

typedef float v2f __attribute__((ext_vector_type(2)));

// One symbol period (5 samples) of one channel into the LDS tile.
//   wi, wq   bit j = sign of symbol S - 9 + j (1: -1), j = 0 .. 9
//   live     kZeros only: bit j clear = that symbol is before the stream's
//            first (a zero in tx_filter)
//   ph       carrier of the period's 5 samples; scale 8192 (preamble) or 16384
// fir(): y = sum_i mem[i]*c[i], i ascending (src/fir.c:36-42), where only the
// symbol instants are nonzero: sample jj of the period has symbol S - m at tap
// i = 48 - jj - 5 m.  The reference rounds twice per tap, mem*c and y + that;
// mem is +-1 (or 0), so the product is exact and fma(mem, c, y), which rounds
// mem*c + y once, is the same fp32 value: an explicit fma here is not a
// contraction that changes a result.  (re, im) ride one packed instruction.
template <bool kZeros>
__device__ inline void period(uint32_t wi, uint32_t wq, uint32_t live, const float2 (&ph)[5],
                              float scale, int16_t* dst) {
    v2f s[10];
#pragma unroll
    for (int j = 0; j < 10; j++) {
        uint32_t a = ((wi << (31 - j)) & 0x80000000u) | 0x3f800000u;   // -1.0f or 1.0f
        uint32_t b = ((wq << (31 - j)) & 0x80000000u) | 0x3f800000u;
        if (kZeros && !((live >> j) & 1u)) a = b = 0u;
        s[j] = v2f{__uint_as_float(a), __uint_as_float(b)};
    }
#pragma unroll
    for (int jj = 0; jj < 5; jj++) {
        v2f y = {0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 10; j++) {
            const int i = 48 - jj - 5 * (9 - j);
            if (i < 0) continue;
            y = __builtin_elementwise_fma(s[j], v2f{QK_RRC[i], QK_RRC[i]}, y);
        }
        y = y * QK_GAIN;
        const float sr = y.x * ph[jj].x - y.y * ph[jj].y;   // crealf(signal * phase), src/qpsk.c:301-304
        dst[jj] = (int16_t)(int)(sr * scale);               // src/qpsk.c:313-319
    }
}

// grid.x = 8 * channel groups (class = x & 7), grid.y = tiles of this launch
// ENC: the element the store pass writes, int16 (QPSK_OUT_S16) or the sample's
// G.711 code (QPSK_OUT_ALAW, QPSK_OUT_ULAW: the planar formats of
// include/qpsk_output.h).  A lane's 8 codes are one 8-byte store, and
// (out + c * ld) mod 8 bytes repeats every 8 rows as (out + c * ld) mod 16
// bytes does for int16, so the tiles, the classes and everything in front of
// the store pass are the same.
// (E is a parameter of its own, int16_t or uint8_t to match ENC: a signature
// that names the format words' unnamed enum would be mangled differently by
// the host and the device pass, and the launch would not find the kernel.)
template <int ENC, typename E>
__global__ void __launch_bounds__(kThreads)
tx_batch_kernel(const uint8_t* __restrict__ bits, const uint32_t* __restrict__ state,
                const float2* __restrict__ tab, E* __restrict__ out, long ld, int nch, int npk, int gap,
                int first, long tile0) {
    static_assert(sizeof(E) == (ENC == QPSK_OUT_S16 ? 2 : 1), "the element of the encoding");
    __shared__ __attribute__((aligned(16))) int16_t tile[2][kTile + 2 * kMargin];
    __shared__ uint32_t sgn[kLoop][2][kSignWords];
    const int tid = threadIdx.x;
    const int cls = blockIdx.x & (kClasses - 1);
    const long cbase = cls + (long)kClasses * kLoop * (blockIdx.x / kClasses);
    if (cbase >= nch) return;
    const int nloop = (int)lmin((long)kLoop, (nch - cbase + kClasses - 1) / kClasses);
    const long P = (long)kTxPacket + gap;
    const long N = (long)npk * P;
    // samples from the row's start back to a boundary of 8 elements: one value per class
    const unsigned a = (unsigned)(((uintptr_t)out / sizeof(E)) + (uint64_t)cbase * (uint64_t)ld) & (kChunk - 1);
    const long pl0 = (tile0 + blockIdx.y) * kTile - (long)a;   // the tile is [pl0, pl0 + kTile)
    const long pl = pl0 > 0 ? pl0 : 0, pe = lmin(pl0 + kTile, N);
    if (pl >= pe) return;
    // TX samples of the call at positions < p; the tile holds [tlo, thi)
    const long kl = pl / P, ke = pe / P;
    const long tlo = kl * kTxPacket + lmin(pl - kl * P, (long)kTxPacket);
    const long thi = ke * kTxPacket + lmin(pe - ke * P, (long)kTxPacket);
    const long slo = tlo / 5;                                  // first period of the tile
    const int nper = thi > tlo ? (int)((thi + 4) / 5 - slo) : 0;
    const long k0 = slo / kSymPacket;
    const int u0 = (int)(slo - k0 * kSymPacket);

    // gap positions stay zero for every channel: nothing writes them again
    for (int i = tid; i < (int)(sizeof(tile) / sizeof(uint32_t)); i += kThreads)
        reinterpret_cast<uint32_t*>(&tile[0][0])[i] = 0u;
    for (int i = tid; i < (int)(sizeof(sgn) / sizeof(uint32_t)); i += kThreads)
        (&sgn[0][0][0])[i] = 0u;
    __syncthreads();
    // sign bits: bit b of a channel's strings is symbol slo - 9 + b of the call.
    // A wave takes 64 symbols of one channel at a time (lane = symbol, so the
    // payload bytes are read once, side by side) and ballots them into two
    // words per component; kFetch of those are in flight together.
    const int ngrp = (nper + kHist + 63) >> 6;
    const int nitem = nloop * ngrp;
    auto fetch = [&](int item, bool& neg_i, bool& neg_q) {
        neg_i = neg_q = false;
        if (item >= nitem) return;
        const int i = item / ngrp, b = (item - i * ngrp) * 64 + (tid & 63);
        if (b >= nper + kHist) return;
        const long c = cbase + (long)kClasses * i;
        const int rel = u0 - kHist + b;                // symbol of packet k0, or its neighbours
        if (rel < 0 && k0 == 0) {                      // before this call: the saved 9 dibits
            if (!first) {
                const uint32_t st = state[c];
                neg_i = (st >> (rel + kHist)) & 1u;
                neg_q = (st >> (rel + kHist + 16)) & 1u;
            }
            return;
        }
        const int dk = rel < 0 ? -1 : rel / kSymPacket;
        const int u = rel - dk * kSymPacket;
        if (u < QK_NPRE) {
            constexpr unsigned long long lo = pre_neg(0), hi = pre_neg(1);
            neg_i = neg_q = ((u < 64 ? lo : hi) >> (u & 63)) & 1ull;
        } else {   // bits[2s] = Q, bits[2s+1] = I; 62 = 2*31, so data symbol d is bytes 2d, 2d+1
            const uint8_t* p = bits + ((size_t)c * npk + (size_t)(k0 + dk)) * kPacketBits +
                               2 * (u - QK_NPRE);
            neg_q = p[0] == 1;                         // qpsk_mod's `== 1`, src/qpsk.c:252-253
            neg_i = p[1] == 1;
        }
    };
    constexpr int kWaves = kThreads / 64, kFetch = 4;
    for (int it = tid >> 6; it < nitem; it += kWaves * kFetch) {
        bool ni[kFetch], nq[kFetch];
#pragma unroll
        for (int f = 0; f < kFetch; f++) fetch(it + f * kWaves, ni[f], nq[f]);
#pragma unroll
        for (int f = 0; f < kFetch; f++) {
            const int item = it + f * kWaves;
            const unsigned long long mi = __ballot(ni[f]), mq = __ballot(nq[f]);
            if ((tid & 63) == 0 && item < nitem) {
                const int i = item / ngrp, w = (item - i * ngrp) * 2;
                sgn[i][0][w] = (uint32_t)mi;
                sgn[i][0][w + 1] = (uint32_t)(mi >> 32);
                sgn[i][1][w] = (uint32_t)mq;
                sgn[i][1][w + 1] = (uint32_t)(mq >> 32);
            }
        }
    }

    // per period, independent of the channel
    float2 ph[kRounds][5];
    float scale[kRounds];
    int slot[kRounds];
    uint32_t live[kRounds];
#pragma unroll
    for (int rd = 0; rd < kRounds; rd++) {
        const int n = tid + rd * kThreads;
        scale[rd] = 0.0f;
        slot[rd] = 0;
        live[rd] = 0x3ffu;
#pragma unroll
        for (int jj = 0; jj < 5; jj++) ph[rd][jj] = make_float2(0.0f, 0.0f);
        if (n < nper) {
            const int rel = u0 + n;
            const int dk = rel / kSymPacket;
            const int u = rel - dk * kSymPacket;
            const long p = (k0 + dk) * P + 5 * u;
            slot[rd] = (int)(p - pl0) + kMargin;       // in [kMargin - 4, kMargin + kTile)
            scale[rd] = u < QK_NPRE ? 8192.0f : 16384.0f;
            const long S = slo + n;
            if (first && S < kHist) live[rd] = 0x3ffu & (0x3ffu << (kHist - (int)S));
#pragma unroll
            for (int jj = 0; jj < 5; jj++) ph[rd][jj] = tab[5 * S + jj];
        }
    }
    const bool zeros = first && slo < kHist;           // block-uniform: the stream's first 45 samples
    const long p0 = pl0 + (long)tid * kChunk;          // this lane's 8 samples in the store pass
    const bool whole = p0 >= 0 && p0 + kChunk <= N;
    __syncthreads();

    for (int i = 0; i < nloop; i++) {
        int16_t* buf = tile[i & 1];
#pragma unroll
        for (int rd = 0; rd < kRounds; rd++) {
            const int n = tid + rd * kThreads;
            if (n >= nper) continue;
            const uint32_t* wi = sgn[i][0];
            const uint32_t* wq = sgn[i][1];
            const uint32_t bi = __funnelshift_r(wi[n >> 5], wi[(n >> 5) + 1], n & 31);
            const uint32_t bq = __funnelshift_r(wq[n >> 5], wq[(n >> 5) + 1], n & 31);
            if (zeros) period<true>(bi, bq, live[rd], ph[rd], scale[rd], buf + slot[rd]);
            else period<false>(bi, bq, 0x3ffu, ph[rd], scale[rd], buf + slot[rd]);
        }
        __syncthreads();   // one barrier per channel: the other buffer's readers passed the last one
        E* row = out + (size_t)(cbase + (long)kClasses * i) * (size_t)ld;
        const int16_t* src = buf + kMargin + tid * kChunk;
        if constexpr (ENC == QPSK_OUT_S16) {
            if (whole) {
                *reinterpret_cast<uint4*>(row + p0) = *reinterpret_cast<const uint4*>(src);
            } else {
                for (int e = 0; e < kChunk; e++)
                    if (p0 + e >= 0 && p0 + e < N) row[p0 + e] = src[e];
            }
        } else {
            if (whole) {
                const uint4 v = *reinterpret_cast<const uint4*>(src);
                *reinterpret_cast<uint2*>(row + p0) = make_uint2(qfmt::encode4<ENC>(v.x, v.y), qfmt::encode4<ENC>(v.z, v.w));
            } else {
                for (int e = 0; e < kChunk; e++)
                    if (p0 + e >= 0 && p0 + e < N)
                        row[p0 + e] = (uint8_t)qfmt::encode<ENC>(src[e]);
            }
        }
    }
}

// The 9 dibits the next call's first packet filters over: data symbols
// 239..247 of this call's last packet.  Bit j = I sign, bit 16 + j = Q sign.
__global__ void __launch_bounds__(kThreads)
tx_state_kernel(const uint8_t* __restrict__ bits, uint32_t* __restrict__ state, int nch, int npk) {
    const long c = (long)blockIdx.x * kThreads + threadIdx.x;
    if (c >= nch) return;
    const uint8_t* p = bits + ((size_t)c * npk + (size_t)(npk - 1)) * kPacketBits +
                       2 * (kSymPacket - QK_NPRE - kHist);
    uint32_t st = 0;
    for (int j = 0; j < kHist; j++) {
        st |= (uint32_t)(p[2 * j + 1] == 1) << j;
        st |= (uint32_t)(p[2 * j] == 1) << (16 + j);
    }
    state[c] = st;
}

// data symbols 239..247 of a packet as a state word
__device__ inline uint32_t last_dibits(const uint8_t* __restrict__ packet) {
    const uint8_t* p = packet + 2 * (kSymPacket - QK_NPRE - kHist);
    uint32_t st = 0;
    for (int j = 0; j < kHist; j++) {
        st |= (uint32_t)(p[2 * j + 1] == 1) << j;
        st |= (uint32_t)(p[2 * j] == 1) << (16 + j);
    }
    return st;
}

// The plan pre-pass of a general context: a lane walks its channel's npk mask
// bytes once (active == nullptr: every slot active), writes the plan word of
// every slot, slot-major so that the lanes' stores lie side by side, and
// leaves the channel's new saved dibits and own index.  It takes the place of
// tx_state_kernel on this path.  Plain stores, no atomics, no block waits for
// another.
__global__ void __launch_bounds__(kThreads)
tx_plan_kernel(const uint8_t* __restrict__ bits, const uint8_t* __restrict__ active,
               uint32_t* __restrict__ state, uint64_t* __restrict__ index, uint32_t* __restrict__ plan,
               int nch, int npk) {
    const long c = (long)blockIdx.x * kThreads + threadIdx.x;
    if (c >= nch) return;
    uint64_t idx = index[c];
    uint32_t st = idx ? state[c] & kDibits : 0u;   // the word of a reset context may be stale
    for (int k = 0; k < npk; k++) {
        uint32_t w = 0;
        if (!active || active[(size_t)c * npk + k]) {
            const uint32_t row = idx < (uint64_t)(kCarrierRows - 1) ? (uint32_t)idx : (uint32_t)(kCarrierRows - 1);
            w = kPlanActive | (row << kPlanRowShift) | st;
            if (idx == 0) w |= kPlanStart;
            if (idx >= (uint64_t)kCarrierRows && (idx & 1)) w |= kPlanNeg;
            st = last_dibits(bits + ((size_t)c * npk + (size_t)k) * kPacketBits);
            idx++;
        }
        plan[(size_t)k * nch + c] = w;
    }
    state[c] = st;
    index[c] = idx;
}

// leaving the uniform state: every channel's own index is the context's count
__global__ void __launch_bounds__(kThreads)
tx_seed_kernel(uint64_t* __restrict__ index, int nch, uint64_t packets) {
    const long c = (long)blockIdx.x * kThreads + threadIdx.x;
    if (c < nch) index[c] = packets;
}

// tx_batch_kernel for a general context: the same tiles, classes, channel
// loop, LDS tile and store pass.  What was independent of the channel per
// period is now read per channel: a slot's plan word says whether the channel
// sends there (an idle slot's periods are written as zeros: the tile's two
// buffers are reused over the channel loop), whether the packet is the
// channel's first (the `live` mask of its first 9 periods), and which carrier
// row and sign it rides; the 5 carrier values come from the 9-row table (135 KB,
// resident in L2) instead of registers.  A packet's history symbols are the
// dibits of its own plan word, never the slot in front of it.
template <int ENC, typename E>
__global__ void __launch_bounds__(kThreads)
tx_mask_kernel(const uint8_t* __restrict__ bits, const uint32_t* __restrict__ plan,
               const float2* __restrict__ tab, E* __restrict__ out, long ld, int nch, int npk, int gap,
               long tile0) {
    static_assert(sizeof(E) == (ENC == QPSK_OUT_S16 ? 2 : 1), "the element of the encoding");
    __shared__ __attribute__((aligned(16))) int16_t tile[2][kTile + 2 * kMargin];
    __shared__ uint32_t sgn[kLoop][2][kSignWords];
    __shared__ uint32_t planw[kLoop][kPlanSlots];   // slots k0 .. k0 + 3 of each channel, 0 past the call
    const int tid = threadIdx.x;
    const int cls = blockIdx.x & (kClasses - 1);
    const long cbase = cls + (long)kClasses * kLoop * (blockIdx.x / kClasses);
    if (cbase >= nch) return;
    const int nloop = (int)lmin((long)kLoop, (nch - cbase + kClasses - 1) / kClasses);
    const long P = (long)kTxPacket + gap;
    const long N = (long)npk * P;
    const unsigned a = (unsigned)(((uintptr_t)out / sizeof(E)) + (uint64_t)cbase * (uint64_t)ld) & (kChunk - 1);
    const long pl0 = (tile0 + blockIdx.y) * kTile - (long)a;   // the tile is [pl0, pl0 + kTile)
    const long pl = pl0 > 0 ? pl0 : 0, pe = lmin(pl0 + kTile, N);
    if (pl >= pe) return;
    // as in tx_batch_kernel: every slot counts its 1880 TX samples, sent or not
    const long kl = pl / P, ke = pe / P;
    const long tlo = kl * kTxPacket + lmin(pl - kl * P, (long)kTxPacket);
    const long thi = ke * kTxPacket + lmin(pe - ke * P, (long)kTxPacket);
    const long slo = tlo / 5;
    const int nper = thi > tlo ? (int)((thi + 4) / 5 - slo) : 0;
    const long k0 = slo / kSymPacket;
    const int u0 = (int)(slo - k0 * kSymPacket);

    for (int i = tid; i < (int)(sizeof(tile) / sizeof(uint32_t)); i += kThreads)
        reinterpret_cast<uint32_t*>(&tile[0][0])[i] = 0u;
    for (int i = tid; i < (int)(sizeof(sgn) / sizeof(uint32_t)); i += kThreads)
        (&sgn[0][0][0])[i] = 0u;
    if (tid < kLoop * kPlanSlots) {
        const int i = tid / kPlanSlots, j = tid % kPlanSlots;
        const long k = k0 + j;
        planw[i][j] = i < nloop && k < npk ? plan[(size_t)k * nch + (size_t)(cbase + (long)kClasses * i)] : 0u;
    }
    __syncthreads();
    // sign bits: bit b of a channel's strings is symbol slo - 9 + b of the slots'
    // common time.  The last 9 symbols of a slot serve the next slot's first
    // periods as history, so there the next slot's plan word decides: its
    // dibits when that slot is active, else the slot's own payload.
    const int ngrp = (nper + kHist + 63) >> 6;
    const int nitem = nloop * ngrp;
    auto fetch = [&](int item, bool& neg_i, bool& neg_q) {
        neg_i = neg_q = false;
        if (item >= nitem) return;
        const int i = item / ngrp, b = (item - i * ngrp) * 64 + (tid & 63);
        if (b >= nper + kHist) return;
        const long c = cbase + (long)kClasses * i;
        const int rel = u0 - kHist + b;                // symbol of slot k0, or its neighbours
        const int dk = rel < 0 ? -1 : rel / kSymPacket;
        const int u = rel - dk * kSymPacket;
        if (u >= kSymPacket - kHist) {
            const uint32_t wn = planw[i][dk + 1];
            if (wn & kPlanActive) {
                const int j = u - (kSymPacket - kHist);
                neg_i = (wn >> j) & 1u;
                neg_q = (wn >> (j + 16)) & 1u;
                return;
            }
        }
        if (dk < 0 || !(planw[i][dk] & kPlanActive)) return;   // idle: its bits row is not read
        if (u < QK_NPRE) {
            constexpr unsigned long long lo = pre_neg(0), hi = pre_neg(1);
            neg_i = neg_q = ((u < 64 ? lo : hi) >> (u & 63)) & 1ull;
        } else {
            const uint8_t* p = bits + ((size_t)c * npk + (size_t)(k0 + dk)) * kPacketBits +
                               2 * (u - QK_NPRE);
            neg_q = p[0] == 1;
            neg_i = p[1] == 1;
        }
    };
    constexpr int kWaves = kThreads / 64, kFetch = 4;
    for (int it = tid >> 6; it < nitem; it += kWaves * kFetch) {
        bool ni[kFetch], nq[kFetch];
#pragma unroll
        for (int f = 0; f < kFetch; f++) fetch(it + f * kWaves, ni[f], nq[f]);
#pragma unroll
        for (int f = 0; f < kFetch; f++) {
            const int item = it + f * kWaves;
            const unsigned long long mi = __ballot(ni[f]), mq = __ballot(nq[f]);
            if ((tid & 63) == 0 && item < nitem) {
                const int i = item / ngrp, w = (item - i * ngrp) * 2;
                sgn[i][0][w] = (uint32_t)mi;
                sgn[i][0][w + 1] = (uint32_t)(mi >> 32);
                sgn[i][1][w] = (uint32_t)mq;
                sgn[i][1][w + 1] = (uint32_t)(mq >> 32);
            }
        }
    }

    // per period, independent of the channel: where it lies, not what it carries
    float scale[kRounds];
    int slot[kRounds], sym[kRounds], dks[kRounds];
#pragma unroll
    for (int rd = 0; rd < kRounds; rd++) {
        const int n = tid + rd * kThreads;
        scale[rd] = 0.0f;
        slot[rd] = sym[rd] = dks[rd] = 0;
        if (n < nper) {
            const int rel = u0 + n;
            const int dk = rel / kSymPacket;
            const int u = rel - dk * kSymPacket;
            const long p = (k0 + dk) * P + 5 * u;
            slot[rd] = (int)(p - pl0) + kMargin;       // in [kMargin - 4, kMargin + kTile)
            scale[rd] = u < QK_NPRE ? 8192.0f : 16384.0f;
            sym[rd] = u;
            dks[rd] = dk;
        }
    }
    const long p0 = pl0 + (long)tid * kChunk;          // this lane's 8 samples in the store pass
    const bool whole = p0 >= 0 && p0 + kChunk <= N;
    __syncthreads();

    for (int i = 0; i < nloop; i++) {
        int16_t* buf = tile[i & 1];
#pragma unroll
        for (int rd = 0; rd < kRounds; rd++) {
            const int n = tid + rd * kThreads;
            if (n >= nper) continue;
            int16_t* dst = buf + slot[rd];
            const uint32_t w = planw[i][dks[rd]];
            if (!(w & kPlanActive)) {                  // an idle slot: the buffer held another channel
#pragma unroll
                for (int jj = 0; jj < 5; jj++) dst[jj] = 0;
                continue;
            }
            // A negated carrier negates sr exactly (both products change sign, and
            // so does their rounded difference), and (-sr) * scale is sr * -scale
            // bit for bit: the sign rides the scale.
            const float2* tp = tab + ((w >> kPlanRowShift) & 15u) * (uint32_t)kTxPacket + 5 * sym[rd];
            const float sc = (w & kPlanNeg) ? -scale[rd] : scale[rd];
            float2 ph[5];
#pragma unroll
            for (int jj = 0; jj < 5; jj++) ph[jj] = tp[jj];
            const uint32_t* wi = sgn[i][0];
            const uint32_t* wq = sgn[i][1];
            const uint32_t bi = __funnelshift_r(wi[n >> 5], wi[(n >> 5) + 1], n & 31);
            const uint32_t bq = __funnelshift_r(wq[n >> 5], wq[(n >> 5) + 1], n & 31);
            if ((w & kPlanStart) && sym[rd] < kHist)   // the stream's first 45 samples
                period<true>(bi, bq, 0x3ffu & (0x3ffu << (kHist - sym[rd])), ph, sc, dst);
            else
                period<false>(bi, bq, 0x3ffu, ph, sc, dst);
        }
        __syncthreads();   // one barrier per channel: the other buffer's readers passed the last one
        E* row = out + (size_t)(cbase + (long)kClasses * i) * (size_t)ld;
        const int16_t* src = buf + kMargin + tid * kChunk;
        if constexpr (ENC == QPSK_OUT_S16) {
            if (whole) {
                *reinterpret_cast<uint4*>(row + p0) = *reinterpret_cast<const uint4*>(src);
            } else {
                for (int e = 0; e < kChunk; e++)
                    if (p0 + e >= 0 && p0 + e < N) row[p0 + e] = src[e];
            }
        } else {
            if (whole) {
                const uint4 v = *reinterpret_cast<const uint4*>(src);
                *reinterpret_cast<uint2*>(row + p0) = make_uint2(qfmt::encode4<ENC>(v.x, v.y), qfmt::encode4<ENC>(v.z, v.w));
            } else {
                for (int e = 0; e < kChunk; e++)
                    if (p0 + e >= 0 && p0 + e < N)
                        row[p0 + e] = (uint8_t)qfmt::encode<ENC>(src[e]);
            }
        }
    }
}

// an allocation the device refused is QPSK_ENOMEM to the transmitter's callers
int enomem(int r) { return r == QPSK_EHIP - (int)hipErrorOutOfMemory ? QPSK_ENOMEM : r; }

}  // namespace

struct qpsk_tx_ctx {
    int device = 0, nch = 0, gap = 0;
    uint64_t packets = 0;
    float phase[2] = {1.0f, 0.0f};    // fbb_tx_phase before the next packet
    qhip::Stream stream;              // qpsk_tx_batch's own (first: released last)
    qhip::DevBuf<uint32_t> d_state;   // [nch] last 9 dibits sent
    qhip::DevBuf<float2> d_tab;       // carrier of the current call's TX samples
    // pinned staging of the carrier table: two slots, so a call never waits for
    // the previous call's kernel before it builds its own table
    qhip::PinBuf<float> h_stage[2];      // (re, im) pairs
    qhip::Event ev_stage[2];          // the slot's upload has been read
    int slot = 0;
    qhip::Event ev_last;              // after the latest call's kernels
    // the modulator's int16 block of calls in another output format
    // (qpsk_output.hip on qpsk_tx_fmt_conv); empty until such a call
    qhip::DevBuf<int16_t> d_conv;
    // Channels that come and go.  uniform: every channel at `packets`, the
    // per-call carrier table and tx_batch_kernel.  Otherwise the own indices
    // are d_index, and the calls go through tx_plan_kernel and tx_mask_kernel.
    // All of it stays empty on a context that never leaves the uniform state.
    bool uniform = true;
    qhip::DevBuf<uint64_t> d_index;   // [nch] own packet index
    qhip::DevBuf<float2> d_rows;      // the 9 carrier rows, uploaded once
    qhip::PinBuf<float> h_rows;       // their staging: an upload may still be pending
    qhip::DevBuf<uint32_t> d_plan;    // [npackets][nch] plan words of the current call
};

extern "C" qpsk_tx_ctx* qpsk_tx_create(int device, int nch, int gap, int* err) {
    if (nch < 1 || gap < 0) return qhip::fail(err, QPSK_EINVAL);
    if (!qhip::device_ok(device)) return qhip::fail(err, QPSK_ENODEV);
    qpsk_tx_ctx* c = new (std::nothrow) qpsk_tx_ctx();
    if (!c) return qhip::fail(err, QPSK_ENOMEM);
    c->device = device;
    c->nch = nch;
    c->gap = gap;
    int r = herr(hipSetDevice(device));
    if (r == QPSK_OK) r = herr(c->stream.create());
    if (r == QPSK_OK) r = herr(c->d_state.reserve((size_t)nch));
    if (r == QPSK_OK) r = herr(hipMemset(c->d_state, 0, sizeof(uint32_t) * (size_t)nch));
    for (int s = 0; s < 2 && r == QPSK_OK; s++) r = herr(c->ev_stage[s].create(hipEventDisableTiming));
    if (r == QPSK_OK) r = herr(c->ev_last.create(hipEventDisableTiming));
    if (r != QPSK_OK) {
        qpsk_tx_destroy(c);
        return qhip::fail(err, enomem(r));
    }
    qhip::set_err(err, QPSK_OK);
    return c;
}

extern "C" void qpsk_tx_destroy(qpsk_tx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->ev_last) (void)hipEventSynchronize(c->ev_last);
    for (int s = 0; s < 2; s++)
        if (c->ev_stage[s]) (void)hipEventSynchronize(c->ev_stage[s]);
    delete c;
}

extern "C" int qpsk_tx_sync(qpsk_tx_ctx* c) {
    if (!c) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    HCHECK(hipEventSynchronize(c->ev_last));
    return QPSK_OK;
}

extern "C" int qpsk_tx_reset(qpsk_tx_ctx* c) {
    const int r = qpsk_tx_sync(c);
    if (r != QPSK_OK) return r;
    c->packets = 0;   // the saved dibits are not read before the first packet
    c->phase[0] = 1.0f;
    c->phase[1] = 0.0f;
    c->uniform = true;   // own indices are seeded again when the context next leaves this state
    return QPSK_OK;
}

extern "C" int qpsk_tx_channels(const qpsk_tx_ctx* c) { return c ? c->nch : QPSK_EINVAL; }
extern "C" int qpsk_tx_gap(const qpsk_tx_ctx* c) { return c ? c->gap : QPSK_EINVAL; }
extern "C" uint64_t qpsk_tx_packets(const qpsk_tx_ctx* c) { return c ? c->packets : 0; }

// the hooks of the output formats (qpsk_tx_internal.h)
extern "C" int qpsk_tx_device(const qpsk_tx_ctx* c) { return c ? c->device : QPSK_EINVAL; }
extern "C" void* qpsk_tx_host_stream(const qpsk_tx_ctx* c) { return c ? (hipStream_t)c->stream : nullptr; }

extern "C" int qpsk_tx_fmt_conv(qpsk_tx_ctx* c, size_t n, int16_t** p) {
    if (!c || !p) return QPSK_EINVAL;
    HCHECK(hipSetDevice(c->device));
    if (n > c->d_conv.cap()) {
        HCHECK(hipDeviceSynchronize());   // an earlier call may still use the block
        const int r = herr(c->d_conv.reserve(n));
        if (r != QPSK_OK) return enomem(r);
    }
    *p = c->d_conv;
    return QPSK_OK;
}

extern "C" int qpsk_tx_mark(qpsk_tx_ctx* c, void* stream) {
    if (!c) return QPSK_EINVAL;
    HCHECK(hipEventRecord(c->ev_last, (hipStream_t)stream));
    return QPSK_OK;
}

static int tx_check(const qpsk_tx_ctx* c, const void* bits, int npackets, const void* out, long ld) {
    if (!c || npackets < 0) return QPSK_EINVAL;
    if (npackets == 0) return QPSK_OK;
    if (!bits || !out || (long)c->nch * npackets >= QPSK_TX_MAX_CHANNEL_PACKETS ||
        ld < (long)npackets * ((long)kTxPacket + c->gap))
        return QPSK_EINVAL;
    return QPSK_OK;
}

static dim3 chan_grid(int nch) { return dim3((unsigned)((nch + kThreads - 1) / kThreads)); }

// Leaving the uniform state, in stream order on s: the carrier rows (once per
// context) and every channel's own index = the context's count.
static int tx_leave_uniform(qpsk_tx_ctx* c, hipStream_t s) {
    if (!c->uniform) return QPSK_OK;
    HCHECK(c->d_index.reserve((size_t)c->nch));
    if (!c->d_rows) {
        constexpr long n = (long)kCarrierRows * kTxPacket;
        HCHECK(c->d_rows.reserve((size_t)n));
        HCHECK(c->h_rows.reserve(2 * (size_t)n));
        qpsk_tx_phase_table(c->h_rows, n);
        HCHECK(hipMemcpyAsync(c->d_rows, c->h_rows, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(tx_seed_kernel, chan_grid(c->nch), dim3(kThreads), 0, s, c->d_index.get(), c->nch,
                       c->packets);
    HCHECK(hipGetLastError());
    c->uniform = false;
    return QPSK_OK;
}

// A call of a general context: the plan pre-pass, then the modulator over it.
static int tx_general(qpsk_tx_ctx* c, const uint8_t* d_bits, const uint8_t* d_active, int npackets, void* d_out,
                      long ld, hipStream_t s, int enc) {
    const int r = tx_leave_uniform(c, s);
    if (r != QPSK_OK) return r;
    const size_t nplan = (size_t)c->nch * (size_t)npackets;
    if (nplan > c->d_plan.cap()) {   // the release waits for the kernels that read the old plan
        HCHECK(c->d_plan.release());
        HCHECK(c->d_plan.reserve(nplan));
    }
    hipLaunchKernelGGL(tx_plan_kernel, chan_grid(c->nch), dim3(kThreads), 0, s, d_bits, d_active,
                       c->d_state.get(), c->d_index.get(), c->d_plan.get(), c->nch, npackets);
    HCHECK(hipGetLastError());
    const long N = (long)npackets * ((long)kTxPacket + c->gap);
    const long ntile = (N + (kChunk - 1) + kTile - 1) / kTile;
    const unsigned gx = (unsigned)(kClasses * (((long)c->nch + kClasses * kLoop - 1) / (kClasses * kLoop)));
    for (long t0 = 0; t0 < ntile; t0 += 65535) {
        const dim3 grid(gx, (unsigned)lmin(65535L, ntile - t0)), block(kThreads);
        const uint32_t* plan = c->d_plan.get();
        const float2* rows = c->d_rows.get();
        qfmt::with_encoding(enc, [&](auto e) {
            using E = std::conditional_t<e() == QPSK_OUT_S16, int16_t, uint8_t>;
            hipLaunchKernelGGL((tx_mask_kernel<e(), E>), grid, block, 0, s, d_bits, plan, rows,
                               static_cast<E*>(d_out), ld, c->nch, npackets, c->gap, t0);
        });
        HCHECK(hipGetLastError());
    }
    HCHECK(hipEventRecord(c->ev_last, s));
    c->packets += (uint64_t)npackets;
    return QPSK_OK;
}

// A call of a uniform context: the carrier of the call's samples from the
// host, tx_batch_kernel, and tx_state_kernel for the next call's history.
static int tx_uniform(qpsk_tx_ctx* c, const uint8_t* d_bits, int npackets, void* d_out, long ld, hipStream_t s,
                      int enc) {
    const long ntx = (long)npackets * kTxPacket;
    if ((size_t)ntx > c->d_tab.cap()) {   // the release waits for the kernels that read the old table
        HCHECK(c->d_tab.release());
        HCHECK(c->d_tab.reserve((size_t)ntx));
    }
    const int sl = c->slot;
    HCHECK(hipEventSynchronize(c->ev_stage[sl]));   // the slot's previous upload (two calls ago)
    if (2 * (size_t)ntx > c->h_stage[sl].cap()) {
        HCHECK(c->h_stage[sl].release());
        HCHECK(c->h_stage[sl].reserve(2 * (size_t)ntx));
    }
    // the carrier of this call's packets, continued from the carried phase; the
    // context takes the new phase only once everything is enqueued
    float ph[2] = {c->phase[0], c->phase[1]};
    qpsk_tx_phase_run(c->h_stage[sl], ntx, ph);
    HCHECK(hipMemcpyAsync(c->d_tab, c->h_stage[sl], sizeof(float2) * (size_t)ntx, hipMemcpyHostToDevice, s));
    HCHECK(hipEventRecord(c->ev_stage[sl], s));
    c->slot = sl ^ 1;
    const long N = (long)npackets * ((long)kTxPacket + c->gap);
    const long ntile = (N + (kChunk - 1) + kTile - 1) / kTile;   // the class with the longest head
    const unsigned gx = (unsigned)(kClasses * (((long)c->nch + kClasses * kLoop - 1) / (kClasses * kLoop)));
    const int first = c->packets == 0;
    for (long t0 = 0; t0 < ntile; t0 += 65535) {
        const unsigned gy = (unsigned)lmin(65535L, ntile - t0);
        const dim3 grid(gx, gy), block(kThreads);
        const float2* tab = c->d_tab.get();
        qfmt::with_encoding(enc, [&](auto e) {
            using E = std::conditional_t<e() == QPSK_OUT_S16, int16_t, uint8_t>;
            hipLaunchKernelGGL((tx_batch_kernel<e(), E>), grid, block, 0, s, d_bits, c->d_state, tab,
                               static_cast<E*>(d_out), ld, c->nch, npackets, c->gap, first, t0);
        });
        HCHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(tx_state_kernel, dim3((unsigned)((c->nch + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, d_bits, c->d_state, c->nch, npackets);
    HCHECK(hipGetLastError());
    HCHECK(hipEventRecord(c->ev_last, s));
    c->phase[0] = ph[0];
    c->phase[1] = ph[1];
    c->packets += (uint64_t)npackets;
    return QPSK_OK;
}

// qpsk_tx_batch_masked_device with the element the store pass writes named:
// d_out is int16 [nch][ld] for QPSK_OUT_S16 and uint8 [nch][ld] G.711 codes for
// QPSK_OUT_ALAW / QPSK_OUT_ULAW (qpsk_tx_internal.h).  A NULL mask on a uniform
// context is the plain call and keeps the context uniform.
extern "C" int qpsk_tx_batch_masked_device_enc(qpsk_tx_ctx* c, const uint8_t* d_bits, const uint8_t* d_active,
                                               int npackets, void* d_out, long ld, void* stream, int enc) {
    if (enc != QPSK_OUT_S16 && enc != QPSK_OUT_ALAW && enc != QPSK_OUT_ULAW) return QPSK_EINVAL;
    const int chk = tx_check(c, d_bits, npackets, d_out, ld);
    if (chk != QPSK_OK || npackets == 0) return chk;
    HCHECK(hipSetDevice(c->device));
    if (c->uniform && !d_active) return tx_uniform(c, d_bits, npackets, d_out, ld, (hipStream_t)stream, enc);
    return enomem(tx_general(c, d_bits, d_active, npackets, d_out, ld, (hipStream_t)stream, enc));
}

extern "C" int qpsk_tx_batch_device_enc(qpsk_tx_ctx* c, const uint8_t* d_bits, int npackets, void* d_out,
                                        long ld, void* stream, int enc) {
    return qpsk_tx_batch_masked_device_enc(c, d_bits, nullptr, npackets, d_out, ld, stream, enc);
}

extern "C" int qpsk_tx_batch_device(qpsk_tx_ctx* c, const uint8_t* d_bits, int npackets,
                                    int16_t* d_out, long ld, void* stream) {
    return qpsk_tx_batch_masked_device_enc(c, d_bits, nullptr, npackets, d_out, ld, stream, QPSK_OUT_S16);
}

extern "C" int qpsk_tx_batch_masked_device(qpsk_tx_ctx* c, const uint8_t* d_bits, const uint8_t* d_active,
                                           int npackets, int16_t* d_out, long ld, void* stream) {
    return qpsk_tx_batch_masked_device_enc(c, d_bits, d_active, npackets, d_out, ld, stream, QPSK_OUT_S16);
}

// ---------------------------------------------------------------- channels on their own
static int range_check(const qpsk_tx_ctx* c, int c0, int n) {
    return c && c0 >= 0 && n >= 0 && c0 <= c->nch && n <= c->nch - c0 ? QPSK_OK : QPSK_EINVAL;
}

extern "C" int qpsk_tx_reset_channels(qpsk_tx_ctx* c, int c0, int n) {
    if (range_check(c, c0, n) != QPSK_OK) return QPSK_EINVAL;
    int r = qpsk_tx_sync(c);
    if (r != QPSK_OK || n == 0) return r;
    r = tx_leave_uniform(c, c->stream);
    if (r != QPSK_OK) return enomem(r);
    HCHECK(hipMemsetAsync(c->d_index.get() + c0, 0, sizeof(uint64_t) * (size_t)n, c->stream));
    HCHECK(hipMemsetAsync(c->d_state.get() + c0, 0, sizeof(uint32_t) * (size_t)n, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    return QPSK_OK;
}

// own indices and canonical state words of [c0, c0 + n) after the calls in flight
static int tx_read_state(qpsk_tx_ctx* c, int c0, int n, uint64_t* idx, uint32_t* words) {
    const int r = qpsk_tx_sync(c);
    if (r != QPSK_OK) return r;
    if (c->uniform) {
        for (int i = 0; i < n; i++) idx[i] = c->packets;
    } else {
        HCHECK(hipMemcpy(idx, c->d_index.get() + c0, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    if (!words) return QPSK_OK;
    HCHECK(hipMemcpy(words, c->d_state.get() + c0, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) words[i] = idx[i] ? words[i] & kDibits : 0u;   // not read before a first packet
    return QPSK_OK;
}

extern "C" int qpsk_tx_channel_packets(qpsk_tx_ctx* c, int c0, int n, uint64_t* out) {
    if (range_check(c, c0, n) != QPSK_OK || (n > 0 && !out)) return QPSK_EINVAL;
    if (n == 0) return qpsk_tx_sync(c);
    return tx_read_state(c, c0, n, out, nullptr);
}

namespace {
constexpr uint32_t kSnapMagic = 0x53585451u, kSnapVersion = 1u;   // "QTXS"
constexpr size_t kSnapHeader = 16;
}  // namespace

extern "C" size_t qpsk_tx_state_size(int n) { return n < 1 ? 0 : kSnapHeader + 12 * (size_t)n; }

extern "C" int qpsk_tx_state_save(qpsk_tx_ctx* c, int c0, int n, void* buf, size_t size) {
    if (range_check(c, c0, n) != QPSK_OK || n < 1 || !buf || size < qpsk_tx_state_size(n)) return QPSK_EINVAL;
    uint64_t* idx = (uint64_t*)malloc(12 * (size_t)n);
    if (!idx) return QPSK_ENOMEM;
    uint32_t* words = (uint32_t*)(idx + n);
    const int r = tx_read_state(c, c0, n, idx, words);
    if (r == QPSK_OK) {
        const uint32_t head[4] = {kSnapMagic, kSnapVersion, (uint32_t)n, 0u};
        memcpy(buf, head, kSnapHeader);
        memcpy((char*)buf + kSnapHeader, idx, 12 * (size_t)n);   // the indices, then the words
    }
    free(idx);
    return r;
}

extern "C" int qpsk_tx_state_load(qpsk_tx_ctx* c, int c0, int n, const void* buf, size_t size) {
    if (range_check(c, c0, n) != QPSK_OK || n < 1 || !buf || size < qpsk_tx_state_size(n)) return QPSK_EINVAL;
    uint32_t head[4];
    memcpy(head, buf, kSnapHeader);
    if (head[0] != kSnapMagic || head[1] != kSnapVersion || head[2] != (uint32_t)n || head[3] != 0u)
        return QPSK_EINVAL;
    uint64_t* idx = (uint64_t*)malloc(12 * (size_t)n);
    if (!idx) return QPSK_ENOMEM;
    uint32_t* words = (uint32_t*)(idx + n);
    memcpy(idx, (const char*)buf + kSnapHeader, 12 * (size_t)n);
    int r = QPSK_OK;
    for (int i = 0; i < n; i++)
        if ((words[i] & ~kDibits) || (!idx[i] && words[i])) r = QPSK_EINVAL;
    if (r == QPSK_OK) r = qpsk_tx_sync(c);
    if (r == QPSK_OK) {
        r = enomem(tx_leave_uniform(c, c->stream));
        if (r == QPSK_OK)
            r = herr(hipMemcpyAsync(c->d_index.get() + c0, idx, sizeof(uint64_t) * (size_t)n,
                                    hipMemcpyHostToDevice, c->stream));
        if (r == QPSK_OK)
            r = herr(hipMemcpyAsync(c->d_state.get() + c0, words, sizeof(uint32_t) * (size_t)n,
                                    hipMemcpyHostToDevice, c->stream));
        const int r2 = herr(hipStreamSynchronize(c->stream));   // idx is freed below
        if (r == QPSK_OK) r = r2;
    }
    free(idx);
    return r;
}

extern "C" int qpsk_tx_batch(qpsk_tx_ctx* c, const uint8_t* bits, int npackets, int16_t* out, long ld) {
    return qpsk_tx_batch_masked(c, bits, nullptr, npackets, out, ld);
}

extern "C" int qpsk_tx_batch_masked(qpsk_tx_ctx* c, const uint8_t* bits, const uint8_t* active, int npackets,
                                    int16_t* out, long ld) {
    const int chk = tx_check(c, bits, npackets, out, ld);
    if (chk != QPSK_OK || npackets == 0) return chk;
    HCHECK(hipSetDevice(c->device));
    // A device call still pending on a caller's stream leaves the 9 dibits this
    // call filters over and reads the carrier table this call replaces; the
    // context's own stream cannot be chained behind it from outside.
    HCHECK(hipEventSynchronize(c->ev_last));
    const size_t nbits = (size_t)c->nch * (size_t)npackets * kPacketBits;
    const size_t N = (size_t)npackets * (size_t)(kTxPacket + (long)c->gap);
    const size_t nact = active ? (size_t)c->nch * (size_t)npackets : 0;
    qhip::DevBuf<uint8_t> d_bits, d_active;   // released on return, after the synchronisation
    qhip::DevBuf<int16_t> d_out;
    int r = herr(d_bits.reserve(nbits));
    if (r == QPSK_OK) r = herr(d_active.reserve(nact));
    if (r == QPSK_OK) r = herr(d_out.reserve(N * (size_t)c->nch));
    if (r == QPSK_OK) r = herr(hipMemcpyAsync(d_bits, bits, nbits, hipMemcpyHostToDevice, c->stream));
    if (r == QPSK_OK && active) r = herr(hipMemcpyAsync(d_active, active, nact, hipMemcpyHostToDevice, c->stream));
    if (r == QPSK_OK) r = qpsk_tx_batch_masked_device(c, d_bits, d_active, npackets, d_out, (long)N, c->stream);
    // only the written samples come back: out[c][N .. ld) keeps its contents
    if (r == QPSK_OK)
        r = herr(hipMemcpy2DAsync(out, sizeof(int16_t) * (size_t)ld, d_out, sizeof(int16_t) * N,
                                  sizeof(int16_t) * N, (size_t)c->nch, hipMemcpyDeviceToHost, c->stream));
    const int r2 = herr(hipStreamSynchronize(c->stream));
    if (r == QPSK_OK) r = r2;
    return enomem(r);
}
