// qpsk_rx_front.h -- the front wave of the receive kernels: prefetch, mixer,
// the three FIRs, the preamble hunt, the window store, and
// the head pre-pass kernel (included by qpsk_rx.hip only).
#pragma once

#include <utility>

#include "qpsk_fft_dev.h"
#include "qpsk_rx_dev.h"
#include "qpsk_split.h"

#pragma clang fp contract(off)

namespace {

constexpr int kFirBatch = 15;   // FIR samples per LDS batch (fir_dec, fir_dec752, fir_split)

// ---------------------------------------------------------------- front wave
// Input of one channel for frame n: kM/2 two-sample items d, item d -> M[2d..2d+1]:
// MODE 0 (696 items):
//   d <  24 : x_{n-2}[1832 + 2d]          d < 620 : x_{n-1}[2(d-24)]
//   d < 644 : x_{n-1}[1832 + 2(d-620)]    d < 696 : x_n[2(d-644)]
// MODE 1 (875 items):
//   d <  24 : x_{n-2}[1832 + 2d]          d < 875 : x_{n-1}[2(d-24)]
// Lane l owns items l + 64i, i < kPf; i is a compile-time constant below.
template <int MODE> constexpr int kItems = Cfg<MODE>::kM / 2;
template <int MODE> constexpr int kPf = (kItems<MODE> + 63) / 64;   // 11 / 14 dwords per lane

struct Src {
    const int16_t* xm2;
    const int16_t* xm1;
    const int16_t* x0;
};

__device__ __forceinline__ Src srcs(const RxArgs& a, int ch, int n) {
    return {frame_ptr(a, ch, n - 2), frame_ptr(a, ch, n - 1), frame_ptr(a, ch, n)};
}

// which frame (0: x_{n-2}, 1: x_{n-1}, 2: x_n; -1: none) and sample index of item l + 64i
template <int MODE, int i>
__device__ __forceinline__ constexpr int item(int lane, int& t) {
    const int d = lane + 64 * i;
    if (i == 0) {
        if (lane < 24) { t = 1832 + 2 * lane; return 0; }
        t = 2 * (lane - 24);
        return 1;
    }
    if (MODE == 1) {
        if (d < kItems<1>) { t = 2 * (d - 24); return 1; }
        t = 0;
        return -1;
    }
    if (i < 9) { t = 2 * (d - 24); return 1; }
    if (i == 9) { t = d < 620 ? 2 * (d - 24) : 1832 + 2 * (d - 620); return 1; }
    if (d < 644) { t = 1832 + 2 * (d - 620); return 1; }
    if (d < kItems<0>) { t = 2 * (d - 644); return 2; }
    t = 0;
    return -1;
}

// CG: the three frames are consecutive rows of `in` (frame n >= 2): items 0
// and 10 (MODE 0), which take each lane's sample from one of two frames, are
// then addressed from one wave-uniform base with a 32-bit lane offset instead
// of a per-lane 64-bit pointer, which the quad-back kernels kept live across
// the channel loop and spilled; its reload waited for every load in flight,
// this prefetch included (profiles/r03_prefetch_ab.txt)
template <int MODE, int i, bool CG>
__device__ __forceinline__ void load_item(const Src& s, int lane, int& r) {
    int t;
    const int f = item<MODE, i>(lane, t);
    if constexpr (CG) {
        if (f >= 0) r = *reinterpret_cast<const int*>(s.xm2 + (unsigned)(f * QK_FRAME + t));
    } else {
        if (f >= 0) r = *reinterpret_cast<const int*>((f == 0 ? s.xm2 : f == 1 ? s.xm1 : s.x0) + t);
    }
}

template <int MODE, bool CG, int... I>
__device__ __forceinline__ void prefetch_seq(const Src& s, int lane, int (&r)[kPf<MODE>],
                                             std::integer_sequence<int, I...>) {
    (load_item<MODE, I, CG>(s, lane, r[I]), ...);
}

// the lane index, laundered: per-lane item offsets and signs derived from it are
// recomputed at each use (a few VALU) instead of being hoisted out of the
// channel loop as live registers
__device__ __forceinline__ int fresh_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

template <int MODE, bool CG = false, int FR = 0>
__device__ __forceinline__ void prefetch(const Src& s, int lane, int (&r)[kPf<MODE>]) {
    prefetch_seq<MODE, CG>(s, (FR & 1) ? fresh_lane(lane) : lane, r, std::make_integer_sequence<int, kPf<MODE>>{});
}

// MODE 0, frame n >= 2 of a call, for the 4x2 split kernel: x_{n-2}, x_{n-1}
// and x_n are consecutive rows of `in`, and there item()'s pieces meet (x_{n-2}
// [1880 + k] is x_{n-1}[k]): item d starts 1832 + 2d samples into row x_{n-2}
// for d < 620 and 640 samples (1280 B) further for d >= 620.  So all 11 loads
// take one wave-uniform base, `mid` (item 5's first sample: every constant then
// fits a load's 13-bit immediate), one lane offset, and for item 9, whose
// lanes straddle d = 620, a second one.
constexpr int row_item(int d) { return 1832 + 2 * d + (d < 620 ? 0 : 640); }
template <int i>
constexpr bool row_item_is_item() {
    for (int l = 0; l < 64; l++) {
        int t = 0;
        const int f = item<0, i>(l, t);
        if (f >= 0 && f * QK_FRAME + t != row_item(l + 64 * i)) return false;
        if ((f >= 0) != (l + 64 * i < kItems<0>)) return false;
    }
    return true;
}
template <int... I>
constexpr bool row_items_are_items(std::integer_sequence<int, I...>) {
    return (row_item_is_item<I>() && ...);
}
static_assert(row_items_are_items(std::make_integer_sequence<int, kPf<0>>{}), "prefetch_rows: item()'s samples");
template <int FR>
__device__ __forceinline__ void prefetch_rows(const int16_t* xm2, int lane, int (&r)[kPf<0>]) {
    if (FR & 1) lane = fresh_lane(lane);
    typedef __attribute__((address_space(1))) const char gchar;   // global memory, as `in` is
    typedef __attribute__((address_space(1))) const int gint;
    unsigned long long m = reinterpret_cast<unsigned long long>(xm2 + row_item(64 * 5));
    asm volatile("" : "+s"(m));   // kept as the loads' scalar base: the constants below stay immediates
    gchar* mid = reinterpret_cast<gchar*>(m);
    const unsigned v = 4u * (unsigned)lane;
    const unsigned v9 = v + (lane < 620 - 64 * 9 ? 0u : 1280u);
    auto ld = [&](unsigned voff, int imm) { return *reinterpret_cast<gint*>(mid + imm + voff); };
#pragma unroll
    for (int i = 0; i < 9; i++) r[i] = ld(v, 256 * (i - 5));
    r[9] = ld(v9, 1024);
    if (lane < kItems<0> - 640) r[10] = ld(v, 2560);
}

// src/qpsk.c:139-144 as (-1)^G * P[t] * (x * 2^-14), two samples per item.
// NO: frame g-1 (f == 1) is the negated one (then g-2 and g are not).  Items
// 1..9 (MODE 0) / 1..13 (MODE 1) hold frame g-1 in every lane, so their sign is
// a compile-time negation (a free source modifier); items 0 and 10 (MODE 0)
// straddle two frames per lane.
template <int MODE, int i, bool NO>
__device__ __forceinline__ void mix_item(int lane, int r, const float2* P, float2* M) {
    int t;
    const int f = item<MODE, i>(lane, t);
    if (f < 0) return;
    const float4 p = *reinterpret_cast<const float4*>(P + t);
    const float v0 = (float)(int16_t)(r & 0xffff);
    const float v1 = (float)(int16_t)(r >> 16);
    float4 o;
    constexpr bool kAllPrev = MODE == 1 ? i >= 1 : (i >= 1 && i <= 9);
    if (kAllPrev) {
        o = NO ? make_float4((-p.x) * v0, (-p.y) * v0, (-p.z) * v1, (-p.w) * v1)
               : make_float4(p.x * v0, p.y * v0, p.z * v1, p.w * v1);
    } else {
        const float sg = ((f == 1) == NO) ? -1.0f : 1.0f;   // exact sign flip
        o = make_float4((sg * p.x) * v0, (sg * p.y) * v0, (sg * p.z) * v1, (sg * p.w) * v1);
    }
    *reinterpret_cast<float4*>(M + 2 * (lane + 64 * i)) = o;
}

template <int MODE, bool NO, int... I>
__device__ __forceinline__ void mix_seq(int lane, const int (&r)[kPf<MODE>], const float2* P,
                                        float2* M, std::integer_sequence<int, I...>) {
    (mix_item<MODE, I, NO>(lane, r[I], P, M), ...);
}

template <int MODE, int FR = 0>
__device__ __forceinline__ void mix(int lane, const int (&r)[kPf<MODE>], unsigned g,
                                    const float2* P, float2* M) {
    constexpr auto kSeq = std::make_integer_sequence<int, kPf<MODE>>{};
    if (FR & 2) lane = fresh_lane(lane);
    if (((g - 1u) & 1u) != 0) mix_seq<MODE, true>(lane, r, P, M, kSeq);   // frame g-1 odd
    else mix_seq<MODE, false>(lane, r, P, M, kSeq);
}

using qhunt::wave_max_u32;

// same, but volatile so the load/store optimizer does not pair it into a
// ds_read2_b64 (8 LDS cycles per pair vs 2 per ds_read_b64: MI355X_MICROARCH.md)
typedef __attribute__((address_space(3))) const volatile f2 lds_vf2;
__device__ __forceinline__ f2 ld2nt(const float2* p) {
    return *(lds_vf2*)p;   // p points into LDS
}
// an accumulator pinned in a VGPR at this point of the instruction stream:
// keeps a batch's arithmetic inside it.  Without it LLVM sinks every
// multiply-add below the batch's last wait (the FIR ran as rounds of loads, all
// the arithmetic after them, 59 samples live).  The split FIR is anchored (the
// 4x2 kernel: 0 VGPR spills instead of 5, C3 -1.2% over 5 interleaved rounds,
// profiles/r06_anc_ab.txt); the dual shapes' FIRs are not (+-0 at 8,192-32,768
// channels, +1% at 4,096)
__device__ __forceinline__ void anchor_f2(f2& y) { asm volatile("" : "+v"(y)); }
// one lgkmcnt(0) per LDS sample batch of a FIR, not one per sample
// (profiles/r04_firwait_ab.txt)
__device__ __forceinline__ void fir_batch_wait() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
    __builtin_amdgcn_sched_barrier(0);
}

#ifdef QPSK_STAMPS
#define FSTAMP(i) do { const unsigned long long t_ = stamp_now(); facc[8 + (i)] += t_ - ft0; ft0 = t_; } while (0)
#define FACC_PARAM , unsigned long long (&facc)[16]
#define FACC_ARG , st_acc
#define FACC_FWD , facc
#else
#define FSTAMP(i) do { } while (0)
#define FACC_PARAM
#define FACC_ARG
#define FACC_FWD
#endif
// MODE 1 (dec752): dec_{n+1} = D_n[0..289] only; lane l makes D[5l .. 5l+4]
// from the 69 samples M[25l + rt + s] (58 lanes: 290 outputs, 490 packed
// instructions per channel like MODE 0's 188 + 102).  Lane stride 25 float2
// = 50 dwords (odd multiple of 2): the b64 reads of 32 lanes cover the 64
// banks once.
__device__ __forceinline__ void fir_dec752(int lane, int rt, const float2* M, float2* dec) {
    if (lane < QK_NDECOBS / 5) {
        const float2* b = M + 25 * lane + rt;
        f2 y[5] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
        for (int s0 = 0; s0 < 69; s0 += kFirBatch) {
            f2 v[kFirBatch];
#pragma unroll
            for (int j = 0; j < kFirBatch; j++)
                if (s0 + j < 69) v[j] = ld2nt(b + s0 + j);
            fir_batch_wait();
#pragma unroll
            for (int j = 0; j < kFirBatch; j++) {
                const int s = s0 + j;
#pragma unroll
                for (int m = 0; m < 5; m++) {
                    const int k = s - 5 * m;
                    if (s < 69 && k >= 0 && k < QK_NTAPS) y[m] = y[m] + v[j] * QK_RRC[k];
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 5; m++) {
            const f2 o = y[m] * QK_GAIN;
            dec[5 * lane + m] = make_float2(o.x, o.y);
        }
    }
}

// The FFT-correlation hunt of the QPSK_MODE_FFT_HUNT variant (cpu_ref.h
// qc_fft_hunt): S = ifft(fft(dec[0..255]) * Q) with the reference's kiss_fft
// (qpsk_fft_dev.h, bit-identical to src/fft.c), then the hunt loop of
// src/qpsk.c:172-183 over cnormf(S[l]), l < 128.  The two 256-point buffers
// reuse M (free after the FIR).  HT (LDS): twiddles forward [0, 256) and
// inverse [256, 512), Q [512, 768) as (re, im) pairs, then kf_work's input
// permutation as 256 ints.
// hunt tables (floats): the bf16 pass's B table + the exact chain's p line
constexpr int kHuntTab = qhunt::kBH + qhunt::kPL;
__device__ __forceinline__ int fft_hunt(int lane, float2* M, const float2* dec, const float* HT) {
    const qfft::cf* tw = reinterpret_cast<const qfft::cf*>(HT);
    const int* perm = reinterpret_cast<const int*>(HT + 768 * 2);
    qfft::cf* X = reinterpret_cast<qfft::cf*>(M);
    qfft::cf* Y = X + 256;
    const qfft::cf* d = reinterpret_cast<const qfft::cf*>(dec);
    for (int pos = lane; pos < 256; pos += 64) X[pos] = d[perm[pos]];   // kf_work leaves
    qfft::lds_sync();
    qfft::stages(lane, 256, X, tw, false);
    for (int pos = lane; pos < 256; pos += 64) {   // Y = X * Q, in the inverse's leaf order
        const int k = perm[pos];
        Y[pos] = qfft::mul(X[k], tw[512 + k]);
    }
    qfft::lds_sync();
    qfft::stages(lane, 256, Y, tw + 256, true);
    const qfft::cf s0 = Y[lane], s1 = Y[lane + 64];   // lags lane and 64 + lane
    const float c0 = s0.r * s0.r + s0.i * s0.i;       // cnormf, src/qpsk.c:75-80
    const float c1 = s1.r * s1.r + s1.i * s1.i;
    const unsigned k0 = c0 > 0.0f ? __float_as_uint(c0) : 0u;   // as the direct hunt below
    const unsigned k1 = c1 > 0.0f ? __float_as_uint(c1) : 0u;
    const unsigned km = wave_max_u32(max(k0, k1));
    qfft::lds_sync();   // X / Y (M) are rewritten by the next channel's mixer
    if (km == 0u) return 0;
    const unsigned long long m0 = __ballot(k0 == km), m1 = __ballot(k1 == km);
    return m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
}

// RRC (src/fir.c:36-42), outputs accumulated in tap order.  Decimated outputs
// D[o] = fir_out[5o + rt] (model A): lane l makes o = 3l..3l+2
// from the 59 samples M[15l + rt + s], read in batches of FB samples.
template <int FB = kFirBatch>
__device__ __forceinline__ void fir_dec(int lane, int rt, const float2* M, float2* dec) {
    if (lane < 63) {
        const float2* b = M + 15 * lane + rt;
        f2 y[3] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
        for (int s0 = 0; s0 < 59; s0 += FB) {
            f2 v[FB];
#pragma unroll
            for (int j = 0; j < FB; j++)
                if (s0 + j < 59) v[j] = ld2nt(b + s0 + j);
            fir_batch_wait();
#pragma unroll
            for (int j = 0; j < FB; j++) {
                const int s = s0 + j;
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    const int k = s - 5 * m;
                    if (s < 59 && k >= 0 && k < QK_NTAPS) y[m] = y[m] + v[j] * QK_RRC[k];
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (3 * lane + m < QK_NDEC) {
                const f2 o = y[m] * QK_GAIN;
                dec[3 * lane + m] = make_float2(o.x, o.y);
            }
    }
}

// One FIR output per lane: out = GAIN * sum_k b[k] * RRC[k], k ascending
// (the same operations in the same order as fir_dec / fir_head_at).
constexpr int kFirOneBatch = 8;   // fir_one's samples per LDS batch
__device__ __forceinline__ f2 fir_one(const float2* b) {
    f2 y = {0.0f, 0.0f};
#pragma unroll
    for (int s0 = 0; s0 < QK_NTAPS; s0 += kFirOneBatch) {
        f2 v[kFirOneBatch];
#pragma unroll
        for (int j = 0; j < kFirOneBatch; j++)
            if (s0 + j < QK_NTAPS) v[j] = ld2nt(b + s0 + j);
        fir_batch_wait();
#pragma unroll
        for (int j = 0; j < kFirOneBatch; j++)
            if (s0 + j < QK_NTAPS) y = y + v[j] * QK_RRC[s0 + j];
        anchor_f2(y);
    }
    return y * QK_GAIN;
}

// The split FIR of the 4x2 kernel in reference mode.  dec = [D_n[0..187],
// F_{n+1}[0..101]]; the hunt correlates dec[0..254] (lags < 128 over 128
// symbols) and the window's observable entries are dec[mi .. mi+162]
// (slots past the data symbols never reach an output), so
// F_{n+1}[67..101] = dec[255..289] matter only when mi >= 93.  Every output is
// one 49-tap dot product over consecutive samples, so a lane's outputs may come
// from D or from F as long as its code is the same:
//   pass 1 (fir_dec's code: 3 outputs 5 samples apart): lanes 0..62 D[3l ..
//     3l+2] (D[188] of lane 62 discarded), lane 63 F[56], F[61], F[66];
//   pass 2 (one output per lane): F[l + (l >= 56) + (l >= 60)], 0..66 less
//     56, 61, 66;
//   after the hunt, mi >= 93: F[67 + l], l < 35 (fir_split_tail).
// 392 packed operations before the hunt (294 + 98) instead of 490, and 98 more
// for the ~27% of channels whose window reaches past dec[254].
constexpr int kSplitMi = 255 - (QK_NPRE + QK_NDSYM + 3);   // 93: mi + 162 >= 255
// LDS banks (ds_read_b64: lanes 0-31 and 32-63 are serviced apart, float2 f in
// bank pair f mod 32; MI355X_MICROARCH.md "LDS").  Pass 1's lanes 32..62 read
// M[15l + rt + s]: 31 distinct pairs, so lane 63's base must be the 32nd,
// (15*63 + rt) mod 32; its outputs F[j1], F[j1+5], F[j1+10] follow from that
// residue r: j1 = r + 32 (r <= 24) or r (both <= 56).  Pass 2 reads M[kM1 + j
// + s] for the 64 other j of [0, 66]: lanes 32..63 take j = 35..66 with each of
// pass 1's j in that range replaced by j - 32 (one j per bank pair), lanes 0..31
// the rest.  [0, 66] holds the pairs of j = 0, 1, 2 three times and pass 1's
// triple is 5 apart, so one lane group always keeps a 2-way conflict: 49 extra
// LDS cycles per channel in pass 2, none in pass 1 (before this mapping: pass 1
// lane 63 at F[56] collided for 31 of 32 rt mod 32, and pass 2's j = 64, 65
// with j = 32, 33 -- profiles/probe/fir_split_banks.py).
// The map is qpsk_split.h (split_r, split_j1, make_split_tab), checked on the
// host for every rt by tests/test_split_tab.py.
static_assert(kSplitM1 == kM1, "qpsk_split.h: F_{n+1}'s offset in M");
__constant__ SplitTab kSplitTab = make_split_tab();
constexpr int kSplitTabWords = (int)sizeof(SplitTab) / 4;

// Lane 63's pass-1 base and outputs differ from the other lanes' by wave-uniform
// values only (rt, j1), so each per-lane address is one multiply-add of the
// laundered lane, one select against an SGPR and the shift into bytes; the three
// outputs of a lane are `st` entries apart (1, lane 63: 5), and the only one
// discarded is D[188], lane 62's third.
__device__ __forceinline__ void fir_split(int lane, int rt, const float2* M, float2* dec,
                                          const uint8_t* p2tab) {
    lane = fresh_lane(lane);   // the per-lane bases below are recomputed, not kept live across the loop
    rt = __builtin_amdgcn_readfirstlane(rt);
    const int r = split_r(rt);
    const int j1 = split_j1(r);
    const int j2 = p2tab[r * 64 + lane];
    const bool l63 = lane == 63;
    {   // pass 1
        const float2* b = M + (l63 ? kM1 + j1 : 15 * lane + rt);
        f2 y[3] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
        for (int s0 = 0; s0 < 59; s0 += kFirBatch) {
            f2 v[kFirBatch];
#pragma unroll
            for (int j = 0; j < kFirBatch; j++)
                if (s0 + j < 59) v[j] = ld2nt(b + s0 + j);
            fir_batch_wait();
#pragma unroll
            for (int j = 0; j < kFirBatch; j++) {
                const int s = s0 + j;
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    const int k = s - 5 * m;
                    if (s < 59 && k >= 0 && k < QK_NTAPS) y[m] = y[m] + v[j] * QK_RRC[k];
                }
            }
#pragma unroll
            for (int m = 0; m < 3; m++) anchor_f2(y[m]);
        }
        float2* o = dec + (l63 ? QK_NDEC + j1 : 3 * lane);
        const int st = l63 ? 5 : 1;
        static_assert(3 * 62 + 2 == QK_NDEC, "lane 62's third output is D[188]");
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const f2 q = y[m] * QK_GAIN;
            if (m < 2 || lane != 62) o[m * st] = make_float2(q.x, q.y);
        }
    }
    {   // pass 2
        const f2 o = fir_one(M + kM1 + j2);
        dec[QK_NDEC + j2] = make_float2(o.x, o.y);
    }
}

__device__ __forceinline__ void fir_split_tail(int lane, const float2* M, float2* dec) {
    lane = fresh_lane(lane);
    if (lane < QK_NHEAD - 67) {
        const f2 o = fir_one(M + kM1 + 67 + lane);
        dec[QK_NDEC + 67 + lane] = make_float2(o.x, o.y);
    }
}

// Undecimated head F_{n+1}[j] = fir_out'[j], j < 102: lane l makes j = 2l, 2l+1
// from M[kM1 + 2l + s], s < 50, read as 16-B sample pairs (lane stride 16 B:
// ds_read_b128's lane groups cover the 64 banks once; a b64 read at that
// stride is 2-way conflicted).  It does not depend on rx_timing.
__device__ __forceinline__ void fir_head_at(int lane, const float2* H, float2* out) {
    if (lane < 51) {
        const float2* b = H + 2 * lane;
        f2 y[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
        for (int s0 = 0; s0 < 50; s0 += 10) {
            f2 v[10];
#pragma unroll
            for (int j = 0; j < 10; j += 2) {
                const float4 q = *reinterpret_cast<const float4*>(b + s0 + j);
                v[j] = f2{q.x, q.y};
                v[j + 1] = f2{q.z, q.w};
            }
            fir_batch_wait();
#pragma unroll
            for (int j = 0; j < 10; j++) {
                const int s = s0 + j;
#pragma unroll
                for (int m = 0; m < 2; m++) {
                    const int k = s - m;
                    if (k >= 0 && k < QK_NTAPS) y[m] = y[m] + v[j] * QK_RRC[k];
                }
            }
        }
        const f2 o0 = y[0] * QK_GAIN, o1 = y[1] * QK_GAIN;   // one 16-B store
        *reinterpret_cast<float4*>(out + 2 * lane) = make_float4(o0.x, o0.y, o1.x, o1.y);
    }
}

// ---------------------------------------------------------------- head pre-pass
// SURVEY.md 8f rank 4, as an execution strategy (QPSK_HEADPASS=1; not the
// default, measured slower: profiles/r03_headpass_ab.txt).  F_{n+1}[0..101],
// the undecimated FIR head that dec_{n+1} ends with, does not depend on
// rx_timing, so it is computed for every frame of the call at once, ahead of
// the serial frame loop: one wave per channel-frame mixes the 152 samples the
// head reads -- x_{n-1}[1832..1879] ++ x_n[0..103], each (-1)^k P[t] x 2^-14
// for its global frame k, as mix_item -- and runs the front's fir_head on
// them.  The fronts of the frame loop then copy the 102 outputs into dec
// instead of filtering (front_channel<.., HP>).
constexpr int kHeadM = 152;
__global__ void __launch_bounds__(256) head_kernel(const int16_t* in, const int16_t* hist,
                                                  const float2* ptab, float2* heads, int nch,
                                                  int F, unsigned g0) {
    __shared__ __attribute__((aligned(16))) float2 Mh[4][kHeadM];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t cf = (size_t)blockIdx.x * 4 + w;   // channel-frame ch * F + n
    if (cf >= (size_t)nch * F) return;              // wave-uniform
    const int ch = (int)(cf / (size_t)F), n = (int)(cf % (size_t)F);
    const unsigned g = g0 + (unsigned)n;            // global index of frame n
    const int16_t* xm1 = n >= 1 ? in + ((size_t)ch * F + (n - 1)) * QK_FRAME
                                : hist + ((size_t)ch * 2 + 1) * QK_FRAME;
    const int16_t* x0 = in + ((size_t)ch * F + n) * QK_FRAME;
    float2* H = Mh[w];
    for (int e = lane; e < kHeadM / 2; e += 64) {   // item e: two samples
        const bool prev = e < 24;                   // x_{n-1} tail, else x_n head
        const int t = prev ? 1832 + 2 * e : 2 * (e - 24);
        const int r = *reinterpret_cast<const int*>((prev ? xm1 : x0) + t);
        const float4 p = *reinterpret_cast<const float4*>(ptab + t);
        const float v0 = (float)(int16_t)(r & 0xffff);
        const float v1 = (float)(int16_t)(r >> 16);
        const unsigned k = prev ? g - 1u : g;       // (-1)^k
        const float sg = (k & 1u) ? -1.0f : 1.0f;   // exact sign flip
        *reinterpret_cast<float4*>(H + 2 * e) =
            make_float4((sg * p.x) * v0, (sg * p.y) * v0, (sg * p.z) * v1, (sg * p.w) * v1);
    }
    wave_lds_sync();
    fir_head_at(lane, H, heads + cf * kHeadOut);
}

// correlate (src/qpsk.c:88-96) for all 128 lags of dec and the hunt's argmax
// (src/qpsk.c:172-183).  The T images reuse M (the FIR is done with it).
template <int MODE>
__device__ __forceinline__ int hunt(int lane, float2* M, const float2* dec, const float* BT FACC_PARAM) {
#ifdef QPSK_STAMPS
    unsigned long long ft0 = stamp_now();
#endif
    if constexpr ((MODE & 2) != 0) return fft_hunt(lane, M, dec, BT);
    // bf16 pass, exact chain when in doubt (qpsk_hunt.h hunt_index)
    bool fb;
    const int mi = qhunt::hunt_index(lane, dec, reinterpret_cast<float*>(M), BT, wave_max_u32, fb);
#ifdef QPSK_STAMPS
    facc[2] += 1;          // hunts
    facc[3] += fb ? 1 : 0; // of which the exact chain decided
#endif
    FSTAMP(2);
    return mi;
}

// One channel of frame n's front: D_n (decimated with rx_timing rt), F_{n+1},
// correlation of dec_{n+1} = [D_n, F_{n+1}] and its argmax mi.
// HP (QPSK_HEADPASS): F_{n+1} comes from the head pre-pass (head_kernel), at
// `head` (global, 51 x 16 B), instead of the head FIR.
template <int MODE, bool HP = false, bool SPLIT = false>
__device__ __forceinline__ int front_channel(int lane, int rt, float2* M, float2* dec,
                                             const float* BT, const uint8_t* p2tab,
                                             const float2* head FACC_PARAM) {
#ifdef QPSK_STAMPS
    unsigned long long ft0 = stamp_now();
#endif
    if constexpr ((MODE & 1) != 0) {
        fir_dec752(lane, rt, M, dec);
        FSTAMP(0);
    } else if constexpr (HP) {
        float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (lane < kHeadOut / 2) h = reinterpret_cast<const float4*>(head)[lane];   // under the FIR
        fir_dec(lane, rt, M, dec);
        FSTAMP(0);
        if (lane < kHeadOut / 2) *reinterpret_cast<float4*>(dec + QK_NDEC + 2 * lane) = h;
    } else if constexpr (MODE == 0 && SPLIT) {
        fir_split(lane, rt, M, dec, p2tab);   // dec[0..254]
        FSTAMP(0);
        wave_lds_sync();
        FSTAMP(1);
        const int mi = hunt<MODE>(lane, M, dec, BT FACC_FWD);
        if (mi >= kSplitMi) {          // wave-uniform
            fir_split_tail(lane, M, dec);   // dec[255..289]
            wave_lds_sync();
        }
        return mi;
    } else {
        fir_dec(lane, rt, M, dec);
        FSTAMP(0);
        fir_head_at(lane, M + kM1, dec + QK_NDEC);   // F_{n+1}: M[kM1 ..] (head input)
    }
    wave_lds_sync();
    FSTAMP(1);
    return hunt<MODE>(lane, M, dec, BT FACC_FWD);
}

// window slots (2q, 2q+1) = dec[mi+2q-1], dec[mi+2q] (slot 0 unused); 84
// float4 = 1344 B per channel, full 128-B lines
__device__ __forceinline__ void store_window(int lane, int mi, const float2* dec, float2* out) {
    float4* o = reinterpret_cast<float4*>(out);
    {
        const float2 lo = dec[max(mi + 2 * lane - 1, 0)], hi = dec[mi + 2 * lane];
        o[lane] = make_float4(lo.x, lo.y, hi.x, hi.y);
    }
    if (lane < kWinStride / 2 - 64) {
        const int q = lane + 64;
        const float2 lo = dec[mi + 2 * q - 1], hi = dec[mi + 2 * q];
        o[q] = make_float4(lo.x, lo.y, hi.x, hi.y);
    }
}

}  // namespace
