// qpsk_rx.hip -- MI355X receive path for the single-carrier QPSK modem.
//
// Replaces the reference's per-frame receiver qpsk_rx_frame()
// (/root/reference/src/qpsk.c:133-239) and everything it calls (fir
// src/fir.c:22-44, correlate src/qpsk.c:88-96, kalman_calculate
// src/kalman.c:85-141, train_eq/data_eq src/equalizer.c:25-90, qpsk_demod
// src/qpsk.c:268-271, scramble src/scramble.c:57-84), batched over many
// independent 8 kHz channels.  Output is bit-identical to the reference
// (gcc -O2 build): every fp32 operation is issued in the
// reference's order with no contraction (-ffp-contract=off + the pragma below),
// divisions are correctly rounded, denormals are kept.
//
// One persistent workgroup of two waves owns a group of 64 channels for every
// frame of a call (DESIGN.md "Kernels"):
//   front wave (channel after channel, LDS-staged): mixer -> RRC FIR (only the
//        290 observable outputs) -> decimation -> 128-lag preamble correlation
//        -> argmax -> equalizer window dec[mi .. mi+162] -> HBM (L2)
//   back wave (lane per channel): 128 train_eq + 31 data_eq steps of the
//        square-root Kalman equalizer, slicer, descrambler.
// The front of frame n+1 needs only rx_timing of frame n, so in iteration n the
// front wave works on frame n+1 while the back wave finishes frame n; one
// __syncthreads() per frame hands rx_timing (LDS) and the window (global) over.
//
// This file is the kernels' translation unit: rx_kernel, its launcher and the
// few host functions that must sit beside the kernels.  What rx_kernel runs is
// in the headers included below, by pipeline stage (qpsk_rx_dev.h, _front.h,
// _back.h, _quad.h); the context and every other host function are in
// qpsk_rx_host.hip, which shares only qpsk_rx_shared.h with this file.

// Compile-time A/B knobs whose rejected branches are gone: a -D of one of them
// would build this source unchanged and compare it with itself.
#if defined(QPSK_FRESH) || defined(QPSK_FRESH_SPLIT) || defined(QPSK_HUNT_MFMA) || \
    defined(QPSK_HUNT_FILTER) || defined(QPSK_HUNT_OVERLAP) || defined(QPSK_FIR_WAIT) || \
    defined(QPSK_FIR_ANCHOR) || defined(QPSK_FIR_SPLIT) || defined(QPSK_SPLIT_BANKS) || \
    defined(QPSK_QDMUL) || defined(QPSK_TRAIN_PRETAB) || defined(QPSK_DYNPRIO) || \
    defined(QPSK_DATA_RING) || defined(QPSK_LATE_YIELD) || defined(QPSK_FB) || defined(QPSK_FB1) || \
    defined(QPSK_ZERO_COPY)
#error "QPSK_FRESH, QPSK_FRESH_SPLIT, QPSK_HUNT_MFMA, QPSK_HUNT_FILTER, QPSK_HUNT_OVERLAP, QPSK_FIR_WAIT, QPSK_FIR_ANCHOR, QPSK_FIR_SPLIT, QPSK_SPLIT_BANKS, QPSK_QDMUL, QPSK_TRAIN_PRETAB, QPSK_DYNPRIO, QPSK_DATA_RING, QPSK_LATE_YIELD, QPSK_FB, QPSK_FB1 and QPSK_ZERO_COPY were removed with their alternative branches: DESIGN.md, Removed knobs, names the commit that still has each"
#endif

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "qpsk_batch.h"
#include "qpsk_consts.h"
#include "qpsk_hunt.h"
#include "qpsk_rx_shared.h"
// the kernels' stages, in pipeline order
#include "qpsk_rx_dev.h"
#include "qpsk_rx_front.h"
#include "qpsk_rx_back.h"
#include "qpsk_rx_quad.h"

#pragma clang fp contract(off)

namespace {

#ifndef QPSK_RX_ATTR
#define QPSK_RX_ATTR   // A/B: e.g. __attribute__((amdgpu_num_vgpr(128))) to price a 4-wave budget
#endif
// 4x2 fronts: the frame's last K channels at the back wave's issue priority.
// Since the anchored FIR the back is the frame's last wave (4.4% of a frame
// alone, profiles/r06_c19_stamps_c3_both.json); K = 2: C3 -0.7% over 12
// interleaved rounds (10 faster), K = 1 / 4 +-0, K = 8 +2.4%
// (profiles/r06_ly_ab.txt, r06_ly2_ab.txt)
constexpr int kLateYield = 2;

// Plain pointer parameters (not a by-value struct): the compiler then knows every
// pointer is a global-memory pointer (global_load/store, no flat) and nothing of
// the argument block is indexed dynamically (no scratch copy).
// 12 waves per workgroup, 3 per SIMD (<= 168 VGPRs), one workgroup per CU (LDS).
//
// DUAL (G <= 2): two back waves per group, one for the even and one for the odd
// frames of the call.  Frame n's training needs only frame n-1's front, and
// frame n-1's front needs frame n-2's decision, so consecutive frames' training
// is independent: the back of frame n+1 starts as soon as the front of frame n
// is done, while the back of frame n is still running.  The per-frame time
// drops from max(back, front) to (back + front) / 2 where one serial back wave
// per CU bounds the kernel (<= 16,384 channels per GPU).  Progress is handed
// over through LDS counters (bseq: frames decided per back wave; fcnt: front
// frames finished, by frame parity) instead of __syncthreads().
//
// W (DUAL only): channels per group, 64, 32 or 16.  A narrower group leaves
// back lanes idle but spreads a small batch over more CUs and gives each front
// wave fewer channels per frame, which shortens the front half of the chain.
//
// QUAD (DUAL, G == 1 only): the back waves hold a quad of lanes per channel
// (back_frame_quad), 16 channels per wave, W / 16 waves per frame chain.
template <int G, bool DUAL, int W, bool QUAD>
constexpr int kBackWavesOf = DUAL ? 2 * G * (QUAD ? W / 16 : 1) : G;

// An instantiation's waves: rx_kernel's __launch_bounds__ and kBlock and the
// host's launch (launch_rx) all take the block size from here.
// waves per SIMD = ceil(waves / 4): 3 (<= 168 VGPRs) for the 12-wave shapes
template <int G, int FP, bool DUAL, int W, bool QUAD>
constexpr int kWavesOf = kBackWavesOf<G, DUAL, W, QUAD> + G * FP;

//
// HP: the fronts take F_{n+1} from the head pre-pass (head_kernel, QPSK_HEADPASS).
template <int G, int FP, int MODE, bool DUAL, int W = QK_GROUP, bool QUAD = false, bool HP = false>
__global__ void __launch_bounds__((64 * kWavesOf<G, FP, DUAL, W, QUAD>),
                                  ((kWavesOf<G, FP, DUAL, W, QUAD> + 3) / 4)) QPSK_RX_ATTR rx_kernel(
    const int16_t* in, int16_t* hist, const float2* ptab, const unsigned long long* ks,
    float2* win0, float2* win1, int* mi0, int* mi1, int* rt0, int* rt1, uint8_t* bits,
    uint8_t* valid, int32_t* trace, float2* soft, float4* jobs, unsigned* njobs, int nch, int F,
    unsigned g0, int roles, const float* fft_tab, unsigned long long jcap, int* err) {
    static_assert(W == QK_GROUP || (DUAL && G == 1 && W % FP == 0 && W <= QK_GROUP), "group width");
    static_assert(!QUAD || (DUAL && G == 1 && W % 16 == 0), "quad backs: dual chain, one group");
    constexpr int kGroups = G, kFrontPer = FP;
    constexpr int kBackWaves = kBackWavesOf<G, DUAL, W, QUAD>;
    constexpr int kChainWaves = QUAD ? W / 16 : 1;     // back waves per frame chain and group
    // dynamic issue priority of the dual-chain back waves: they train at the
    // highest priority unless another back wave waits for its fronts.  Quad
    // backs only (-1.5% at 8,192 channels, -4% at 4,096; lane backs +1..4%:
    // profiles/r03_dynprio_ab.txt)
    constexpr bool kDyn = DUAL && QUAD;
    constexpr int kFrontCh = W / kFrontPer;            // channels per front wave
    constexpr int kFrontWaves = kGroups * kFrontPer;
    constexpr int kBlock = 64 * kWavesOf<G, FP, DUAL, W, QUAD>;
    const RxArgs a{in, hist, ptab, ks, win0, win1, mi0, mi1, rt0, rt1, bits, valid, trace, soft,
                   jobs, njobs, nch, F, g0, (size_t)jcap, roles, err,
                   // HP (reference mode only): fft_tab carries the head pre-pass outputs
                   HP ? reinterpret_cast<const float2*>(fft_tab) : nullptr};
    __shared__ __attribute__((aligned(16))) float2 P[QK_FRAME];
    constexpr int DM = MODE & 1;   // decimation semantics; MODE & 2: FFT hunt
    constexpr int kM = Cfg<DM>::kM, kDecBuf = Cfg<DM>::kDecBuf;
    __shared__ __attribute__((aligned(16))) float2 Ms[kFrontWaves][kM];
    __shared__ __attribute__((aligned(16))) float2 decs[kFrontWaves][kDecBuf][kDec];
    __shared__ int mi_s[kGroups][2][QK_GROUP], rt_s[kGroups][2][QK_GROUP];
    // hunt tables: the MFMA correlator's B, or the FFT hunt's twiddles / Q / permutation
    __shared__ __attribute__((aligned(16))) float BT[(MODE & 2) ? kFftHT : kHuntTab];
    // the 4x2 kernel in reference mode (not the head pre-pass, not the FFT
    // hunt) runs the split FIR (fir_split); the dual-chain shapes keep fir_dec +
    // fir_head_at: their fronts are latency-bound and the split's extra LDS
    // reads cost them ~1% (profiles/r05_split_ab.txt).  Its pass-2 lane map
    // (kSplitTab; 2 KB):
    constexpr bool kSplitK = MODE == 0 && !HP && !DUAL;
    __shared__ uint32_t p2w[kSplitK ? kSplitTabWords : 1];
    const uint8_t* p2tab = reinterpret_cast<const uint8_t*>(p2w);
    // DUAL progress counters, per group, frame parity and channel block (one
    // block per back wave of a chain)
    __shared__ int bseq[kGroups][2][kChainWaves], fcnt[kGroups][2][kChainWaves];
    __shared__ int dead_s;                               // DUAL: a wait of this workgroup timed out
    __shared__ int nwait_s;                              // kDyn: back waves waiting for their fronts
#ifdef QPSK_STAMPS
    // diagnostic (4x2): each wave's arrival at the frame barrier and its SIMD;
    // a back wave sums the cycles it trains after the last front of its SIMD
    // arrived (stamp 15) and counts the frames it arrived last (stamp 5)
    __shared__ unsigned long long tarr_s[16];
    __shared__ int tsimd_s[16];
#define TAIL_INIT() do { if (lane == 0 && wave < 16) tsimd_s[wave] = (int)((__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4) >> 4) & 3); } while (0)
#define TAIL_ARRIVE() do { if (lane == 0 && wave < 16) tarr_s[wave] = stamp_now(); } while (0)
#define TAIL_BACK()                                                                           \
    do {                                                                                      \
        unsigned long long tf = 0;                                                            \
        for (int w2 = kBackWaves; w2 < kBackWaves + kFrontWaves && w2 < 16; w2++)             \
            if (tsimd_s[w2] == tsimd_s[wave] && tarr_s[w2] > tf) tf = tarr_s[w2];            \
        if (tf > 0 && tarr_s[wave] > tf) { st_acc[15] += tarr_s[wave] - tf; st_acc[5] += 1; } \
        st_t0 = stamp_now();                                                                  \
    } while (0)
#else
#define TAIL_INIT() do { } while (0)
#define TAIL_ARRIVE() do { } while (0)
#define TAIL_BACK() do { } while (0)
#endif
    // a launch whose block is not this instantiation's waves would leave roles
    // unserved and every progress wait to its bound: report it and do nothing
    if (blockDim.x != (unsigned)kBlock) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, kErrStall);
        return;
    }
    const int lane = threadIdx.x & 63;
    // wave-uniform by construction; readfirstlane tells the compiler, so every
    // per-wave index and pointer below lives in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp0 = blockIdx.x * kGroups;
    TAIL_INIT();
    for (int i = threadIdx.x; i < QK_FRAME / 2; i += kBlock)
        reinterpret_cast<float4*>(P)[i] = reinterpret_cast<const float4*>(a.ptab)[i];
    if constexpr (kSplitK)
        for (int i = threadIdx.x; i < kSplitTabWords; i += kBlock)
            p2w[i] = reinterpret_cast<const uint32_t*>(&kSplitTab)[i];
    if constexpr ((MODE & 2) != 0) {
        for (int i = threadIdx.x; i < kFftHT; i += kBlock) BT[i] = fft_tab[i];
    } else {
        qhunt::bconst_h_lds(threadIdx.x, kBlock, BT);
    }
    if (wave < kGroups) {   // per-channel state of the groups at the call's first frame
        const int ch = (grp0 + wave) * W + lane;
        if (lane < W && ch < a.nch) {
            mi_s[wave][0][lane] = mi_of(a, a.g0)[ch];
            rt_s[wave][0][lane] = rt_of(a, a.g0)[ch];
        }
    }
    if (threadIdx.x < 2 * kGroups * kChainWaves) (&bseq[0][0][0])[threadIdx.x] = (&fcnt[0][0][0])[threadIdx.x] = 0;
    if (threadIdx.x == 0) dead_s = nwait_s = 0;
    __syncthreads();
    if constexpr (DUAL) {
        // Channel blocks: a group's channels split into one block per back wave
        // of a chain (QUAD: 16 channels; lane backs: the whole group).  A back
        // wave waits only for the fronts of its own block, and the front waves
        // serve the blocks one at a time (every front wave takes its share of
        // block 0, signals, then block 1): a block's windows are ready after
        // its share of the front work, not the group's, and the chain waves
        // settle into a stagger of one block's front time
        // (profiles/r03_blocks_ab.txt; lane backs split into 32-channel blocks
        // were measured too: slower, two back waves issue every step).
        // bseq[gi][p][b]: frames of parity p decided by block b's back wave;
        // fcnt[gi][p][b]: front waves done with block b of parity-p frames.
        constexpr int kBlkCh = W / kChainWaves;            // channels per block
        constexpr int kFrontChB = kBlkCh / kFrontPer;      // per front wave and block
        static_assert(kBlkCh % kFrontPer == 0, "block split");
        if (wave < kBackWaves) {
            // ---------------------------------------------------- back of group
            // gi = (wave >> 1) / kChainWaves, block b, frames n = wave mod 2
            const int gi = (wave >> 1) / kChainWaves;
            const int b = (wave >> 1) % kChainWaves;
            // channel of this lane within the block: the lane, or its quad.
            // Lanes past the block (lane backs with W < 64) own no channel:
            // they read their block's first channel's slots and write none.
            const int sub = QUAD ? lane >> 2 : lane;
            const bool own = sub < kBlkCh;
            const int idx = kBlkCh * b + (own ? sub : 0);
            const int ch = (grp0 + gi) * W + idx;
            const bool live = own && ch < a.nch;
            if (kDyn || roles_prio(a.roles) == kPrioBack) __builtin_amdgcn_s_setprio(2);
            // kDyn: every 4 training steps, drop to the lowest
            // issue priority while another back wave waits for its fronts, else the highest
            auto poll = [&] {
                if constexpr (kDyn) {
                    const int w = __builtin_amdgcn_readfirstlane(
                        __hip_atomic_load(&nwait_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                    if (w > 0) __builtin_amdgcn_s_setprio(0);
                    else __builtin_amdgcn_s_setprio(2);
                }
            };
            // tests (roles bit kDebugStall): one wait that cannot end, on the
            // first back wave of workgroup 0, with a short bound
            if (roles_debug_stall(a.roles) && blockIdx.x == 0 && wave == 0)
                spin_wait(&fcnt[gi][0][0], 1 << 30, a.err, &dead_s, 1u << 12);
            // diagnostic stamps (QPSK_STAMPS): 13 frame work, 14 wait for the
            // fronts, 15 wait for the other chain's decision
            STAMP_DECL
            for (int n = wave & 1; n < a.F; n += 2) {
                const int p = n & 1;
                // front(n-1) done by every front wave for this block: window n and mi_n
                if (n > 0) {
                    int* const fc = &fcnt[gi][p ^ 1][b];
                    const int need = kFrontPer * ((n - 1) / 2 + 1);
                    if constexpr (kDyn) {
                        const bool waits = __builtin_amdgcn_readfirstlane(__hip_atomic_load(
                                               fc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < need;
                        if (waits) {   // wait at the lowest priority; poll() resets it
                            __builtin_amdgcn_s_setprio(0);
                            if (lane == 0)
                                __hip_atomic_fetch_add(&nwait_s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        spin_wait(fc, need, a.err, &dead_s);
                        if (waits && lane == 0)
                            __hip_atomic_fetch_add(&nwait_s, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        spin_wait(fc, need, a.err, &dead_s);
                    }
                }
                STAMP(14);
                const int mi = mi_s[gi][p][idx];
                auto get_rt = [&] {   // rx_timing of frame n = the decision of frame n-1
                    STAMP(13);
                    if (n > 0) spin_wait(&bseq[gi][p ^ 1][b], (n - 1) / 2 + 1, a.err, &dead_s);
                    STAMP(15);
                    return rt_s[gi][p][idx];
                };
                const float2* wn = win_of(a, a.g0 + (unsigned)n) + (size_t)(live ? ch : 0) * kWinStride;
                int* rtn = own ? &rt_s[gi][p ^ 1][idx] : nullptr;
                if constexpr (QUAD)
                    back_frame_quad(a, live ? ch : 0, live, n, mi, get_rt, wn, rtn, poll);
                else
                    back_frame(a, live ? ch : 0, live, n, mi, get_rt, wn, rtn, poll);
                signal_add(&bseq[gi][p][b], 1, lane);
                STAMP(13);
            }
            STAMP_FLUSH();
        } else {
            // ---------------------------------------------------- front
            const int f = wave - kBackWaves;
            const int gi = f / kFrontPer;
            const int fl = f % kFrontPer;
            // roles bits 16-19 (split s, one group and one block per workgroup
            // only; pick_shape sets 2 at W = 64): the front waves that share a
            // SIMD with a back wave (waves 4, 5, 8, 9 when waves map to SIMDs by
            // wave % 4) take s channels fewer, the others s more
            const int split = (kGroups == 1 && kChainWaves == 1) ? roles_split(a.roles) : 0;
            auto share = [&](int x) { return ((x + kBackWaves) & 3) < kBackWaves; };
            int cbeg = 0;
            for (int x = 0; x < fl; x++) cbeg += kFrontChB + (share(x) ? -split : split);
            const int mych = kFrontChB + (share(fl) ? -split : split);
            // this wave's channels of block bb: group index kBlkCh * bb + cbeg + c
            auto bch0 = [&](int bb) { return (grp0 + gi) * W + kBlkCh * bb + cbeg; };
            auto blive = [&](int bb) { return max(0, min(mych, a.nch - bch0(bb))); };
            float2* M = Ms[f];
            int pf[kPf<DM>];
            // the dual-chain fronts keep fir_dec + fir_head_at (see kSplitK).  A named
            // constant like the 4x2 fronts' kSplit, not a literal: the quad
            // kernels' frame_iter lambda names it, and without that their
            // register allocation comes out differently
            constexpr bool kSplitD = false;
            if (kDyn) __builtin_amdgcn_s_setprio(1);
            else if (roles_prio(a.roles) == kPrioFront) __builtin_amdgcn_s_setprio(2);
            if (blive(0) > 0) prefetch<DM, false, kSplitD>(srcs(a, bch0(0), 0), lane, pf);
            // diagnostic stamps (QPSK_STAMPS): 7 wait for the backs, 0 mix,
            // 4 window store, 1 prefetch, 8-12 front_channel phases, 6 its tail,
            // 5 signal
            STAMP_DECL
            int k = 0;   // channels done, for the dec buffer ring
// One frame n of a dual-chain front wave's channels.  CG: frame n >= 2, so
// every prefetch reads consecutive rows of `in` (prefetch<.., true>, see
// load_item); the quad-back kernels peel frames 0 and 1 off for it (in the
// lane-back kernels the single loop keeps their code unchanged).
#define QPSK_DUAL_FRONT_FRAME(CG)                                                                              \
    do {                                                                                                       \
        const int p = n & 1;                                                                                   \
        const unsigned g = a.g0 + (unsigned)n;                                                                 \
        float2* wout = win_of(a, g + 1u);                                                                      \
        for (int bb = 0; bb < kChainWaves; bb++) {                                                             \
            /* back(n-1) of this block done: rx_timing of frame n, and */                                      \
            /* window n+1's buffer (window n-1) and mi_{n-1} are free */                                       \
            if (n > 0) spin_wait(&bseq[gi][p ^ 1][bb], (n - 1) / 2 + 1, a.err, &dead_s);                       \
            STAMP(7);                                                                                          \
            const int c0 = bch0(bb), nl = (roles_front_idle(a.roles) && n >= 2) ? 0 : blive(bb);               \
            const int i0 = kBlkCh * bb + cbeg;                                                                 \
            int pmi = 0;                                                                                       \
            for (int c = 0; c < nl; c++, k++) {                                                                \
                const int ch = c0 + c;                                                                         \
                float2* dcur = decs[f][k % kDecBuf];                                                           \
                mix<DM, kSplitD>(lane, pf, g, P, M);                                                           \
                STAMP(0);                                                                                      \
                if (c > 0)                                                                                     \
                    store_window(lane, pmi, decs[f][(k - 1) % kDecBuf], wout + (size_t)(ch - 1) * kWinStride); \
                STAMP(4);                                                                                      \
                {   /* the next channel: of this block, the next live block, or frame n+1 */                   \
                    int nb = bb, nc = c + 1, nn = n;                                                           \
                    if (nc >= nl) {                                                                            \
                        nc = 0;                                                                                \
                        nb = bb + 1;                                                                           \
                        while (nb < kChainWaves && blive(nb) == 0) nb++;                                       \
                        if (nb == kChainWaves) { nb = 0; nn = n + 1; }                                         \
                    }                                                                                          \
                    if (nn < a.F) prefetch<DM, CG, kSplitD>(srcs(a, bch0(nb) + nc, nn), lane, pf);             \
                }                                                                                              \
                wave_lds_sync();                                                                               \
                STAMP(1);                                                                                      \
                pmi = front_channel<MODE, HP, kSplitD>(lane, rt_s[gi][p][i0 + c], M, dcur, BT, p2tab,         \
                                              a.heads + ((size_t)ch * a.F + n) * kHeadOut FACC_ARG);           \
                if (lane == 0) mi_s[gi][p ^ 1][i0 + c] = pmi;                                                  \
                if (c + 1 == nl) store_window(lane, pmi, dcur, wout + (size_t)ch * kWinStride);                \
                wave_lds_sync();                                                                               \
                STAMP(6);                                                                                      \
            }                                                                                                  \
            signal_add(&fcnt[gi][p][bb], 1, lane);                                                             \
            STAMP(5);                                                                                          \
        }                                                                                                      \
    } while (0)
            if constexpr (QUAD) {
                auto frame_iter = [&](auto cg, int n) {
                    constexpr bool CG = decltype(cg)::value;
                    QPSK_DUAL_FRONT_FRAME(CG);
                };
                for (int n = 0; n < a.F && n < 2; n++) frame_iter(std::false_type{}, n);
                for (int n = 2; n < a.F; n++) frame_iter(std::true_type{}, n);
            } else {
                for (int n = 0; n < a.F; n++) QPSK_DUAL_FRONT_FRAME(false);
            }
#undef QPSK_DUAL_FRONT_FRAME
            STAMP_FLUSH();
        }
        __syncthreads();
        if (wave < kBackWaves && (wave & 1) == 0) {   // state after the call's last frame
            const int gi = (wave >> 1) / kChainWaves;
            const int sub = QUAD ? lane >> 2 : lane;
            const int idx = kBlkCh * ((wave >> 1) % kChainWaves) + sub;
            const int ch = (grp0 + gi) * W + idx;
            if (sub < kBlkCh && ch < a.nch && (!QUAD || (lane & 3) == 0)) {
                const unsigned ge = a.g0 + (unsigned)a.F;
                mi_of(a, ge)[ch] = mi_s[gi][a.F & 1][idx];
                rt_of(a, ge)[ch] = rt_s[gi][a.F & 1][idx];
            }
        }
        return;
    }
    if (wave < kBackWaves) {
        // ------------------------------------------------------------ back
        const int gi = wave;
        const int ch = (grp0 + gi) * QK_GROUP + lane;
        const bool live = ch < a.nch;
        const bool any = (grp0 + gi) * QK_GROUP < a.nch;
        if (roles_prio(a.roles) == kPrioBack) __builtin_amdgcn_s_setprio(2);
        STAMP_DECL
        for (int n = 0; n < a.F; n++) {
            const int p = n & 1;
            if (any && roles_back(a.roles)) {
                const int rt = rt_s[gi][p][lane];
                back_frame(a, live ? ch : 0, live, n, mi_s[gi][p][lane], [=] { return rt; },
                           win_of(a, a.g0 + (unsigned)n) + (size_t)(live ? ch : 0) * kWinStride,
                           &rt_s[gi][p ^ 1][lane], [] {});
            }
            else
                rt_s[gi][p ^ 1][lane] = rt_s[gi][p][lane];
            STAMP(13);
            TAIL_ARRIVE();
            __syncthreads();
            STAMP(14);
            TAIL_BACK();
        }
        STAMP_FLUSH();
        if (live) {   // per-channel state after the call's last frame
            const unsigned ge = a.g0 + (unsigned)a.F;
            mi_of(a, ge)[ch] = mi_s[gi][a.F & 1][lane];
            rt_of(a, ge)[ch] = rt_s[gi][a.F & 1][lane];
        }
    } else {
        // ------------------------------------------------------------ front
        // channel by channel: mix (prefetched samples) -> store the previous
        // channel's window -> prefetch the next channel -> FIR/correlate/argmax
        // the split FIR (fir_split) and, to keep the channel loop's per-lane
        // constants out of scratch beside it, recomputed prefetch offsets
        constexpr bool kSplit = MODE == 0 && !HP;
        const int f = wave - kBackWaves;
        const int gi = f / kFrontPer;
        const int cbeg = (f % kFrontPer) * kFrontCh;
        const int ch0 = (grp0 + gi) * QK_GROUP + cbeg;
        const int nlive = max(0, min(kFrontCh, a.nch - ch0));
        float2* M = Ms[f];
        const bool on = roles_front(a.roles) != 0 && nlive > 0;
        if (roles_prio(a.roles) == kPrioFront) __builtin_amdgcn_s_setprio(2);
        int pf[kPf<DM>];
        if (on) prefetch<DM, false, kSplit>(srcs(a, ch0, 0), lane, pf);
        STAMP_DECL
        // One frame n of a 4x2 front wave's channels.  CG: frame n >= 2, so every
        // prefetch reads consecutive rows of `in`: all 11 items from one scalar
        // base (prefetch_rows).  The split kernel peels frames 0 and 1, which
        // read the history, off for it (profiles/front_trim_ab.txt).
#define QPSK_FRONT_FRAME(CG)                                                                                      \
    do {                                                                                                          \
        const int p = n & 1;                                                                                      \
        const unsigned g = a.g0 + (unsigned)n;                                                                    \
        float2* wout = win_of(a, g + 1u);                                                                         \
        int pmi = 0;                                                                                              \
        /* roles bits 8-15 (stagger, kStagger): the second half of the front waves */                             \
        /* (the younger partner on each SIMD) starts each frame that many x */                                    \
        /* 512 cycles late, so partners' FIR and MFMA/LDS phases interleave */                                    \
        /* (MI355X_MICROARCH.md "two waves per SIMD", item 9) */                                                  \
        for (int z = (f >= kFrontWaves / 2) ? roles_stagger(a.roles) : 0; z > 0; z--)                             \
            __builtin_amdgcn_s_sleep(8);                                                                          \
        for (int c = 0; on && c < nlive; c++) {                                                                   \
            const int ch = ch0 + c;                                                                               \
            float2* dcur = decs[f][c % kDecBuf];                                                                  \
            /* the last kLateYield channels of a frame at the back wave's */                                      \
            /* issue priority, so the back (the frame's last wave) gets its */                                    \
            /* share before the fronts reach the barrier */                                                       \
            if (c == nlive - kLateYield && roles_prio(a.roles) == kPrioFront)                                     \
                __builtin_amdgcn_s_setprio(0);                                                                    \
            mix<DM, kSplit>(lane, pf, g, P, M);                                                                   \
            STAMP(0);                                                                                             \
            if (c > 0) store_window(lane, pmi, decs[f][(c - 1) % kDecBuf], wout + (size_t)(ch - 1) * kWinStride); \
            { /* next channel of this frame, else the first of the next frame */                                  \
                const bool same = c + 1 < nlive;                                                                  \
                if constexpr (CG) {                                                                               \
                    /* scalar arithmetic only: a select on `same` would go through the VALU */                    \
                    const int left = __builtin_amdgcn_readfirstlane(nlive - c - 1);                               \
                    const int sm = min(left, 1); /* 1: the next channel is this frame's */                        \
                    const int nn = n + 1 - sm;                                                                    \
                    if (nn < a.F)                                                                                 \
                        prefetch_rows<kSplit>(a.in + ((size_t)(ch0 + sm * (c + 1)) * a.F + (nn - 2)) * QK_FRAME,  \
                                              lane, pf);                                                          \
                } else if (same || n + 1 < a.F) {                                                                 \
                    prefetch<DM, false, kSplit>(srcs(a, same ? ch + 1 : ch0, same ? n : n + 1), lane, pf);        \
                }                                                                                                 \
            }                                                                                                     \
            wave_lds_sync();                                                                                      \
            STAMP(1);                                                                                             \
            pmi = front_channel<MODE, HP, kSplit>(lane, rt_s[gi][p][cbeg + c], M, dcur, BT, p2tab,                \
                                          a.heads + ((size_t)ch * a.F + n) * kHeadOut FACC_ARG);                  \
            if (lane == 0) mi_s[gi][p ^ 1][cbeg + c] = pmi;                                                       \
            if (c + 1 == nlive) store_window(lane, pmi, dcur, wout + (size_t)ch * kWinStride);                    \
            wave_lds_sync();                                                                                      \
            STAMP(6);                                                                                             \
        }                                                                                                         \
        TAIL_ARRIVE();                                                                                            \
        __syncthreads();                                                                                          \
        if (roles_prio(a.roles) == kPrioFront) __builtin_amdgcn_s_setprio(2);                                     \
        STAMP(7);                                                                                                 \
    } while (0)
        if constexpr (kSplit) {
            for (int n = 0; n < a.F && n < 2; n++) QPSK_FRONT_FRAME(false);
            for (int n = 2; n < a.F; n++) QPSK_FRONT_FRAME(true);
        } else {
            for (int n = 0; n < a.F; n++) QPSK_FRONT_FRAME(false);
        }
#undef QPSK_FRONT_FRAME
        STAMP_FLUSH();
    }
}

}  // namespace

// rx_kernel instantiations (pick_shape, qpsk_rx_host.hip); ShapeOf<kind> holds a
// kind's template parameters, the only place that spells them
template <int KIND> struct ShapeOf;
template <int G_, int FP_, bool DUAL_, int W_, bool QUAD_> struct ShapeParams {
    static constexpr int G = G_, FP = FP_, W = W_;
    static constexpr bool DUAL = DUAL_, QUAD = QUAD_;
};
template <> struct ShapeOf<Shape::k4x2> : ShapeParams<4, 2, false, 64, false> {};
template <> struct ShapeOf<Shape::k2x4d> : ShapeParams<2, 4, true, 64, false> {};
template <> struct ShapeOf<Shape::k1x8d64> : ShapeParams<1, 8, true, 64, false> {};
template <> struct ShapeOf<Shape::k1x8q16> : ShapeParams<1, 8, true, 16, true> {};
template <> struct ShapeOf<Shape::k1x8q32> : ShapeParams<1, 8, true, 32, true> {};

// rx_kernel of one shape, mode and head-pass setting.  Grid and block come from
// the parameters the kernel is instantiated with: a workgroup serves G groups
// of W channels with kWavesOf waves (less a.short_block, the launch-shape
// guard's test hook).
template <int KIND, int MODE, bool HP>
static void launch_rx(const RxLaunch& a) {
    using S = ShapeOf<KIND>;
    constexpr size_t kPer = (size_t)S::G * S::W;
    constexpr int kBlock = 64 * kWavesOf<S::G, S::FP, S::DUAL, S::W, S::QUAD>;
    hipLaunchKernelGGL((rx_kernel<S::G, S::FP, MODE, S::DUAL, S::W, S::QUAD, HP>),
                       dim3((unsigned)((a.nch + kPer - 1) / kPer)), dim3(kBlock - a.short_block), 0,
                       a.s, a.in, a.hist, a.ptab, a.ks, a.win[0], a.win[1], a.mi[0],
                       a.mi[1], a.rt[0], a.rt[1], a.bits, a.valid, a.trace,
                       reinterpret_cast<float2*>(a.soft), a.jobs, a.njobs + a.parity, a.nch, a.F,
                       a.g0, a.roles, HP ? reinterpret_cast<const float*>(a.heads) : a.fft_tab,
                       (unsigned long long)a.jobs_cap, a.err);
}

template <int MODE, bool HP>
static void launch_shape(const RxLaunch& a) {
    switch (a.kind) {
        case Shape::k2x4d: return launch_rx<Shape::k2x4d, MODE, HP>(a);
        case Shape::k1x8d64: return launch_rx<Shape::k1x8d64, MODE, HP>(a);
        case Shape::k1x8q16: return launch_rx<Shape::k1x8q16, MODE, HP>(a);
        case Shape::k1x8q32: return launch_rx<Shape::k1x8q32, MODE, HP>(a);
        default: return launch_rx<Shape::k4x2, MODE, HP>(a);
    }
}

namespace {
// read and clear the error word in one atomic exchange: a stall reported by a
// kernel between a read and a separate clear cannot be lost
__global__ void err_take_kernel(int* err) {
    if (threadIdx.x == 0) err[1] = atomicExch(&err[0], 0);
}
}  // namespace

int qpsk_rx_take_err(int* d_err, hipStream_t s) {
    hipLaunchKernelGGL(err_take_kernel, dim3(1), dim3(64), 0, s, d_err);
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

#ifndef QPSK_KERNEL_HASH
#define QPSK_KERNEL_HASH "unknown"
#endif
// the Makefile's hash of the receive kernels' sources and build rules
extern "C" const char* qpsk_kernel_hash(void) { return QPSK_KERNEL_HASH; }

#ifdef QPSK_STAMPS
extern "C" int qpsk_debug_stamps(unsigned long long* out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16) != hipSuccess)
        return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif

// The launches of one call, for qpsk_rx_launch (qpsk_rx_host.hip), which has
// checked the arguments and sized the buffers.
int qpsk_rx_launch_kernels(const RxLaunch& a) {
    if (a.hp) {   // head pre-pass: every channel-frame's F_{n+1}, then the frame loop
        const size_t ncf = (size_t)a.nch * (size_t)a.F;
        hipLaunchKernelGGL(head_kernel, dim3((unsigned)((ncf + 3) / 4)), dim3(256), 0, a.s, a.in,
                           a.hist, a.ptab, a.heads, a.nch, a.F,
                           a.g0);
        HCHECK(hipGetLastError());
        launch_shape<0, true>(a);
    } else {
        switch (a.mode) {
            case 0: launch_shape<0, false>(a); break;
            case 1: launch_shape<1, false>(a); break;
            case 2: launch_shape<2, false>(a); break;
            default: launch_shape<3, false>(a); break;
        }
    }
    HCHECK(hipGetLastError());
    if (a.ev_mid) HCHECK(hipEventRecord(a.ev_mid, a.s));
    // at most one job per channel-frame: a small call (the per-frame drop-in
    // qpsk_rx_frame is one job at most) launches only the workgroups it can use
    const size_t need = (size_t)a.nch * (size_t)a.F;
    const unsigned dgrid = (unsigned)std::min<size_t>(kDataGrid, (need + kDataBlock - 1) / kDataBlock);
    // in front of them the workgroups that carry the sample history (carry_block):
    // one batch of kCarryK channels per wave up to kCarryGrid workgroups, so a
    // one-channel call gets one
    constexpr int kPerBlock = kDataBlock / 64 * kCarryK;
    const unsigned ncarry = (unsigned)std::min(kCarryGrid, (a.nch + kPerBlock - 1) / kPerBlock);
    const int head8 = (a.mode & QPSK_MODE_DEC752) ? 213 : 149;   // x_{F-1}[0..1704) or [0..1192)
    hipLaunchKernelGGL(rx_data_kernel, dim3(ncarry + dgrid), dim3(kDataBlock), 0, a.s, a.jobs,
                       (unsigned long long)a.jobs_cap, a.njobs, a.ks, a.koff, a.bits,
                       reinterpret_cast<float2*>(a.soft), a.parity, a.roles & kForceExact, a.ctx_err,
                       a.err_to, a.in, a.hist, a.nch, a.F, head8, ncarry);
    HCHECK(hipGetLastError());
    if (a.ev_end) HCHECK(hipEventRecord(a.ev_end, a.s));
    return QPSK_OK;
}
