// qpsk_rx_dev.h -- what every stage of the receive kernels shares: the frame
// geometry, the argument block, the diagnostic stamps and the wave / workgroup
// synchronisation helpers (included by qpsk_rx.hip only).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qpsk_cmul.h"
#include "qpsk_consts.h"
#include "qpsk_hunt.h"
#include "qpsk_rx_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int kDec = 296;
// Receiver semantics (qpsk_batch.h QPSK_MODE_*): 0 = the reference as built
// (gcc -O2 "model A" decimated_frame overflow); 1 = dec752, the
// array with the 752 entries its loop writes (NOT
// reference parity).  Only the front wave's inputs and FIR differ.
//
// front LDS (float2 units), MODE 0:
//   M = m_{n-2}[1832..1879] ++ m_{n-1}[0..1191]   (1240)  -> D_n[0..187]
//    ++ m_{n-1}[1832..1879] ++ m_n[0..103]        (152)   -> F_{n+1}[0..101]
// MODE 1:
//   M = m_{n-2}[1832..1879] ++ m_{n-1}[0..1701]   (1750)  -> D_n[0..289]
// TU (255 correlator terms, permuted) reuses M once the FIR is done.  MODE 1
// keeps one dec buffer per front wave (LDS budget); the previous channel's
// window is read from it before the FIR overwrites it (same wave, in order).
constexpr int kM1 = 1240;
template <int MODE> struct Cfg;
template <> struct Cfg<0> { static constexpr int kM = 1392, kDecBuf = 2; };
template <> struct Cfg<1> { static constexpr int kM = 1750, kDecBuf = 1; };

// (f2, the (re, im) pair type, comes from qpsk_cmul.h)

constexpr unsigned long long kPreLo = qhunt::pre_mask(0), kPreHi = qhunt::pre_mask(1);

// the preamble as +-1.0f, read by the training loops as wave-uniform scalar
// loads (s_load): one per 4 steps instead of bit extraction per step
struct alignas(16) PreTab {
    float v[QK_NPRE];
};
constexpr PreTab make_pretab() {
    PreTab t{};
    for (int i = 0; i < QK_NPRE; i++) t.v[i] = ((i < 64 ? kPreLo >> i : kPreHi >> (i - 64)) & 1ull) ? 1.0f : -1.0f;
    return t;
}
__constant__ PreTab kPreTab = make_pretab();

struct RxArgs {
    const int16_t* in;       // [nch][F][1880]
    int16_t* hist;           // [nch][2][1880]: frames -2, -1 of this call
    const float2* ptab;      // [1880] mixer table P[t] * 2^-14
    const unsigned long long* ks;  // [1057] keystream bits of frame g (mod 1057)
    float2* win0;            // [nslot][168] equalizer windows, even global frames
    float2* win1;            //                                odd global frames
    int* mi0;                // [nslot] preamble position (even / odd frames)
    int* mi1;
    int* rt0;                // [nslot] rx_timing (even / odd frames)
    int* rt1;
    uint8_t* bits;           // [nch][F][62]
    uint8_t* valid;          // [nch][F]
    int32_t* trace;          // [nch][F][4] or null
    float2* soft;            // [nch][F][31] or null
    float4* jobs;            // data-symbol jobs of valid frames (rx_data_kernel)
    unsigned* njobs;         // their count (this call's counter)
    int nch, F;
    unsigned g0;             // global index of the call's first frame
    size_t jcap;             // job queue capacity (plane stride of the jobs)
    int roles;               // read with the roles_* getters (qpsk_rx_shared.h, "roles word")
    int* err;                // device error word (kErrStall)
    const float2* heads;     // [nch][F][102] head pre-pass outputs (HP), or null
};

// Diagnostic build only (-DQPSK_STAMPS): per-phase cycle sums of the front
// wave, read back with qpsk_debug_stamps().  In the product build every stamp
// is compiled out.
#ifdef QPSK_STAMPS
__device__ unsigned long long g_stamps[16];
#define STAMP_DECL unsigned long long st_acc[16] = {}; unsigned long long st_t0 = stamp_now();
#define STAMP(i) do { const unsigned long long t_ = stamp_now(); st_acc[i] += t_ - st_t0; st_t0 = t_; } while (0)
#define STAMP_FLUSH() do { if (lane == 0) for (int i_ = 0; i_ < 16; i_++) atomicAdd(&g_stamps[i_], st_acc[i_]); } while (0)
__device__ __forceinline__ unsigned long long stamp_now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#else
#define STAMP_DECL
#define STAMP(i) do { } while (0)
#define STAMP_FLUSH() do { } while (0)
#endif

__device__ __forceinline__ float2* win_of(const RxArgs& a, unsigned g) { return (g & 1u) ? a.win1 : a.win0; }
__device__ __forceinline__ int* mi_of(const RxArgs& a, unsigned g) { return (g & 1u) ? a.mi1 : a.mi0; }
__device__ __forceinline__ int* rt_of(const RxArgs& a, unsigned g) { return (g & 1u) ? a.rt1 : a.rt0; }

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Dual-chain kernel (rx_kernel<.., DUAL = true>): per-frame progress counters
// in LDS instead of a workgroup barrier.  Every wave of the (single) workgroup
// is resident, and every counter is advanced by every frame of its producer,
// so each wait ends.  The bound keeps a logic error from hanging the GPU: a
// wait that runs out sets kErrStall in the call's device error word, which
// the host returns as QPSK_ESTALL (qpsk_rx_sync / qpsk_rx_batch /
// qpsk_stream_retrieve), so stale windows or rx_timing never pass as a result.
// The timeout is sticky per workgroup: it also sets the LDS word `dead`, and
// every later wait of the workgroup returns at once, so a broken counter costs
// one bound per workgroup, not one per frame.
constexpr unsigned kSpinBound = 1u << 22;   // ~0.1 s; a frame is ~2.5k spins

__device__ __forceinline__ void spin_wait(int* p, int v, int* err, int* dead,
                                          unsigned bound = kSpinBound) {
    unsigned it = 0;
    for (; it < bound; it++) {
        const int c = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        const int d = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (c >= v || d != 0) break;
        __builtin_amdgcn_s_sleep(1);
    }
    if (it == bound && __lane_id() == 0) {
        __hip_atomic_store(dead, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        atomicOr(err, kErrStall);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// publish: every earlier store of this wave (LDS and global) is visible to the
// workgroup before the counter moves
__device__ __forceinline__ void signal_add(int* p, int v, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ const int16_t* frame_ptr(const RxArgs& a, int ch, int k) {
    return k >= 0 ? a.in + ((size_t)ch * a.F + k) * QK_FRAME
                  : a.hist + ((size_t)ch * 2 + (k + 2)) * QK_FRAME;
}

}  // namespace
