// qpsk_rx_shared.h -- all that the receive kernels' translation unit
// (qpsk_rx.hip) and the host code around it (qpsk_rx_host.hip) know of each
// other: the constants that size the host's buffers, the kernel shapes, the
// layout of the `roles` word and the one call that performs a call's launches.
// The context (qpsk_ctx) stays on the host side.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qpsk_batch.h"
#include "qpsk_consts.h"
#include "qpsk_herr.h"   // herr, HCHECK

// A workgroup owns G groups of 64 channels: waves 0..G-1 are their back waves,
// waves G.. are front waves, FP per group (rx_kernel<G, FP>).  Every shape has
// 8 front waves, so the LDS footprint is the same; large batches use G = 4
// (256 channels per CU), smaller ones spread over more CUs with G = 2 or 1.
constexpr int kMaxGroups = 4;
constexpr int kWinStride = 168;        // window row: slot k+1 = dec[mi+k], 84 float4
constexpr int kFftHT = 768 * 2 + 256;   // floats of the FFT hunt's LDS image (fft_hunt, qpsk_rx_front.h)
constexpr int kHeadOut = QK_NHEAD;   // 102 outputs per channel-frame
constexpr int kJobF4 = 28;           // 16-B words of a data-symbol job (DataJob, qpsk_rx_back.h)
constexpr int kErrStall = 1;                // device error word bits
// front stagger, 512-cycle units (roles bits 8-15): round 1 measured 12 as
// -0.7%; on round 5's kernels 0 is -0.4% (profiles/r05_stagger_ab.txt)
constexpr int kStagger = 0;
// rx_data_kernel's job grid: persistent, 4 workgroups of 256 per CU (other geometries
// measured within 2%, profiles/r01_data_ab.txt); the workgroups that carry the
// sample history lead it (kCarryGrid, qpsk_rx_back.h)
constexpr int kDataGrid = 1024, kDataBlock = 256;

// ---------------------------------------------------------------- roles word
// rx_kernel's `roles` argument: the host composes it (qpsk_ctx's initialiser,
// ctx_read_env, pick_shape, qpsk_rx_launch), the kernels read it, both through
// the names below and nowhere by shift and mask.
//   bits 0-1    roles served: back, front (both in production; QPSK_ABLATE)
//   bits 4-5    issue priority boost (RolePrio)
//   bit 6       force exact   bit 7   debug stall
//   bits 8-15   front stagger, 512-cycle units (4x2 fronts)
//   bits 16-19  front split (1x8 lane backs: channels moved between front waves)
//   bit 20      front idle
constexpr int kRoleBack = 1, kRoleFront = 2;
enum RolePrio { kPrioNone = 0, kPrioFront = 1, kPrioBack = 2 };
constexpr int kPrioShift = 4, kPrioMask = 3;
constexpr int kForceExact = 64;   // roles bit: take the exact-division path (tests)
constexpr int kDebugStall = 128;  // roles bit: force one progress wait past its bound (tests)
constexpr int kStaggerShift = 8, kStaggerMask = 255;
constexpr int kSplitShift = 16, kSplitMask = 15;
constexpr int kFrontIdle = 1 << 20;  // roles bit (QPSK_ABLATE=frontidle, profiling; output invalid):
                                     // dual-chain fronts skip their channels from frame 2 on, so
                                     // the back waves train (stale windows) with the SIMDs to themselves

// (the served bits come back as the masked word, not as bool: with a bool
// roles_back() the 4x2 kernels of the head pre-pass and the dec752 / FFT-hunt
// modes spill two more SGPRs, profiles/rx_split_asm.txt)
__host__ __device__ constexpr int roles_back(int r) { return r & kRoleBack; }     // nonzero: serve the backs
__host__ __device__ constexpr int roles_front(int r) { return r & kRoleFront; }   // nonzero: serve the fronts
__host__ __device__ constexpr int roles_prio(int r) { return (r >> kPrioShift) & kPrioMask; }
__host__ __device__ constexpr bool roles_force_exact(int r) { return (r & kForceExact) != 0; }
__host__ __device__ constexpr bool roles_debug_stall(int r) { return (r & kDebugStall) != 0; }
__host__ __device__ constexpr int roles_stagger(int r) { return (r >> kStaggerShift) & kStaggerMask; }
__host__ __device__ constexpr int roles_split(int r) { return (r >> kSplitShift) & kSplitMask; }
__host__ __device__ constexpr bool roles_front_idle(int r) { return (r & kFrontIdle) != 0; }

// host side: the word with one field replaced
constexpr int roles_with_served(int r, int served) { return (r & ~(kRoleBack | kRoleFront)) | served; }
constexpr int roles_with_prio(int r, int prio) { return (r & ~(kPrioMask << kPrioShift)) | (prio << kPrioShift); }
constexpr int roles_with_stagger(int r, int v) { return (r & ~(kStaggerMask << kStaggerShift)) | (v << kStaggerShift); }
constexpr int roles_with_split(int r, int s) { return (r & ~(kSplitMask << kSplitShift)) | (s << kSplitShift); }

// rx_kernel instantiations (pick_shape, qpsk_rx_host.hip); ShapeOf<kind>
// (qpsk_rx.hip) holds a kind's template parameters, the only place that spells
// them
struct Shape {
    enum Kind { k4x2, k2x4d, k1x8d64, k1x8q16, k1x8q32 };
    int kind;
    int roles;
};

// ---------------------------------------------------------------- one call
// Everything the launches of one call take: the context's buffers, the call's
// own, and what selects the rx_kernel instantiation.
struct RxLaunch {
    hipStream_t s;
    int kind;                // Shape::Kind
    int mode;                // QPSK_MODE_* of the context
    bool hp;                 // head pre-pass first (reference mode only)
    int short_block;         // threads rx_kernel's block is launched short (QPSK_DEBUG_BLOCK)
    const int16_t* in;       // as RxArgs (qpsk_rx_dev.h) from here on
    int16_t* hist;
    const float2* ptab;
    const unsigned long long* ks;
    const unsigned* koff;    // [nslot] per channel: (own frame index - the context's) mod 1057
    float2* win[2];
    int* mi[2];
    int* rt[2];
    uint8_t *bits, *valid;
    int32_t* trace;
    float* soft;
    float4* jobs;
    size_t jobs_cap;
    unsigned* njobs;         // [2] counters; the call uses [parity]
    int parity;
    int nch, F;
    unsigned g0;
    int roles;
    const float* fft_tab;    // FFT-hunt tables, or null
    float2* heads;           // head pre-pass outputs (hp)
    int* err;                // the error word rx_kernel's progress waits report to
    int* ctx_err;            // the context's error word, which rx_data_kernel
    int* err_to;             // takes into err_to (nullable)
    hipEvent_t ev_mid, ev_end;   // recorded after rx_kernel / after rx_data_kernel; null: not timed
};

// head_kernel (hp), rx_kernel of the kind, mode and hp, rx_data_kernel, with the
// two optional event records after the latter two; a QPSK_* status
int qpsk_rx_launch_kernels(const RxLaunch& a);
// Takes the error word d_err[0] into d_err[1] in one atomic exchange, on stream s
int qpsk_rx_take_err(int* d_err, hipStream_t s);
