// qpsk_rx_plan.h -- the decisions of the receive path's host side that are
// plain arithmetic: which rx_kernel instantiation a batch gets, how the
// host-memory entry point lays out its staging block, and how large a state
// snapshot is.  No HIP runtime call, so all of it runs (and is tested,
// tests/test_rx_plan.py) without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_consts.h"
#include "qpsk_rx_shared.h"

// ---------------------------------------------------------------- knobs
// The environment's test, profiling and A/B settings of a context
// (ctx_read_env, qpsk_rx_host.hip).
struct RxKnobs {
    // roles + front issue priority + front stagger (0 since round 5; 12 x 512
    // cycles was -0.7% in round 1, profiles/r01_stagger_ab.txt); QPSK_ABLATE
    // (profiling), QPSK_FORCE_EXACT / QPSK_DEBUG_STALL (tests)
    int roles = roles_with_stagger(roles_with_prio(kRoleBack | kRoleFront, kPrioFront), kStagger);
    int shape = -1;          // Shape::Kind forced by QPSK_SHAPE (A/B runs); -1: by batch size
    int width = 0;           // dual-chain group width forced by QPSK_WIDTH; 0: by batch size
    int prio = -1;           // issue priority forced by QPSK_PRIO (a RolePrio); -1: by shape
    bool headpass = false;   // QPSK_HEADPASS: the FIR-head pre-pass (reference mode only)
    int stall_calls = -1;    // QPSK_DEBUG_STALL=first: the stall only in the first launch; -1: every call
    int short_block = 0;     // QPSK_DEBUG_BLOCK (tests): rx_kernel launched one wave short
};

// ---------------------------------------------------------------- kernel shape
// The rx_kernel instantiation for a context of nch channels on a device of ncu
// compute units (DESIGN.md "Kernels"):
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
inline Shape pick_shape(const RxKnobs& k, int nch, int ncu) {
    const int ngroup = (nch + QK_GROUP - 1) / QK_GROUP;
    Shape sh{k.shape, k.roles};
    if (sh.kind < 0)
        sh.kind = ngroup <= ncu ? Shape::k1x8d64 : ngroup <= 2 * ncu ? Shape::k2x4d : Shape::k4x2;
    if (sh.kind == Shape::k1x8d64) {
        const int W = k.width > 0 ? k.width
                    : (size_t)nch <= (size_t)16 * ncu ? 16
                    : (size_t)nch <= (size_t)32 * ncu ? 32 : 64;
        if (W == 16) sh.kind = Shape::k1x8q16;
        else if (W == 32) sh.kind = Shape::k1x8q32;
        else sh.roles = roles_with_split(roles_with_prio(sh.roles, kPrioBack), 2);
    }
    if (k.prio >= 0) sh.roles = roles_with_prio(sh.roles, k.prio);
    return sh;
}

// ---------------------------------------------------------------- pointer alignment
// What the receive kernels need of a call's device pointers (include/qpsk_input.h
// "Pointer rules of the device receive calls"): the fronts load the input as
// int4, a trace row is one int4 store, soft symbols are float2 stores and a
// symbol's two bits one uint16_t store (back_frame, back_frame_quad,
// rx_data_kernel); the valid flags are byte stores.  A channel's row keeps the
// alignment: rows are 62 (bits), 16 (trace) and 248 (soft) bytes, frames 3760.
constexpr uintptr_t kAlignIn = 16, kAlignTrace = 16, kAlignSoft = 8, kAlignBits = 2;
static_assert(QK_NBITS % kAlignBits == 0 && (sizeof(int32_t) * 4) % kAlignTrace == 0 &&
              (sizeof(float) * 2 * QK_NDSYM) % kAlignSoft == 0 && (sizeof(int16_t) * QK_FRAME) % kAlignIn == 0,
              "a view that starts at a channel row keeps the alignment");
// The alignment rule alone: a NULL pointer passes (which pointers may be NULL
// is the entry point's own check), and valid may lie anywhere.
inline bool rx_ptrs_aligned(const void* in, const void* bits, const void* valid, const void* trace,
                            const void* soft) {
    auto ok = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    (void)valid;
    return ok(in, kAlignIn) && ok(bits, kAlignBits) && ok(trace, kAlignTrace) && ok(soft, kAlignSoft);
}

// ---------------------------------------------------------------- staging block
// The host-memory entry point (qpsk_rx_batch) stages a call through one block
// [in | bits | valid | err | trace | soft]: byte offsets for cf channel-frames.
struct Stage {
    size_t in, bits, valid, err, trace, soft, end;
};
inline Stage stage_of(size_t cf) {
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

// A block of that layout at `base` (device memory, or its pinned host image),
// as the pointers a call takes
struct StageView {
    char* base;
    Stage g;
    int16_t* in() const { return reinterpret_cast<int16_t*>(base + g.in); }
    uint8_t* bits() const { return reinterpret_cast<uint8_t*>(base + g.bits); }
    uint8_t* valid() const { return reinterpret_cast<uint8_t*>(base + g.valid); }
    int* err() const { return reinterpret_cast<int*>(base + g.err); }
    int32_t* trace() const { return reinterpret_cast<int32_t*>(base + g.trace); }
    float* soft() const { return reinterpret_cast<float*>(base + g.soft); }
};

// ---------------------------------------------------------------- state snapshots
// qpsk_batch.h qpsk_rx_state_*: a 64-byte header, then history, window row, mi
// and rt of the n channels, each field as one contiguous block.
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
constexpr size_t kHistB = sizeof(int16_t) * 2 * QK_FRAME, kWinB = sizeof(float) * 2 * kWinStride;
constexpr size_t kChanB = kHistB + kWinB + 2 * sizeof(int);
constexpr int kWinObs = QK_NPRE + QK_NDSYM + 5;   // slots 0..163 = dec[mi-1 .. mi+162]
static_assert(kWinObs == 164 && kWinObs <= kWinStride, "window slots");

inline size_t rx_state_size(int n) { return n < 1 ? 0 : sizeof(StateHdr) + (size_t)n * kChanB; }

// ---------------------------------------------------------------- channel frame index
// A channel that was reset or joined on its own (qpsk_rx_reset_channels,
// qpsk_rx_state_join) counts its frames from another start than its context.
// The host keeps, per channel, lead = own index - context's index as a wrapped
// 64-bit difference: both advance together, so it changes only in those calls.
// Exact for any two indices below 2^64.
inline uint64_t rx_index_lead(uint64_t own, uint64_t ctx) { return own - ctx; }
inline uint64_t rx_own_index(uint64_t ctx, uint64_t lead) { return ctx + lead; }
// What the data kernel adds to a job's descrambler word (koff, qpsk_rx_back.h):
// (own - ctx) mod 1057 in [0, 1057), from the two residues -- not from the
// wrapped difference, since 2^64 mod 1057 != 0.
inline unsigned rx_koff(uint64_t own, uint64_t ctx) {
    const unsigned a = (unsigned)(own % (uint64_t)QK_KS_FRAMES), b = (unsigned)(ctx % (uint64_t)QK_KS_FRAMES);
    return a >= b ? a - b : a + (unsigned)QK_KS_FRAMES - b;
}
// The mixer sign and the state parity stay the context's for every channel
// (negating a channel's mixed samples changes no output), so a
// channel whose lead is odd holds its window row negated with respect to a
// context that counts as the channel does.  Snapshots are written in the
// channel's own convention: save and join negate the row when this is true.
inline bool rx_lead_odd(uint64_t own, uint64_t ctx) { return ((own ^ ctx) & 1u) != 0; }

// state arrays cover whole workgroups of the largest shape (kMaxGroups groups)
inline size_t rx_nslot(int nch) {
    const int ngroup = (nch + QK_GROUP - 1) / QK_GROUP;
    return (size_t)((ngroup + kMaxGroups - 1) / kMaxGroups) * kMaxGroups * QK_GROUP;
}
