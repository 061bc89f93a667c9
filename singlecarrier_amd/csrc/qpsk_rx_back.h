// qpsk_rx_back.h -- the lane-per-channel back wave of the receive kernels: the
// square-root Kalman equalizer's training, the data-symbol job queue and the
// data-symbol kernel (included by qpsk_rx.hip only).
#pragma once

#include "qpsk_rcp.h"
#include "qpsk_rx_dev.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------- back role
// The complex products cmul / cmulc (inline form) and cmul_t / cmulc_t<EXACT>
// (EXACT: with the Annex G recovery the reference's compiler adds) are in
// qpsk_cmul.h.
// a + conj(b) = (a.x + b.x, a.y + (-b.y)), one packed add
__device__ __forceinline__ f2 addc(f2 a, f2 b) {
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f2 conj2(f2 A) { return f2{A.x, -A.y}; }

struct Kal {
    f2 eq[5];                // eq_coeff     src/kalman.c:19
    f2 g[5];                 // kalman_gain  src/kalman.c:20
    f2 u[10];                // u[i][j], i < j (src/kalman.c:25), index uix(i, j)
    f2 d[5];                 // src/kalman.c:29, kept as (d, d) for packed g = f*d
};

__host__ __device__ constexpr int uix(int i, int j) { return j * (j - 1) / 2 + i; }

// kalman_calculate (src/kalman.c:85-141) then update_eq (src/equalizer.c:25-40)
// EXACT = false: the five divisions use the fast correctly-rounded reciprocal
// (qpsk_rcp.h), valid inside [2^-125, 2^125], and the complex products their
// inline form (qpsk_cmul.h), which is the whole product while no value is
// inf or NaN.  `bad` collects lanes whose frame left either premise -- tone-like
// full-scale input does that: the equalizer state overflows fp32 inside a
// frame -- and the caller then recomputes the whole frame with EXACT = true
// (IEEE division, products with the Annex G recovery, 6.5/6.6 from the full
// product).  No branch in the step, so the step is one basic block.
// the gain half of update_eq: kalman_calculate (src/kalman.c:85-141); returns
// kalman_y (the last 6.22 y).  It never reads eq or the error: the gain
// recursion of a frame depends only on its window.
// EXACT = false: `bmax` collects the bit pattern of the step's largest
// reciprocal operand xs[4] (the callers test bmax <= bits(2^125) once per
// frame or job: qk_rcp_in_range() for every step, a NaN or -x has larger bits).
template <bool EXACT>
__device__ __forceinline__ float kal_gain(Kal& k, const f2 (&x)[5], unsigned& bmax) {
    const float E = QK_KAL_E, q = QK_KAL_Q;
    f2 f[5];
    float a[5];
    f[0] = conj2(x[0]);                                   // 6.2  f0 = conj(x0)
#pragma unroll
    for (int j = 1; j < 5; j++) {
        // u0j*conj(x0) + conj(xj) (the double conj() sum rounds to the fp32 sum)
        f[j] = addc(cmulc_t<EXACT>(k.u[uix(0, j)], x[0]), x[j]);
#pragma unroll
        for (int i = 1; i < j; i++) f[j] = f[j] + cmulc_t<EXACT>(k.u[uix(i, j)], x[i]);
    }
#pragma unroll
    for (int j = 0; j < 5; j++) k.g[j] = f[j] * k.d[j];   // 6.4  g = f*d (both halves d)
#pragma unroll
    for (int j = 0; j < 5; j++) {                         // 6.5/6.6 Re(g * conj(f))
        // gr*fr - gi*(-fi) == gr*fr + gi*fi (gi*(-fi) == -(gi*fi) exactly).
        // EXACT: crealf() of the whole product, whose recovery looks at the
        // imaginary part too
        const f2 t = k.g[j] * f[j];
        const float re = EXACT ? cmulc_g(k.g[j], f[j]).x : t.x + t.y;
        a[j] = (j == 0 ? E : a[j - 1]) + re;
    }
    const float hq = 1.0f + q;                            // 6.7
    const float ht = a[4] * q;
    // the five divisor operands of 6.19 / 6.22.  They are nondecreasing in j:
    // a_j = a_{j-1} + (gr*fr + gi*fi) and every g*conj(f) term is >= 0 (g = f*d,
    // d > 0), so xs[0] >= E = 0.1 and xs[4] is the largest; one check of xs[4]
    // (false for +inf/NaN, which propagate into a_4) covers all five
    // (qk_rcp_fast == 1.0f / x inside [2^-125, 2^125], see qpsk_rcp.h).
    float xs[5], ys[5];
#pragma unroll
    for (int j = 0; j < 5; j++) xs[j] = a[j] + ht;
    if (EXACT) {
#pragma unroll
        for (int j = 0; j < 5; j++) ys[j] = qk_div_ieee(xs[j]);
    } else {
        // the one check: xs[0] >= E unless NaN, and a NaN reaches xs[4] too
        bmax = max(bmax, __float_as_uint(xs[4]));
        // (the Newton steps as packed pairs: 15 fewer instructions per 4
        // steps but 4 more spilled VGPRs in the 4x2 kernel, C3 +0.8%,
        // profiles/r05_knobs_ab.txt, code in commit 868e9f0)
#pragma unroll
        for (int j = 0; j < 5; j++) ys[j] = qk_rcp_fast(xs[j]);
    }
    float y = ys[0];                                      // 6.19
    k.d[0] = k.d[0] * ((hq * (E + ht)) * y);              // 6.20 (both halves)
#pragma unroll
    for (int j = 1; j < 5; j++) {
        const float B = a[j - 1] + ht;                    // 6.21
        const f2 h = (-f[j]) * y;                         // 6.11
        y = ys[j];                                        // 6.22
        k.d[j] = k.d[j] * ((hq * B) * y);                 // 6.13
#pragma unroll
        for (int i = 0; i < j; i++) {
            const f2 B1 = k.u[uix(i, j)];
            k.u[uix(i, j)] = B1 + cmulc_t<EXACT>(h, k.g[i]);   // 6.15
            k.g[i] = k.g[i] + cmulc_t<EXACT>(k.g[j], B1);      // 6.16
        }
    }
    return y;
}

// update_eq (src/equalizer.c:25-40): the gain, then error *= kalman_y and
// eq_i += error * conj(g_i)
template <bool EXACT>
__device__ __forceinline__ void update_eq(Kal& k, const f2 (&x)[5], f2 e, unsigned& bmax) {
    const float y = kal_gain<EXACT>(k, x, bmax);
    e = e * y;                                            // error *= kalman_y
#pragma unroll
    for (int i = 0; i < 5; i++) k.eq[i] = k.eq[i] + cmulc_t<EXACT>(e, k.g[i]);
}

// True unless eq, u or d holds an inf or a NaN (v * 0 is 0 for a finite v and
// NaN otherwise; no contraction, no fast-math: the products stay).
//
// Why one test of the state after a frame's (or job's) steps finds every step
// whose inline product was not the reference's.  The inline form differs from
// the reference's product only where both of its parts are NaN, which takes an
// inf or NaN among its operands or its four partial products.  Every product
// of a step ends in the carried state or in the checked divisor:
//   u*conj(x) -> f -> g = f*d -> Re(g conj f) -> a_j -> a_4 + ht   (bmax)
//   h*conj(g) -> u;  g_j*conj(B1) -> g_i -> e*conj(g_i) -> eq;
//   x*eq -> val -> e -> e*conj(g) -> eq
// (an inf or NaN factor makes a product inf or NaN whatever the other factor
// is, so `e * y` and `e * conj(g)` pass it on even through a zero).  And the
// state keeps it: eq and u only ever change by `+=`, d by `*=`, and inf or NaN
// plus or times anything is inf or NaN.  The state is reset per frame
// (kal_reset), so nothing crosses into the next one.  The test is outside the
// steps: finite frames run the loops they always ran.
__device__ __forceinline__ bool kal_finite(const Kal& k) {
    f2 z = {0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 5; i++) z = z + k.eq[i] * 0.0f;
#pragma unroll
    for (int i = 0; i < 10; i++) z = z + k.u[i] * 0.0f;
#pragma unroll
    for (int i = 0; i < 5; i++) z = z + k.d[i] * 0.0f;
    return z.x + z.y == 0.0f;
}

// A valid frame handed from the back wave to rx_data_kernel: the window
// samples of its data symbols, the equalizer state after the 128 training
// steps, and where its outputs go.  112 floats (28 x 16 B), plane-major: 16-B
// word q of job slot s is at jobs[q * cap + s] (cap = the queue's capacity), so
// the lanes of a wave, which hold consecutive slots, read and write adjacent
// 16-B words (one uncoalesced 448-B job per lane touched 64 cache lines per
// load instruction):
//   [0, 70)  x = dec[mi+128+t], t < 35, as (re, im)
//   [70, 80) eq[5]   [80, 100) u[10]   [100, 105) d[5] (one copy of each)
//   [105, 107) cf (channel-frame index, 64-bit)   [107] keystream frame index
struct DataJob {
    Kal k;
    size_t cf;
    unsigned ks;
};

__device__ __forceinline__ int lane_id() { return __lane_id(); }

// one job float (compile-time index i < 112) from its source
__device__ __forceinline__ float job_word(int i, const DataJob& j, const float* xf) {
    if (i < 70) return xf[i];
    if (i < 80) return (i & 1) ? j.k.eq[(i - 70) >> 1].y : j.k.eq[(i - 70) >> 1].x;
    if (i < 100) return (i & 1) ? j.k.u[(i - 80) >> 1].y : j.k.u[(i - 80) >> 1].x;
    if (i < 105) return j.k.d[i - 100].x;
    if (i == 105) return __uint_as_float((unsigned)(j.cf & 0xffffffffu));
    if (i == 106) return __uint_as_float((unsigned)(j.cf >> 32));
    if (i == 107) return __uint_as_float(j.ks);
    return 0.0f;
}

// Streamed: each 16-B store right after the window loads it needs (the job
// queue may alias the window as far as the compiler knows, so staging the
// whole job first would hold all 112 floats in registers).
// Addresses: plane base (wave-uniform, SGPRs) + 32-bit lane byte offset slot * 16
// (global_load/store saddr form; the queue holds < 2^28 jobs, qpsk_rx_batch_device).
__device__ __forceinline__ const char* job_plane(const float4* jobs, size_t cap, int q) {
    return reinterpret_cast<const char*>(jobs) + (size_t)q * cap * sizeof(float4);
}

__device__ __forceinline__ void put_job(float4* jobs, size_t cap, unsigned slot, const DataJob& j,
                                        const f2* x35) {
    const float* xf = reinterpret_cast<const float*>(x35);
    const unsigned off = slot * (unsigned)sizeof(float4);
#pragma unroll
    for (int q = 0; q < kJobF4; q++)
        *reinterpret_cast<float4*>(const_cast<char*>(job_plane(jobs, cap, q)) + off) = make_float4(job_word(4 * q, j, xf), job_word(4 * q + 1, j, xf),
                             job_word(4 * q + 2, j, xf), job_word(4 * q + 3, j, xf));
}

__device__ __forceinline__ void get_job(const float4* jobs, size_t cap, unsigned off, DataJob& j) {
    float v[112];
#pragma unroll
    for (int q = 17; q < kJobF4; q++) {   // floats 68..111 (state and indices)
        const float4 w = *reinterpret_cast<const float4*>(job_plane(jobs, cap, q) + off);
        v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
    }
#pragma unroll
    for (int t = 0; t < 5; t++) j.k.eq[t] = f2{v[70 + 2 * t], v[71 + 2 * t]};
#pragma unroll
    for (int t = 0; t < 10; t++) j.k.u[t] = f2{v[80 + 2 * t], v[81 + 2 * t]};
#pragma unroll
    for (int t = 0; t < 5; t++) { j.k.d[t] = f2{v[100 + t], v[100 + t]}; j.k.g[t] = f2{0.0f, 0.0f}; }
    j.cf = (size_t)__float_as_uint(v[105]) | ((size_t)__float_as_uint(v[106]) << 32);
    j.ks = __float_as_uint(v[107]);
}

// Window reads are plain loads: the window was stored by the front wave of this
// workgroup before the frame's __syncthreads(), which makes it visible to the
// whole workgroup (same CU).  (Non-temporal loads re-fetch each line from L2/HBM
// per step: 2x the traffic in profiles/calib.)
__device__ __forceinline__ float4 ldw(const float4* p) { return *p; }

// kalman_reset, src/kalman.c:42-55
__device__ __forceinline__ Kal kal_reset() {
    Kal k;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        k.eq[i] = k.g[i] = f2{0.0f, 0.0f};
        k.d[i] = f2{1.0f, 1.0f};
    }
#pragma unroll
    for (int i = 0; i < 10; i++) k.u[i] = f2{0.0f, 0.0f};
    return k;
}

// window slots 1..5 = dec[mi .. mi+4]
__device__ __forceinline__ void load_x0(const float4* wp, f2 (&x)[5]) {
    const float4 w0 = ldw(wp + 0), w1 = ldw(wp + 1), w2 = ldw(wp + 2);
    x[0] = f2{w0.z, w0.w};
    x[1] = f2{w1.x, w1.y};
    x[2] = f2{w1.z, w1.w};
    x[3] = f2{w2.x, w2.y};
    x[4] = f2{w2.z, w2.w};
}

// 128 x train_eq (src/equalizer.c:45-58) from the window; returns matches.
// (The window load one step ahead stays: a 4-step ring loaded an iteration
// ahead, as qtrain's, changes this loop's schedule to one with ~50 s_nop per
// step in the 4x2 kernel.)
template <bool EXACT, typename PollFn>
__device__ __forceinline__ int train(Kal& k, f2 (&x)[5], const f2* wp2, bool& bad, PollFn poll) {
    int matches = 0;
    unsigned bmax = 0u;
#pragma unroll 4
    for (int i = 0; i < QK_NPRE; i++) {
        if ((i & 3) == 0) poll();                  // every 4 steps (dynamic priority)
        const f2 nx = wp2[i + 6];                  // slot i+6 (next step)
        const float ref = kPreTab.v[i];            // wave-uniform scalar load (kPreTab)
        f2 v = {0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 5; t++) v = v + cmul_t<EXACT>(x[t], k.eq[t]);
        const float er = ref - v.x;                // conjf(ref - val) = (ref - vr, vi)
        update_eq<EXACT>(k, x, f2{er, v.y}, bmax);
        if (er * ref > 0.0f) matches++;
#pragma unroll
        for (int t = 0; t < 4; t++) x[t] = x[t + 1];
        x[4] = nx;
    }
    // out of the fast path's premises: a divisor outside the reciprocal's
    // range, or an inf / NaN in the state (see kal_finite)
    if (!EXACT) bad |= bmax > __float_as_uint(0x1p125f) || !kal_finite(k);
    return matches;
}

// One frame of the back wave: lane = channel.  Window slots 1..163 hold
// dec[mi .. mi+162]; read two slots (16 B) every two steps.
// get_rt() yields rx_timing of frame n; it is called only after the training,
// so the dual-chain kernel can wait for the previous frame's decision there.
template <typename RtFn, typename PollFn>
__device__ __forceinline__ void back_frame(const RxArgs& a, int ch, bool live, int n, int mi,
                                           RtFn get_rt, const float2* win, int* rt_next,
                                           PollFn poll) {
    const float4* wp = reinterpret_cast<const float4*>(win);
    Kal k = kal_reset();
    f2 x[5];
    load_x0(wp, x);
    // equalize(): 128 x train_eq (src/qpsk.c:111-123, src/equalizer.c:45-58)
    const f2* wp2 = reinterpret_cast<const f2*>(win);
    bool bad = roles_force_exact(a.roles);
    int matches = train<false>(k, x, wp2, bad, poll);
    if (__builtin_expect(__ballot(bad) != 0ull, 0)) {   // recompute the frame exactly
        k = kal_reset();
        load_x0(wp, x);
        matches = train<true>(k, x, wp2, bad, poll);
    }
    const bool valid = live && matches > QK_MATCH_MIN;   // src/qpsk.c:196
    const size_t cf = (size_t)ch * a.F + n;
    // Valid frames continue in rx_data_kernel (data_eq needs nothing the next
    // frame depends on): enqueue the equalizer state and the 35 window samples
    // of the data symbols.  One slot reservation per wave.
    const unsigned long long vm = __ballot(valid);
    if (vm) {
        unsigned base = 0;
        if (lane_id() == 0) base = atomicAdd(a.njobs, (unsigned)__popcll(vm));
        base = __builtin_amdgcn_readfirstlane(base);
        if (valid) {
            const unsigned slot = base + (unsigned)__popcll(vm & ((1ull << lane_id()) - 1ull));
            DataJob j;
            j.k = k;
            j.cf = cf;
            j.ks = (a.g0 + (unsigned)n) % QK_KS_FRAMES;
            put_job(a.jobs, a.jcap, slot, j, wp2 + 129);
        }
    }
    if (live && !valid) {   // invalid frame: bits (and soft symbols) are zero
        uint16_t* bo = reinterpret_cast<uint16_t*>(a.bits + cf * QK_NBITS);
        for (int ss = 0; ss < QK_NDSYM; ss++) bo[ss] = 0;
        if (a.soft) {
            float2* so = a.soft + cf * QK_NDSYM;
            for (int ss = 0; ss < QK_NDSYM; ss++) so[ss] = make_float2(0.0f, 0.0f);
        }
    }
    const int rt = get_rt();
    const int rtn = valid ? mi + QK_NPRE : rt;    // src/qpsk.c:219
    if (rt_next) *rt_next = rtn;   // null: a lane past its block (no channel)
    if (live) {
        a.valid[cf] = valid ? 1 : 0;
        if (a.trace)
            *reinterpret_cast<int4*>(a.trace + cf * 4) = make_int4(mi, matches, valid ? 1 : 0, rtn);
    }
}

// 31 x data_eq + qpsk_demod (src/equalizer.c:64-90, src/qpsk.c:268-271) from
// the job's window samples xs; returns the raw dibits (bit 2s = Q, 2s+1 = I).
// Decisions collect in a register; the caller stores the 62 bytes after the
// loop, so no wait on a store sits inside it.
// the job's window samples: x[t] is float2 (t & 1) of 16-B word t >> 1
struct JobX {
    const float4* jobs;
    size_t cap;
    unsigned off;   // slot * 16
    __device__ __forceinline__ f2 operator[](int t) const {
        return *reinterpret_cast<const f2*>(job_plane(jobs, cap, t >> 1) + off + 8u * (t & 1));
    }
};

constexpr int kDataRing = 4;   // job samples loaded this many steps ahead (profiles/r02_data_ring_ab.txt)
template <bool EXACT>
__device__ __forceinline__ void data_step(Kal& k, f2 (&x)[5], f2 nx, int s, unsigned long long& dib,
                                          float2* so, unsigned& bmax) {
    f2 sy = {0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 5; t++) sy = sy + cmulc_t<EXACT>(x[t], k.eq[t]);
    const int dI = sy.x < 0.0f, dQ = sy.y < 0.0f;
    const f2 cst = {dI ? -1.0f : 1.0f, dQ ? -1.0f : 1.0f};
    update_eq<EXACT>(k, x, (cst - sy) * 0.1f, bmax);
    dib |= (unsigned long long)(dQ | (dI << 1)) << (2 * s);
    if (so) so[s] = make_float2(sy.x, sy.y);
#pragma unroll
    for (int t = 0; t < 4; t++) x[t] = x[t + 1];
    x[4] = nx;
}

template <bool EXACT>
__device__ __forceinline__ unsigned long long data_steps(Kal& k, f2 (&x)[5], const JobX xs,
                                                         float2* so, bool& bad) {
    unsigned long long dib = 0;
    unsigned bmax = 0u;
    // the job's samples arrive from HBM (written ~ms earlier by rx_kernel):
    // each is loaded R steps before it enters x
    constexpr int R = kDataRing;
    f2 cur[R];
#pragma unroll
    for (int t = 0; t < R; t++) cur[t] = xs[min(5 + t, 34)];
    for (int s0 = 0; s0 < QK_NDSYM; s0 += R) {
        f2 nxt[R];
#pragma unroll
        for (int t = 0; t < R; t++) nxt[t] = xs[min(s0 + R + 5 + t, 34)];
#pragma unroll
        for (int t = 0; t < R; t++)
            if (s0 + t < QK_NDSYM) data_step<EXACT>(k, x, cur[t], s0 + t, dib, so, bmax);
#pragma unroll
        for (int t = 0; t < R; t++) cur[t] = nxt[t];
    }
    // as in train(): a job that starts from or reaches a non-finite state is
    // redone with the reference's whole products
    if (!EXACT) bad |= bmax > __float_as_uint(0x1p125f) || !kal_finite(k);
    return dib;
}

// ---------------------------------------------------------------- history carry
// The samples the next call needs, from the call's input into the context's
// history [nch][2][1880] (h0, h1): x_{F-1}[0..8 head8) and x_{F-1}[1832..1879]
// into h1, x_{F-2}[1832..1879] into h0; head8 = 149 (1192 samples), or 213
// (1704) in the dec752 mode.  One channel is 16-B units u < head8 + 12, four
// per lane: u < head8 the head, the next 6 h1's tail, the last 6 h0's.
// A wave takes kCarryK channels at a time and waves stride over the channels;
// it issues the loads of all of them before the first store, so each wave keeps
// kCarryK x 4 KB in flight.  A one-frame call's x_{F-2} tail is what h1 holds:
// that load precedes the wave's stores to h1, and no other wave writes the
// channel.
constexpr int kCarryK = 4;       // channels per wave in flight
constexpr int kCarryGrid = 256;  // carry workgroups at most (profiles/carry_data_launch_ab.txt)

typedef int carry_v4 __attribute__((ext_vector_type(4)));   // (an int4 array stays in scratch)
__device__ __forceinline__ void carry_block(const int16_t* in, int16_t* hist, int nch, int F, int head8,
                                            int wave, int nwaves, int lane) {
    const int nunit = head8 + 12;
    for (int c0 = wave * kCarryK; c0 < nch; c0 += nwaves * kCarryK) {
        carry_v4 v[kCarryK][4];
#pragma unroll
        for (int k = 0; k < kCarryK; k++) {
            // (a lane past the batch's channels or the channel's units loads the
            // last one's again and stores nothing: every load is unconditional)
            const int ch = min(c0 + k, nch - 1);
            const int16_t* h1 = hist + ((size_t)ch * 2 + 1) * QK_FRAME;
            const int16_t* last = in + ((size_t)ch * F + (F - 1)) * QK_FRAME;
            const int16_t* prev = F >= 2 ? last - QK_FRAME : h1;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = min(lane + 64 * j, nunit - 1);
                const int16_t* src = u < head8       ? last + 8 * u
                                     : u < head8 + 6 ? last + 1832 + 8 * (u - head8)
                                                     : prev + 1832 + 8 * (u - head8 - 6);
                v[k][j] = *reinterpret_cast<const carry_v4*>(src);
            }
        }
#pragma unroll
        for (int k = 0; k < kCarryK; k++) {
            const int ch = c0 + k;
            int16_t* h0 = hist + (size_t)ch * 2 * QK_FRAME;
            int16_t* h1 = h0 + QK_FRAME;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = lane + 64 * j;
                if (ch < nch && u < nunit) {
                    int16_t* dst = u < head8       ? h1 + 8 * u
                                   : u < head8 + 6 ? h1 + 1832 + 8 * (u - head8)
                                                   : h0 + 1832 + 8 * (u - head8 - 6);
                    *reinterpret_cast<carry_v4*>(dst) = v[k][j];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- data kernel
// The 31 data symbols of every valid frame (src/qpsk.c:204-215: data_eq
// src/equalizer.c:64-90, qpsk_demod src/qpsk.c:268-271, scramble
// src/scramble.c:57-84), one job per lane, packed: only ~1 frame in 5 is
// valid, so running them inside the lane-per-channel back wave would idle most
// lanes for 31 of its 159 steps.  Jobs come from the call's rx_kernel in any
// order; every output location is fixed by the job, so results do not depend
// on it.
// The launch's first ncarry workgroups carry the sample history instead
// (carry_block): the jobs keep the VALU busy and leave the memory system
// nearly idle, so the copy runs beside them.  The call's rx_kernel, which reads
// the history for its first frame, is done (stream order), and the next
// call's comes after this launch.
// The descrambler word is the one place where a frame's index shows in the
// outputs, and it is applied here: a job carries the word of the call's own
// frame index (j.ks), and koff[channel] moves it to the channel's.
__global__ void __launch_bounds__(256) rx_data_kernel(const float4* jobs, unsigned long long jcap,
                                                      unsigned* njobs,
                                                      const unsigned long long* ks_tab,
                                                      const unsigned* koff, uint8_t* bits, float2* soft, int parity,
                                                      int force_exact, int* err, int* err_to,
                                                      const int16_t* in, int16_t* hist, int nch, int F,
                                                      int head8, unsigned ncarry) {
    if (blockIdx.x < ncarry) {
        // ncarry >= 1, so workgroup 0 always carries; its first thread has the
        // launch's two single-thread duties (on a job workgroup's they keep the
        // job index live over the loop: 15 spilled SGPRs and a 159th VGPR)
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            // err_to (host calls, qpsk_rx_batch): the context's error word, taken in one
            // atomic exchange after rx_kernel (stream order), stored with the outputs:
            // no separate launch for it
            if (err_to) *err_to = atomicExch(err, 0);
            // the next call's counter (calls on one context are stream-ordered)
            njobs[parity ^ 1] = 0u;
        }
        carry_block(in, hist, nch, F, head8, (int)(blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64),
                    (int)(ncarry * (blockDim.x / 64)), lane_id());
        return;
    }
    // the job workgroups follow the carry workgroups
    const size_t cap = (size_t)jcap;
    const unsigned n = njobs[parity];
    const unsigned stride = (gridDim.x - ncarry) * blockDim.x;
    for (unsigned i = (blockIdx.x - ncarry) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned off = i * (unsigned)sizeof(float4);
        DataJob j;
        get_job(jobs, cap, off, j);
        const JobX xs{jobs, cap, off};   // x = dec[mi+128+t], t < 35
        f2 x[5];
#pragma unroll
        for (int t = 0; t < 5; t++) x[t] = xs[t];
        // the channel's own frame index, koff[ch] frames ahead of the call's
        // (mod 1057; zero unless the channel was reset or joined on its own):
        // ch = cf / F, 32-bit (cf < 2^28, qpsk_rx_launch)
        unsigned kw = j.ks + koff[(unsigned)j.cf / (unsigned)F];
        if (kw >= (unsigned)QK_KS_FRAMES) kw -= (unsigned)QK_KS_FRAMES;
        const unsigned long long ks = ks_tab[kw];
        float2* so = soft ? soft + j.cf * QK_NDSYM : nullptr;
        bool bad = force_exact != 0;
        unsigned long long dib = data_steps<false>(j.k, x, xs, so, bad);
        if (__builtin_expect(bad, 0)) {   // recompute the job exactly (EXACT = true)
            get_job(jobs, cap, off, j);
#pragma unroll
            for (int t = 0; t < 5; t++) x[t] = xs[t];
            dib = data_steps<true>(j.k, x, xs, so, bad);
        }
        dib ^= ks;   // descramble (src/scramble.c:57-84): keystream bits 62g .. 62g+61
        uint16_t* bo = reinterpret_cast<uint16_t*>(bits + j.cf * QK_NBITS);
#pragma unroll
        for (int q = 0; q < QK_NDSYM; q++)
            bo[q] = (uint16_t)(((dib >> (2 * q)) & 1ull) | (((dib >> (2 * q + 1)) & 1ull) << 8));
    }
}
}  // namespace
