// qpsk_rx_quad.h -- the quad-lane back wave of the receive kernels: four lanes
// per channel split a training step (included by qpsk_rx.hip only).
#pragma once

#include "qpsk_rx_back.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------- quad back
// Small batches (the dual-chain kernel at <= 32 channels per workgroup) are
// bound by the latency of one channel's 128 serial train_eq steps, and a lane
// per channel issues every one of the step's ~234 instructions: one wave
// cannot issue faster than one VALU instruction per ~4.7 cycles
// (profiles/calib/valu_rate_r01.txt), so a step costs ~1,100 cycles however
// idle the SIMD is.  Here a QUAD of lanes owns a channel and splits the step:
// lane c (0..3) of the quad holds
//   row c of u          R[d-1] = u[c][c+d]        (0 past column 4)
//   column c+1 of u     C[d-1] = u[c+1-d][c+1]    (0 above row 0; C[0] is R[0])
//   d[c+1], eq[c] and (lane 3) eq[4]; d[0] is kept by all four lanes,
// computes column c+1's f/g/s/y/d/h, row c's chain of 6.15/6.16 updates and the
// 5-term sums by quad DPP (v_*_dpp quad_perm), ~135 instructions per step.
// Every fp32 operation is the one update_eq() issues, on the same operands and
// in the same order: the prefix sums (a[j], val) run sequentially over the
// quad's lanes, zero padding enters only as (+-0) addends / factors of a
// finite value, which leave every nonzero sum unchanged (the row chains are
// independent across rows: row i uses only its own running g[i] and the
// ORIGINAL g[j], h[j] of the columns right of it, src/kalman.c:131-139).
namespace qd {
constexpr int kB0 = 0x00, kB1 = 0x55, kB2 = 0xAA, kB3 = 0xFF;   // broadcast lane k of the quad
constexpr int kRot1 = 0x93;   // [3,0,1,2]: lane c <- lane c-1 (lane 0 <- lane 3)
constexpr int kRot2 = 0x4E;   // [2,3,0,1]: lane c <- lane c-2
constexpr int kRot3 = 0x39;   // [1,2,3,0]: lane c <- lane c+1
}

template <int CTRL>
__device__ __forceinline__ float qdf(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ f2 qd2(f2 v) { return f2{qdf<CTRL>(v.x), qdf<CTRL>(v.y)}; }
// qd2<CTRL>(v) * m as two v_mul_f32_dpp (the moves fold into the products);
// the empty asm keeps the products scalar, else they pack into a v_pk_mul_f32
// that takes no DPP source and the two moves stay
template <int CTRL>
__device__ __forceinline__ f2 qd_mul(f2 v, float m) {
    float x = qdf<CTRL>(v.x) * m, y = qdf<CTRL>(v.y) * m;
    asm("" : "+v"(x), "+v"(y));
    return f2{x, y};
}

struct QKal {
    f2 R[4];      // R[d-1] = u[c][c+d]
    f2 C[3];      // C[d-2] = u[c+1-d][c+1], d = 2..4
    f2 eqr;       // eq_coeff[c]
    f2 eq4;       // eq_coeff[4] (lane 3)
    f2 dd;        // (d[0], d[c+1]): one packed multiply updates both
};

__device__ __forceinline__ QKal qkal_reset() {   // kalman_reset, src/kalman.c:42-55
    QKal k;
#pragma unroll
    for (int i = 0; i < 4; i++) k.R[i] = f2{0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 3; i++) k.C[i] = f2{0.0f, 0.0f};
    k.eqr = k.eq4 = f2{0.0f, 0.0f};
    k.dd = f2{1.0f, 1.0f};
    return k;
}

// Packed products with the conj() of the reference folded into a negate
// modifier (conj never materialised; (-a)*b == -(a*b) exactly):
// (x.x * d0, (-x.y) * d0) with d0 = dd.x broadcast: conj(x) * d[0]
__device__ __forceinline__ f2 mul_conj_d0(f2 x, f2 dd) {
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0] neg_hi:[1,0]" : "=v"(r) : "v"(x), "v"(dd));
    return r;
}
// (a.x * b.x, a.y * (-b.y)): a * conj(b) componentwise
__device__ __forceinline__ f2 mul_conjb(f2 a, f2 b) {
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (f.x * dc, f.y * dc) with dc = dd.y broadcast
__device__ __forceinline__ f2 mul_dc(f2 f, f2 dd) {
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(f), "v"(dd));
    return r;
}


// one train_eq step (src/equalizer.c:45-58 with update_eq/kalman_calculate,
// exactly update_eq<false>'s operations) on the quad layout.  X0..X4 = x[c+1-d]
// (x[index+t] of the reference), zero before x[0].  Returns er = Re(error).
// Fast path only (fast reciprocal, inline complex products): `bmax` collects
// the bit patterns of the step's largest reciprocal operand (xso, lane c:
// xs[c+1], nondecreasing in j, and >= xs[0] >= E unless NaN); the caller tests
// bmax <= bits(2^125) once per frame, which is qk_rcp_in_range() for every
// step (a NaN or -x has larger bits).  There is no exact quad step: the zero
// padding of this layout is multiplied by h and x, and 0 * inf is NaN, so a
// frame whose state leaves fp32 range is redone a lane per channel
// (back_frame_quad).
__device__ __forceinline__ float qstep(QKal& k, const f2& X0, const f2& X1, const f2& X2, const f2& X3,
                                       const f2& X4, float ref, int c, unsigned& bmax) {
    const float E = QK_KAL_E, q = QK_KAL_Q;
    // 1 where row c has column c+d (d = 2, 3, 4), else 0: h of a missing
    // column is multiplied by 0, so the padding entries of R stay +0
    const float m2 = c < 3 ? 1.0f : 0.0f, m3 = c < 2 ? 1.0f : 0.0f, m4 = c < 1 ? 1.0f : 0.0f;
    // val = sum_t x[t] * eq[t], t = 0..4 in order (src/equalizer.c:49-51); the
    // reference's 0 + x[0]*eq[0] only differs from x[0]*eq[0] in the sign of a
    // zero, which no output observes, so the chain starts with
    // the broadcast itself
    const f2 p = cmul(X1, k.eqr);         // lane c: x[c] * eq[c]
    const f2 p4 = cmul(X0, k.eq4);        // lane 3: x[4] * eq[4]
    // (the empty asm keeps the two components scalar adds, so each folds its
    // DPP source into one v_add_f32_dpp instead of two moves and a packed add)
    float vr = qdf<qd::kB0>(p.x), vi = qdf<qd::kB0>(p.y);
#define QV(CT, P)                                                   \
    vr = vr + qdf<CT>(P.x); vi = vi + qdf<CT>(P.y);                 \
    asm("" : "+v"(vr), "+v"(vi))
    QV(qd::kB1, p); QV(qd::kB2, p); QV(qd::kB3, p); QV(qd::kB3, p4);
#undef QV
    const float er = ref - vr;            // conjf(ref - val) = (ref - vr, vi)
    // column 0 (every lane): f0 = conj(x0), 6.2; g0 = f0 * d0, 6.4; t0 = g0 * f0
    const f2 x0 = qd2<qd::kB0>(X1);
    const f2 g0 = mul_conj_d0(x0, k.dd);
    const f2 t0 = mul_conjb(g0, x0);
    const float a0 = E + (t0.x + t0.y);                   // 6.5
    // column c+1: f = u[0][j]*conj(x0) + conj(xj) + sum_{0<i<j} u[i][j]*conj(xi)
    f2 f = addc(cmulc(k.C[2], X4), X0);
    f = f + cmulc(k.C[1], X3);
    f = f + cmulc(k.C[0], X2);
    f = f + cmulc(k.R[0], X1);
    const f2 g = mul_dc(f, k.dd);                         // 6.4
    const f2 t = g * f;
    const float s = t.x + t.y;
    // 6.6 a[j] = a[j-1] + Re(g conj f), the quad's s in column order
    const float a1 = a0 + qdf<qd::kB0>(s);
    const float a2 = a1 + qdf<qd::kB1>(s);
    const float a3 = a2 + qdf<qd::kB2>(s);
    const float a4 = a3 + qdf<qd::kB3>(s);
    const float hq = 1.0f + q;                            // 6.7
    const float ht = a4 * q;
    const float ap = c == 0 ? a0 : c == 1 ? a1 : c == 2 ? a2 : a3;   // a[c]
    const float ao = ap + s;                              // a[c+1], the chain's own add
    const f2 xs = f2{a0, ao} + f2{ht, ht};               // (xs[0], xs[c+1]), 6.19 / 6.22 operands
    bmax = max(bmax, __float_as_uint(xs.y));
    const f2 y = f2{qk_rcp_fast(xs.x), qk_rcp_fast(xs.y)};
    // 6.20 / 6.21+6.13: d[0] *= (hq * (E + ht)) * y0, d[c+1] *= (hq * (a[c] + ht)) * y[c+1]
    k.dd = k.dd * ((f2{hq, hq} * (f2{E, ap} + f2{ht, ht})) * y);
    const float y0 = y.x, yo = y.y;
    // (every DPP move is made unconditionally, then selected: a move inside
    // a conditional would become a branch, the intrinsic being convergent)
    const float yr = qdf<qd::kRot1>(yo);
    const float yp = c == 0 ? y0 : yr;                    // y[c]
    const f2 h = (-f) * yp;                               // 6.11 h[c+1]
    // row c (6.15/6.16) from g[c]: column c's gain (lane c-1; column 0: g0)
    const f2 gr = qd2<qd::kRot1>(g);
    f2 G = c == 0 ? g0 : gr;
    {   // column c+1: this lane
        const f2 B1 = k.R[0];
        k.R[0] = B1 + cmulc(h, G);
        G = G + cmulc(g, B1);
    }
    {   // column c+2 (lane c+1); none for row 3
        const f2 hd = qd_mul<qd::kRot3>(h, m2);
        const f2 gd = qd2<qd::kRot3>(g);
        const f2 B1 = k.R[1];
        k.R[1] = B1 + cmulc(hd, G);
        G = G + cmulc(gd, B1);
    }
    {   // column c+3 (lane c+2); none for rows 2, 3
        const f2 hd = qd_mul<qd::kRot2>(h, m3);
        const f2 gd = qd2<qd::kRot2>(g);
        const f2 B1 = k.R[2];
        k.R[2] = B1 + cmulc(hd, G);
        G = G + cmulc(gd, B1);
    }
    {   // column c+4 (lane c+3); row 0 only
        const f2 hd = qd_mul<qd::kRot1>(h, m4);
        const f2 B1 = k.R[3];
        k.R[3] = B1 + cmulc(hd, G);
        G = G + cmulc(gr, B1);
    }
    // next step's columns: C[d-2](c) = R[d-1](c+1-d); the lanes with no such
    // row read a padding entry of R (zero) through the rotation
    k.C[0] = qd2<qd::kRot1>(k.R[1]);
    k.C[1] = qd2<qd::kRot2>(k.R[2]);
    k.C[2] = qd2<qd::kRot3>(k.R[3]);
    // update_eq: error *= kalman_y (y[4], lane 3); eq[i] += error * conj(g[i])
    const float y4 = qdf<qd::kB3>(yo);
    const f2 e = f2{er, vi} * y4;
    k.eqr = k.eqr + cmulc(e, G);     // row c's final gain
    k.eq4 = k.eq4 + cmulc(e, g);     // lane 3: g[4] (row 4 has no updates)
    return er;
}

// x[index+t] at step 0: X[d] = x[c+1-d] = window slot c+2-d (slot k+1 = dec[mi+k])
__device__ __forceinline__ void qload_x0(const f2* wp2, int c, f2 (&X)[5]) {
#pragma unroll
    for (int d = 0; d < 5; d++) X[d] = d <= c + 1 ? wp2[c + 2 - d] : f2{0.0f, 0.0f};
}

// The window as a ring of 8 samples per lane, w[s mod 8] = x[c+1] of step s
// (wl[s]; w of a negative step: X of step 0, zero-padded); step s reads
// X[d] = w[(s - d) mod 8].  Eight steps per loop iteration, so the ring's
// roles repeat every iteration and no register moves at the back edge; the
// sample of step s+4 is loaded right after step s, into the slot step s read
// last (reads run to step 131, inside the 168-slot window row).
template <typename PollFn>
__device__ __forceinline__ int qtrain(QKal& k, const f2 (&X)[5], const f2* wl, int c, bool& bad, PollFn poll) {
    int matches = 0;
    unsigned bmax = 0u;
    f2 w[8];
    w[0] = X[0];
    w[7] = X[1];
    w[6] = X[2];
    w[5] = X[3];
    w[4] = X[4];
#pragma unroll
    for (int t = 1; t < 4; t++) w[t] = wl[t];
    for (int i = 0; i < QK_NPRE; i += 8) {
        const float4 r0 = *reinterpret_cast<const float4*>(&kPreTab.v[i]);
        const float4 r1 = *reinterpret_cast<const float4*>(&kPreTab.v[i + 4]);
        const float ref8[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if ((t & 3) == 0) poll();   // every 4 steps (dynamic priority, rx_kernel kDyn)
            const float ref = ref8[t];
            const float er = qstep(k, w[t & 7], w[(t + 7) & 7], w[(t + 6) & 7], w[(t + 5) & 7],
                                          w[(t + 4) & 7], ref, c, bmax);
            matches += (er * ref > 0.0f) ? 1 : 0;
            w[(t + 4) & 7] = wl[i + t + 4];   // sample of step i+t+4
        }
    }
    // the fast path's premises, as in train(): the divisors inside the
    // reciprocal's range and the state finite (kal_finite's argument holds for
    // the quad layout's real entries, which undergo the same operations; a
    // padding entry can only add an inf or NaN, never hide one).  Lanes 0..2
    // accumulate an unused eq4: it is left out.
    f2 z = k.eqr * 0.0f + k.dd * 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) z = z + k.R[i] * 0.0f;
    if (c == 3) z = z + k.eq4 * 0.0f;
    bad |= bmax > __float_as_uint(0x1p125f) || !(z.x + z.y == 0.0f);
    return matches;
}

// The lanes of `vm` (at most one per quad) each append a job: one slot
// reservation per wave, then lane `mine` stores its job.
__device__ __forceinline__ void quad_push_jobs(float4* jobs, size_t jcap, unsigned* njobs,
                                               unsigned long long vm, bool mine, const DataJob& j,
                                               const f2* x35) {
    unsigned base = 0;
    if (lane_id() == 0) base = atomicAdd(njobs, (unsigned)__popcll(vm));
    base = __builtin_amdgcn_readfirstlane(base);
    if (mine) {
        const unsigned slot = base + (unsigned)__popcll(vm & ((1ull << lane_id()) - 1ull));
        put_job(jobs, jcap, slot, j, x35);
    }
}

// The exact recomputation of a quad wave's frames (a `bad` lane in the wave):
// every lane of a quad runs its channel's lane-per-channel training on the
// same window slots, and valid frames' jobs take that state.  Returns matches.
// Called by the whole wave.  Out of line, job store included, so that the lane
// state (Kal, 50 VGPRs) never meets the quad loop's register allocation; the
// training's priority polls are left out (rare path).
__device__ __attribute__((noinline)) int quad_redo_frame(const float2* win, bool live, bool lead,
                                                         float4* jobs, size_t jcap,
                                                         unsigned* njobs, size_t cf, unsigned ks) {
    const f2* wp2 = reinterpret_cast<const f2*>(win);
    DataJob j;
    j.k = kal_reset();
    f2 x[5];
    load_x0(reinterpret_cast<const float4*>(win), x);
    bool bad = true;
    const int matches = train<true>(j.k, x, wp2, bad, [] {});
    const bool mine = live && lead && matches > QK_MATCH_MIN;
    const unsigned long long vm = __ballot(mine);
    if (vm) {
        j.cf = cf;
        j.ks = ks;
        quad_push_jobs(jobs, jcap, njobs, vm, mine, j, wp2 + 129);
    }
    return matches;
}

// back_frame() for a quad per channel: every lane of the quad has the same
// matches / valid / rt; the quad's lane 0 writes the per-channel outputs.
template <typename RtFn, typename PollFn>
__device__ __forceinline__ void back_frame_quad(const RxArgs& a, int ch, bool live, int n, int mi,
                                                RtFn get_rt, const float2* win, int* rt_next,
                                                PollFn poll) {
    const int c = lane_id() & 3;
    const bool lead = c == 0;
    const f2* wp2 = reinterpret_cast<const f2*>(win);
    QKal k = qkal_reset();
    f2 X[5];
    qload_x0(wp2, c, X);
    bool bad = roles_force_exact(a.roles);
    int matches = qtrain(k, X, wp2 + c + 2, c, bad, poll);
    const size_t cf = (size_t)ch * a.F + n;
    const unsigned ks = (a.g0 + (unsigned)n) % QK_KS_FRAMES;
    // a lane left the fast path's premises: the wave's frames are recomputed
    // exactly, and their jobs stored, out of line (wave-uniform branch)
    const bool redo = __ballot(bad) != 0ull;
    if (__builtin_expect(redo, 0)) {
        poll();   // the priority this frame's training would run at
        matches = quad_redo_frame(win, live, lead, a.jobs, a.jcap, a.njobs, cf, ks);
    }
    const bool valid = live && matches > QK_MATCH_MIN;   // src/qpsk.c:196
    const unsigned long long vm = redo ? 0ull : __ballot(valid && lead);
    if (vm) {   // gather the quad's state (all lanes take part in the DPP moves)
        DataJob j;
        j.k.eq[0] = qd2<qd::kB0>(k.eqr);
        j.k.eq[1] = qd2<qd::kB1>(k.eqr);
        j.k.eq[2] = qd2<qd::kB2>(k.eqr);
        j.k.eq[3] = qd2<qd::kB3>(k.eqr);
        j.k.eq[4] = qd2<qd::kB3>(k.eq4);
#define QU(i, jj, CT) j.k.u[uix(i, jj)] = qd2<CT>(k.R[(jj) - (i) - 1])
        QU(0, 1, qd::kB0); QU(0, 2, qd::kB0); QU(0, 3, qd::kB0); QU(0, 4, qd::kB0);
        QU(1, 2, qd::kB1); QU(1, 3, qd::kB1); QU(1, 4, qd::kB1);
        QU(2, 3, qd::kB2); QU(2, 4, qd::kB2);
        QU(3, 4, qd::kB3);
#undef QU
        j.k.d[0] = f2{k.dd.x, k.dd.x};
        const float d1 = qdf<qd::kB0>(k.dd.y), d2 = qdf<qd::kB1>(k.dd.y);
        const float d3 = qdf<qd::kB2>(k.dd.y), d4 = qdf<qd::kB3>(k.dd.y);
        j.k.d[1] = f2{d1, d1};
        j.k.d[2] = f2{d2, d2};
        j.k.d[3] = f2{d3, d3};
        j.k.d[4] = f2{d4, d4};
        j.cf = cf;
        j.ks = ks;
        quad_push_jobs(a.jobs, a.jcap, a.njobs, vm, valid && lead, j, wp2 + 129);
    }
    if (live && !valid) {   // invalid frame: bits (and soft symbols) are zero
        uint16_t* bo = reinterpret_cast<uint16_t*>(a.bits + cf * QK_NBITS);
        for (int ss = c; ss < QK_NDSYM; ss += 4) bo[ss] = 0;
        if (a.soft) {
            float2* so = a.soft + cf * QK_NDSYM;
            for (int ss = c; ss < QK_NDSYM; ss += 4) so[ss] = make_float2(0.0f, 0.0f);
        }
    }
    const int rt = get_rt();
    const int rtn = valid ? mi + QK_NPRE : rt;    // src/qpsk.c:219
    if (lead) *rt_next = rtn;
    if (live && lead) {
        a.valid[cf] = valid ? 1 : 0;
        if (a.trace)
            *reinterpret_cast<int4*>(a.trace + cf * 4) = make_int4(mi, matches, valid ? 1 : 0, rtn);
    }
}

}  // namespace
