// rx_plan_check.cc -- csrc/qpsk_rx_plan.h on the CPU (tests/test_rx_plan.py):
// the kernel shape per batch size and forced knob, the staging layout, the
// pointer alignment rule and the snapshot size.  Built with
// -fsanitize=address,undefined; exits nonzero after printing every check that
// failed.  Prints "limits <kZeroCopyCF> <largest pinned cf>", then the last
// lines are "state_size <n> <bytes>".
#include <stdio.h>
#include <stdlib.h>

#include "qpsk_rx_plan.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); g_fail++; } } while (0)

static void shapes() {
    const int ncu = 256;
    const RxKnobs def;
    struct { int nch, kind; } by_size[] = {
        {1, Shape::k1x8q16},     {4096, Shape::k1x8q16},  {4097, Shape::k1x8q32},  {8192, Shape::k1x8q32},
        {8193, Shape::k1x8d64},  {16384, Shape::k1x8d64}, {16385, Shape::k2x4d},   {32768, Shape::k2x4d},
        {32769, Shape::k4x2},    {65536, Shape::k4x2}};
    for (const auto& e : by_size) {
        const Shape sh = pick_shape(def, e.nch, ncu);
        CHECK(sh.kind == e.kind);
        if (e.kind == Shape::k1x8d64) {
            CHECK(roles_prio(sh.roles) == kPrioBack);
            CHECK(roles_split(sh.roles) == 2);
        } else {   // the default word, untouched
            CHECK(sh.roles == def.roles);
            CHECK(roles_prio(sh.roles) == kPrioFront && roles_split(sh.roles) == 0);
        }
        CHECK(roles_back(sh.roles) && roles_front(sh.roles));
    }
    // a forced shape wins over the batch size
    for (int nch : {1, 4096, 20000, 65536}) {
        RxKnobs k;
        k.shape = Shape::k4x2;
        CHECK(pick_shape(k, nch, ncu).kind == Shape::k4x2);
        k.shape = Shape::k2x4d;
        CHECK(pick_shape(k, nch, ncu).kind == Shape::k2x4d);
    }
    {   // forced into the 1x8 family, the width still goes by the batch size
        RxKnobs k;
        k.shape = Shape::k1x8d64;
        CHECK(pick_shape(k, 65536, ncu).kind == Shape::k1x8d64);
        CHECK(pick_shape(k, 100, ncu).kind == Shape::k1x8q16);
        CHECK(pick_shape(k, 5000, ncu).kind == Shape::k1x8q32);
    }
    // a forced width acts only inside the 1x8 family
    const int kind_of_width[][2] = {{16, Shape::k1x8q16}, {32, Shape::k1x8q32}, {64, Shape::k1x8d64}};
    for (const auto& w : kind_of_width) {
        RxKnobs k;
        k.width = w[0];
        for (int nch : {1, 4096, 8192, 16384}) {
            const Shape sh = pick_shape(k, nch, ncu);
            CHECK(sh.kind == w[1]);
            CHECK((roles_split(sh.roles) == 2) == (w[0] == 64));
        }
        CHECK(pick_shape(k, 16385, ncu).kind == Shape::k2x4d);
        CHECK(pick_shape(k, 65536, ncu).kind == Shape::k4x2);
        CHECK(pick_shape(k, 65536, ncu).roles == def.roles);
        k.shape = Shape::k4x2;
        CHECK(pick_shape(k, 100, ncu).kind == Shape::k4x2);
    }
    // a forced priority is applied last: over the default and over the lane backs'
    for (int prio : {(int)kPrioNone, (int)kPrioFront, (int)kPrioBack}) {
        RxKnobs k;
        k.prio = prio;
        for (int nch : {100, 5000, 10000, 20000, 65536}) {
            const Shape sh = pick_shape(k, nch, ncu), plain = pick_shape(def, nch, ncu);
            CHECK(sh.kind == plain.kind);
            CHECK(roles_prio(sh.roles) == prio);
            CHECK(sh.roles == roles_with_prio(plain.roles, prio));
        }
    }
}

static void stages() {
    for (size_t cf : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)96 * 2}) {
        const Stage g = stage_of(cf);
        const size_t nin = sizeof(int16_t) * cf * QK_FRAME, nbits = cf * QK_NBITS, nvalid = cf;
        const size_t ntr = sizeof(int32_t) * cf * 4, nso = sizeof(float) * cf * QK_NDSYM * 2;
        // every section but valid and err starts on a 256-byte boundary
        for (size_t o : {g.in, g.bits, g.trace, g.soft, g.end}) CHECK(o % 256 == 0);
        CHECK(g.valid == g.bits + nbits);   // valid follows bits directly
        CHECK(g.err % 4 == 0 && g.err >= g.valid + nvalid && g.err - (g.valid + nvalid) <= 3);
        // [bits, err + 4) is one span, nothing else inside it
        CHECK(g.bits < g.valid && g.valid < g.err && g.err + sizeof(int) <= g.trace);
        // no section overlaps the next
        CHECK(g.in == 0 && g.in + nin <= g.bits);
        CHECK(g.trace + ntr <= g.soft);
        CHECK(g.soft + nso <= g.end);
        // the typed view yields exactly these offsets
        char* const base = reinterpret_cast<char*>(4096);
        const StageView v{base, g};
        CHECK(reinterpret_cast<char*>(v.in()) == base + g.in);
        CHECK(reinterpret_cast<char*>(v.bits()) == base + g.bits);
        CHECK(reinterpret_cast<char*>(v.valid()) == base + g.valid);
        CHECK(reinterpret_cast<char*>(v.err()) == base + g.err);
        CHECK(reinterpret_cast<char*>(v.trace()) == base + g.trace);
        CHECK(reinterpret_cast<char*>(v.soft()) == base + g.soft);
    }
    CHECK(kZeroCopyCF == 64 && stage_of(kZeroCopyCF).bits <= kPinnedStage);
}

// the largest cf whose staging block is pinned (Staging::grow, rx_batch_host)
static size_t pinned_limit() {
    size_t cf = kPinnedStage / (sizeof(int16_t) * QK_FRAME);
    while (stage_of(cf + 1).bits <= kPinnedStage) cf++;
    while (stage_of(cf).bits > kPinnedStage) cf--;
    return cf;
}

// rx_ptrs_aligned: every pointer at every byte offset of a 16-byte line, the
// others on the line; NULL for each optional pointer; and the views of a
// staging block, at any 16-byte aligned base, always pass.  Addresses are
// computed as integers and cast once (no arithmetic on pointers that point
// to no object); the views of the small blocks are taken of a real block.
static const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

static void pointers() {
    const uintptr_t L = (uintptr_t)0x7f0000001000ull;
    const void* const line = at(L);
    CHECK(kAlignIn == 16 && kAlignTrace == 16 && kAlignSoft == 8 && kAlignBits == 2);
    for (uintptr_t o = 0; o < 16; o++) {
        const void* const p = at(L + o);
        CHECK(rx_ptrs_aligned(p, line, line, line, line) == (o % 16 == 0));      // in
        CHECK(rx_ptrs_aligned(line, p, line, line, line) == (o % 2 == 0));       // bits
        CHECK(rx_ptrs_aligned(line, line, p, line, line));                       // valid: any
        CHECK(rx_ptrs_aligned(line, line, line, p, line) == (o % 16 == 0));      // trace
        CHECK(rx_ptrs_aligned(line, line, line, line, p) == (o % 8 == 0));       // soft
        // absent optional outputs change nothing for the others
        CHECK(rx_ptrs_aligned(line, p, line, nullptr, nullptr) == (o % 2 == 0));
        CHECK(rx_ptrs_aligned(line, line, line, nullptr, p) == (o % 8 == 0));
        CHECK(rx_ptrs_aligned(line, line, line, p, nullptr) == (o % 16 == 0));
        CHECK(rx_ptrs_aligned(nullptr, line, p, nullptr, nullptr));
    }
    CHECK(rx_ptrs_aligned(nullptr, nullptr, nullptr, nullptr, nullptr));
    // the minimum legal placement of each array past a 16-byte line, together
    CHECK(rx_ptrs_aligned(line, at(L + 2), at(L + 1), at(L + 16), at(L + 8)));
    // a channel's row of aligned arrays stays aligned (62, 16, 248, 3760-byte rows)
    for (uintptr_t cf : {(uintptr_t)1, (uintptr_t)3, (uintptr_t)1000001})
        CHECK(rx_ptrs_aligned(at(L + cf * sizeof(int16_t) * QK_FRAME), at(L + 2 + cf * QK_NBITS), at(L + 1 + cf),
                              at(L + cf * 16), at(L + 8 + cf * sizeof(float) * 2 * QK_NDSYM)));
    // the sections of a block at any 16-byte aligned base (StageView's pointers
    // are base + offset: stages() above)
    auto sections_ok = [&](size_t cf) {
        const Stage g = stage_of(cf);
        for (uintptr_t B : {L, L + 256, L + 16}) {
            CHECK(rx_ptrs_aligned(at(B + g.in), at(B + g.bits), at(B + g.valid), at(B + g.trace), at(B + g.soft)));
            CHECK(rx_ptrs_aligned(at(B + g.in), at(B + g.bits), at(B + g.valid), nullptr, at(B + g.soft)));
            CHECK((B + g.err) % sizeof(int) == 0);
        }
        CHECK(g.in % kAlignIn == 0 && g.bits % kAlignBits == 0 && g.trace % kAlignTrace == 0 &&
              g.soft % kAlignSoft == 0);
    };
    // the views themselves, of a real block as hipMalloc aligns it
    char* const block = static_cast<char*>(aligned_alloc(256, stage_of(70).end));
    CHECK(block != nullptr);
    for (size_t cf = 1; cf <= 70; cf++) {
        sections_ok(cf);
        if (!block) continue;
        const StageView v{block, stage_of(cf)};
        CHECK(rx_ptrs_aligned(v.in(), v.bits(), v.valid(), v.trace(), v.soft()));
        CHECK(rx_ptrs_aligned(v.in(), v.bits(), v.valid(), nullptr, nullptr));
    }
    free(block);
    const size_t lim = pinned_limit();
    CHECK(stage_of(lim).bits <= kPinnedStage && stage_of(lim + 1).bits > kPinnedStage);
    for (size_t cf : {lim - 1, lim, lim + 1, (size_t)65536 * 32}) sections_ok(cf);
    printf("limits %zu %zu\n", (size_t)kZeroCopyCF, lim);
}

int main() {
    shapes();
    stages();
    pointers();
    for (int n : {0, -3, 1, 96, 65536}) printf("state_size %d %zu\n", n, rx_state_size(n));
    return g_fail ? 1 : 0;
}
