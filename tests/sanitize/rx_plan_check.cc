// rx_plan_check.cc -- csrc/qpsk_rx_plan.h on the CPU (tests/test_rx_plan.py):
// the kernel shape per batch size and forced knob, the staging layout, and the
// snapshot size.  Built with -fsanitize=address,undefined; exits nonzero after
// printing every check that failed.  The last lines are "state_size <n> <bytes>".
#include <stdio.h>

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

int main() {
    shapes();
    stages();
    for (int n : {0, -3, 1, 96, 65536}) printf("state_size %d %zu\n", n, rx_state_size(n));
    return g_fail ? 1 : 0;
}
