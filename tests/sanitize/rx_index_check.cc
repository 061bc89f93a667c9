// rx_index_check.cc -- the per-channel frame index arithmetic of
// csrc/qpsk_rx_plan.h on the CPU (tests/test_channel_index.py): a channel's own
// index from the context's and its lead, and the residue the data kernel adds
// to a job's descrambler word (koff).  Built with -fsanitize=address,undefined;
// exits nonzero after printing every check that failed.  The last line is
// "pairs <n>".
#include <stdio.h>

#include "qpsk_rx_plan.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); g_fail++; } } while (0)

int main() {
    const uint64_t at[] = {0, 1056, 1057, 2113, (1ull << 32) - 1, (1ull << 32) + 1, 1ull << 63, ~0ull};
    int pairs = 0;
    for (uint64_t own : at)
        for (uint64_t ctx : at) {
            const unsigned k = rx_koff(own, ctx);
            CHECK(k < (unsigned)QK_KS_FRAMES);
            // own - ctx as an integer, not as a wrapped 64-bit word
            const __int128 d = (__int128)own - (__int128)ctx;
            const int want = (int)(((d % QK_KS_FRAMES) + QK_KS_FRAMES) % QK_KS_FRAMES);
            CHECK((int)k == want);
            // the word a job of context frame ctx + n gets is the channel's own, for
            // the frames of a call (no index passes 2^64 inside one)
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)1056, (uint64_t)4000}) {
                if (own + n < own || ctx + n < ctx) continue;
                unsigned w = (unsigned)((ctx + n) % QK_KS_FRAMES) + k;
                if (w >= (unsigned)QK_KS_FRAMES) w -= (unsigned)QK_KS_FRAMES;
                CHECK(w == (unsigned)((own + n) % QK_KS_FRAMES));
            }
            // the host's record of the channel gives its index back exactly, at
            // once and after both have advanced
            const uint64_t lead = rx_index_lead(own, ctx);
            CHECK(rx_own_index(ctx, lead) == own);
            if (own + 77 > own && ctx + 77 > ctx) CHECK(rx_own_index(ctx + 77, lead) == own + 77);
            CHECK(rx_lead_odd(own, ctx) == (((own & 1) != 0) != ((ctx & 1) != 0)));
            // the wrapped difference is not enough: 2^64 mod 1057 != 0
            if (own < ctx) CHECK((unsigned)(lead % QK_KS_FRAMES) != k);
            pairs++;
        }
    CHECK(rx_koff(0, 0) == 0 && rx_koff(5, 5) == 0 && rx_koff(0, 3) == 1054 && rx_koff(7, 4) == 3);
    CHECK(rx_koff((1ull << 32) + 5, 1055) == 11);   // 2^32 mod 1057 = 4
    printf("pairs %d\n", pairs);
    return g_fail ? 1 : 0;
}
