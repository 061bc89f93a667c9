/* compact_check.c -- the host twin of the record layer (csrc/
 * qpsk_compact_host.c, include/qpsk_compact.h) under ASan + UBSan
 * (tests/test_compact_host.py).  Every array is a heap block of exactly the
 * size the header states, so a read or write past min(count, cap) rows, past
 * groups[G] or past the dense inputs is a sanitizer report; the results are
 * checked against a restatement that sorts nothing and packs nothing in place:
 * it walks the order and compares field by field. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_compact.h"

static uint32_t lcg = 2463534242u;
static uint32_t rnd(void) {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg >> 8;
}

static int fails = 0;
#define EXPECT(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

/* density: per mille of valid frames */
static void one_case(int nch, int nf, int order, int density, int cap_delta) {
    const size_t n = (size_t)nch * (size_t)nf;
    uint8_t *bits = malloc(n * 62 + 1), *valid = malloc(n + 1);
    int32_t *trace = malloc(n * 16 + 1);
    float *soft = malloc(n * 248 + 1);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        valid[i] = (uint8_t)((int)(rnd() % 1000u) < density ? 1 + rnd() % 3u : 0);
        total += valid[i] != 0;
        for (int b = 0; b < 62; b++) {
            const uint32_t r = rnd() % 16u;
            bits[i * 62 + b] = (uint8_t)(r < 7 ? 0 : r < 14 ? 1 : r == 14 ? 2 : 255);
        }
        for (int k = 0; k < 4; k++) trace[i * 4 + k] = (int32_t)rnd();
        for (int k = 0; k < 62; k++) soft[i * 62 + k] = (float)(int)(rnd() % 4096u) - 2048.0f;
    }
    long capl = (long)total + cap_delta;
    if (cap_delta == -1000000) capl = 0;
    if (capl < 0) capl = 0;
    const size_t cap = (size_t)capl, rows = cap < total ? cap : total;
    const int G = order == QPSK_REC_BY_FRAME ? nf : nch;
    /* exactly `rows` rows: one more written row is a heap overflow */
    qpsk_frame_rec *rec = malloc(rows * sizeof *rec + 1);
    int32_t *rtr = malloc(rows * 16 + 1);
    float *rso = malloc(rows * 248 + 1);
    uint32_t *groups = malloc(((size_t)G + 1) * 4), count = 0xdeadbeefu;
    const int r = qpsk_compact_host(bits, valid, trace, soft, nch, nf, order, cap, cap ? rec : NULL, rtr, rso,
                                    groups, &count);
    EXPECT(r == QPSK_OK);
    EXPECT(count == total);
    EXPECT(groups[G] == count);
    size_t rank = 0;
    const int outer = order == QPSK_REC_BY_FRAME ? nf : nch, inner = order == QPSK_REC_BY_FRAME ? nch : nf;
    for (int g = 0; g < outer; g++) {
        EXPECT(groups[g] == rank);
        for (int k = 0; k < inner; k++) {
            const int c = order == QPSK_REC_BY_FRAME ? k : g, f = order == QPSK_REC_BY_FRAME ? g : k;
            const size_t src = (size_t)c * nf + f;
            if (!valid[src]) continue;
            if (rank < rows) {
                EXPECT(rec[rank].channel == (uint32_t)c && rec[rank].frame == (uint32_t)f);
                for (int b = 0; b < 64; b++)
                    EXPECT(((rec[rank].bits >> b) & 1u) == (uint64_t)(b < 62 && bits[src * 62 + b] == 1));
                EXPECT(memcmp(rtr + rank * 4, trace + src * 4, 16) == 0);
                EXPECT(memcmp(rso + rank * 62, soft + src * 62, 248) == 0);
            }
            rank++;
        }
    }
    /* the same without the optional outputs, and as a pure count */
    uint32_t count2 = 0;
    EXPECT(qpsk_compact_host(bits, valid, NULL, NULL, nch, nf, order, cap, cap ? rec : NULL, NULL, NULL, NULL,
                             &count2) == QPSK_OK && count2 == total);
    count2 = 0;
    EXPECT(qpsk_compact_host(bits, valid, trace, soft, nch, nf, order, 0, NULL, NULL, NULL, NULL, &count2) == QPSK_OK &&
           count2 == total);
    /* the dense packers on the same rows */
    uint64_t *words = malloc(n * 8 + 1);
    uint8_t *back = malloc(n * 62 + 1);
    EXPECT(qpsk_bits_pack_host(bits, n, words) == QPSK_OK);
    EXPECT(qpsk_bits_unpack_host(words, n, back) == QPSK_OK);
    for (size_t i = 0; i < n * 62; i++) EXPECT(back[i] == (bits[i] == 1));
    free(words), free(back);
    free(bits), free(valid), free(trace), free(soft), free(rec), free(rtr), free(rso), free(groups);
}

int main(void) {
    static const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {5, 7}, {64, 3}, {33, 65}, {0, 4}, {4, 0}};
    static const int dens[] = {0, 1000, 200, 30};
    static const int caps[] = {-1000000, -1, 0, 5};
    int ncases = 0;
    for (size_t s = 0; s < sizeof shapes / sizeof shapes[0]; s++)
        for (int order = 0; order < 2; order++)
            for (size_t d = 0; d < 4; d++)
                for (size_t c = 0; c < 4; c++, ncases++) one_case(shapes[s][0], shapes[s][1], order, dens[d], caps[c]);
    /* refusals touch nothing */
    uint32_t count = 7;
    uint8_t b[62] = {0}, v[1] = {1};
    qpsk_frame_rec rec;
    EXPECT(qpsk_compact_host(b, v, NULL, NULL, 1, 1, 2, 1, &rec, NULL, NULL, NULL, &count) == QPSK_EINVAL);
    EXPECT(qpsk_compact_host(b, v, NULL, NULL, -1, 1, 0, 1, &rec, NULL, NULL, NULL, &count) == QPSK_EINVAL);
    EXPECT(qpsk_compact_host(b, v, NULL, NULL, 1, 1, 0, 1, NULL, NULL, NULL, NULL, &count) == QPSK_EINVAL);
    EXPECT(qpsk_compact_host(b, v, NULL, NULL, 1 << 14, 1 << 14, 0, 0, NULL, NULL, NULL, NULL, &count) == QPSK_EINVAL);
    EXPECT(count == 7);
    printf("compact_check: %d cases, %d failures\n", ncases, fails);
    return fails != 0;
}
