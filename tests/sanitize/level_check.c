/* level_check.c -- the host twin of the level meter and the squelch (csrc/
 * qpsk_level_host.c, include/qpsk_level.h) under ASan + UBSan
 * (tests/test_level_host.py).  Every array is a heap block of exactly the size
 * the header states, so a read or write past it is a sanitizer report.  The
 * inputs and what the calls made of them go to two files in argv[1], which the
 * test reads back and compares with the unsanitized library on the same
 * inputs; the values the header states outright are checked here too. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_level.h"

#define N 1880

static uint32_t lcg = 2463534242u;
static uint32_t rnd(void) {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg >> 8;
}

static int fails = 0;
#define EXPECT(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

static void put(FILE *f, const void *p, size_t n) {
    if (n && fwrite(p, 1, n, f) != n) {
        perror("fwrite");
        exit(2);
    }
}

/* a copy in a block of exactly n bytes (n == 0: one byte that nobody may touch) */
static void *exact(const void *src, size_t n) {
    void *p = malloc(n ? n : 1);
    if (src && n) memcpy(p, src, n);
    return p;
}

static void meter(FILE *f) {
    static const int at[6] = {0, 7, 8, 1871, 1872, 1879};
    static const int16_t val[6] = {-32768, 32767, -1, 1, 12345, -32767};
    enum { ROWS = 3 + 6 + 8 };
    int16_t *x = malloc(sizeof(int16_t) * ROWS * N);
    for (int i = 0; i < N; i++) {
        x[0 * N + i] = -32768;
        x[1 * N + i] = 32767;
        x[2 * N + i] = (int16_t)(i % 2 ? -32767 : 32767);
    }
    memset(x + 3 * N, 0, sizeof(int16_t) * 6 * N);
    for (int k = 0; k < 6; k++) x[(3 + k) * N + at[k]] = val[k];
    for (int i = 9 * N; i < ROWS * N; i++) x[i] = (int16_t)(rnd() & 0xffff);
    qpsk_frame_level *out = malloc(sizeof *out * ROWS);
    EXPECT(qpsk_level_host(x, ROWS, out) == QPSK_OK);
    EXPECT(out[0].sumsq == (1880ull << 30) && out[0].sum == -61603840 && out[0].peak == 32768 && out[0].clipped == N);
    EXPECT(out[1].sumsq == 1880ull * 32767 * 32767 && out[1].sum == 61601960 && out[1].peak == 32767 &&
           out[1].clipped == N);
    EXPECT(out[2].sumsq == 1880ull * 32767 * 32767 && out[2].sum == 0 && out[2].peak == 32767 && out[2].clipped == N / 2);
    for (int k = 0; k < 6; k++) {
        const int v = val[k], a = v < 0 ? -v : v;
        EXPECT(out[3 + k].sumsq == (uint64_t)a * (uint64_t)a && out[3 + k].sum == v && out[3 + k].peak == a &&
               out[3 + k].clipped == (v == 32767 || v == -32768));
    }
    /* one row in a block of its own, no rows, and the refusals */
    int16_t *one = exact(x + 9 * N, sizeof(int16_t) * N);
    qpsk_frame_level *o1 = malloc(sizeof *o1);
    EXPECT(qpsk_level_host(one, 1, o1) == QPSK_OK && memcmp(o1, out + 9, sizeof *o1) == 0);
    EXPECT(qpsk_level_host(NULL, 0, NULL) == QPSK_OK);
    EXPECT(qpsk_level_host(NULL, 1, o1) == QPSK_EINVAL && qpsk_level_host(one, 1, NULL) == QPSK_EINVAL);
    EXPECT(qpsk_level_host(one, (size_t)1 << 28, o1) == QPSK_EINVAL);
    /* the dB helpers */
    EXPECT(qpsk_level_dbfs(out) == 0.0 && qpsk_level_sumsq_of_dbfs(0.0) == (1880ull << 30));
    EXPECT(qpsk_level_dbfs(out + 5) < 0 && isinf(qpsk_level_dbfs(out + 5)) == 0);
    memset(o1, 0, sizeof *o1);
    EXPECT(isinf(qpsk_level_dbfs(o1)) && qpsk_level_dbfs(o1) < 0 && qpsk_level_sumsq_of_dbfs(-INFINITY) == 0);
    EXPECT(qpsk_level_sumsq_of_dbfs(3.0) == (1880ull << 30) && qpsk_level_sumsq_of_dbfs(-400.0) == 1);
    for (int k = 0; k < ROWS; k++) EXPECT(qpsk_level_sumsq_of_dbfs(qpsk_level_dbfs(out + k)) == out[k].sumsq);
    const int32_t rows = ROWS;
    put(f, &rows, 4);
    put(f, x, sizeof(int16_t) * ROWS * N);
    put(f, out, sizeof *out * ROWS);
    free(x), free(out), free(one), free(o1);
}

/* alias: 1 = valid_out is valid_in, 2 = last is prev, 4 = no bits / soft / last */
static void squelch(FILE *f, int nch, int nf, int hasprev, uint64_t min_sumsq, int alias) {
    static const uint64_t lv[6] = {0, 1, 999999999ull, 1000000000ull, 1000000001ull, 1880ull << 30};
    const size_t n = (size_t)nch * (size_t)nf;
    if (alias & 2) hasprev = 1;   /* last is prev: there is one */
    qpsk_frame_level *level = malloc(n ? n * sizeof *level : 1), *prev = malloc(nch ? nch * sizeof *prev : 1);
    uint8_t *vin = malloc(n ? n : 1), *bits = malloc(n ? n * 62 : 1);
    float *soft = malloc(n ? n * 248 : 1);
    for (size_t i = 0; i < n; i++) {
        level[i].sumsq = lv[rnd() % 6u];
        level[i].sum = (int32_t)(rnd() % 2001u) - 1000;
        level[i].peak = (uint16_t)(rnd() % 32769u);
        level[i].clipped = (uint16_t)(rnd() % 1881u);
        vin[i] = (uint8_t)(rnd() % 4u);
        for (int b = 0; b < 62; b++) bits[i * 62 + b] = (uint8_t)(1 + rnd() % 255u);
        for (int b = 0; b < 62; b++) soft[i * 62 + b] = (float)(1 + rnd() % 999u);
    }
    for (int c = 0; c < nch; c++) {
        prev[c].sumsq = lv[rnd() % 6u];
        prev[c].sum = (int32_t)(rnd() % 2001u) - 1000;
        prev[c].peak = (uint16_t)(rnd() % 32769u);
        prev[c].clipped = (uint16_t)(rnd() % 1881u);
    }
    const int32_t head[5] = {nch, nf, hasprev, alias, 0};
    put(f, head, sizeof head);
    put(f, &min_sumsq, 8);
    put(f, level, n * sizeof *level);
    put(f, prev, (size_t)nch * sizeof *prev);
    put(f, vin, n);
    put(f, bits, n * 62);
    put(f, soft, n * 248);
    uint8_t *vout = (alias & 1) ? vin : exact(NULL, n);
    qpsk_frame_level *last = (alias & 2) ? prev : exact(NULL, (size_t)nch * sizeof *last);
    if (!(alias & 1)) memset(vout, 0xA5, n);
    if (!(alias & 2)) memset(last, 0xA5, (size_t)nch * sizeof *last);
    const int bare = (alias & 4) != 0;
    EXPECT(qpsk_squelch_host(level, hasprev ? prev : NULL, nch, nf, min_sumsq, vin, vout,
                             bare ? NULL : bits, bare ? NULL : soft, bare ? NULL : last) == QPSK_OK);
    put(f, vout, n);
    put(f, bits, n * 62);
    put(f, soft, n * 248);
    put(f, last, (size_t)nch * sizeof *last);
    if (!(alias & 1)) free(vout);
    if (!(alias & 2)) free(last);
    free(level), free(prev), free(vin), free(bits), free(soft);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    char path[4096];
    snprintf(path, sizeof path, "%s/level.bin", argv[1]);
    FILE *f = fopen(path, "wb");
    if (!f) return 2;
    meter(f);
    fclose(f);
    snprintf(path, sizeof path, "%s/squelch.bin", argv[1]);
    f = fopen(path, "wb");
    if (!f) return 2;
    static const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {5, 7}, {33, 12}, {0, 4}, {4, 0}};
    int ncases = 0;
    for (size_t s = 0; s < sizeof shapes / sizeof shapes[0]; s++)
        for (int hasprev = 0; hasprev < 2; hasprev++)
            for (int m = 0; m < 3; m++)
                for (int alias = 0; alias < 5; alias++, ncases++)
                    squelch(f, shapes[s][0], shapes[s][1], hasprev, m == 0 ? 0 : m == 1 ? 1000000000ull : 1880ull << 30,
                            alias);
    fclose(f);
    /* refusals touch nothing */
    uint8_t v[1] = {1}, vo[1] = {7};
    qpsk_frame_level l[1];
    memset(l, 0, sizeof l);
    EXPECT(qpsk_squelch_host(l, NULL, -1, 1, 0, v, vo, NULL, NULL, NULL) == QPSK_EINVAL);
    EXPECT(qpsk_squelch_host(l, NULL, 1, -1, 0, v, vo, NULL, NULL, NULL) == QPSK_EINVAL);
    EXPECT(qpsk_squelch_host(NULL, NULL, 1, 1, 0, v, vo, NULL, NULL, NULL) == QPSK_EINVAL);
    EXPECT(qpsk_squelch_host(l, NULL, 1, 1, 0, NULL, vo, NULL, NULL, NULL) == QPSK_EINVAL);
    EXPECT(qpsk_squelch_host(l, NULL, 1, 1, 0, v, NULL, NULL, NULL, NULL) == QPSK_EINVAL);
    EXPECT(qpsk_squelch_host(l, NULL, 1 << 14, 1 << 14, 0, v, vo, NULL, NULL, NULL) == QPSK_EINVAL);
    EXPECT(vo[0] == 7);
    printf("level_check: %d squelch cases, %d failures\n", ncases, fails);
    return fails != 0;
}
