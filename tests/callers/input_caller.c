/*
 * input_caller.c -- qpsk_input_convert_host (csrc/qpsk_input_host.c) as a
 * stand-alone program, for the AddressSanitizer + UBSan build of
 * tests/test_input_host.py.  Every format over the edge shapes of the tests,
 * with the source in a heap block of exactly qpsk_input_bytes() bytes behind
 * an odd byte offset and the output in one of exactly nch * T int16: a read or
 * a write one element too far is a report.  The result is compared with the
 * expansion of include/qpsk_input.h written out here.
 *
 *   input_caller            exit 0 and "ok <cases>" when every case matched
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_input.h"

static int ulaw(unsigned code) {
    unsigned u = ~code & 0xff;
    int t = (int)((((u & 15) << 3) + 0x84) << ((u >> 4) & 7));
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}

static int alaw(unsigned code) {
    unsigned a = (code ^ 0x55) & 0xff;
    int m = (int)((a & 15) << 4), s = (int)((a >> 4) & 7);
    int v = s == 0 ? m + 8 : s == 1 ? m + 0x108 : (m + 0x108) << (s - 1);
    return (a & 0x80) ? v : -v;
}

static unsigned lcg = 12345;
static unsigned rnd(void) {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg >> 16;
}

static int one(int fmt, int nch, long ld, int nframes, int offset, int nthreads) {
    const int enc = fmt & 0x0f, inter = (fmt & ~0x0f) == QPSK_IN_INTERLEAVED;
    const size_t es = enc == QPSK_IN_S16 ? 2 : 1, T = (size_t)nframes * 1880;
    const size_t bytes = qpsk_input_bytes(fmt, nch, nframes, ld);
    const size_t want = (inter ? (T - 1) * (size_t)ld + (size_t)nch : (size_t)nch * T) * es;
    if (bytes != want) return 1;
    uint8_t *block = malloc(bytes + (size_t)offset);
    int16_t *out = malloc(sizeof(int16_t) * (size_t)nch * T);
    if (!block || !out) return 2;
    uint8_t *src = block + offset;
    for (size_t i = 0; i < bytes; i++) src[i] = (uint8_t)rnd();
    int bad = qpsk_input_convert_host(fmt, src, ld, nch, nframes, out, nthreads) != QPSK_OK;
    for (int c = 0; c < nch && !bad; c++)
        for (size_t t = 0; t < T && !bad; t++) {
            const size_t e = inter ? t * (size_t)ld + (size_t)c : (size_t)c * T + t;
            int v;
            if (enc == QPSK_IN_S16) {
                int16_t x;
                memcpy(&x, src + 2 * e, 2);
                v = x;
            } else {
                v = enc == QPSK_IN_ALAW ? alaw(src[e]) : ulaw(src[e]);
            }
            bad = out[(size_t)c * T + t] != v;
        }
    free(block);
    free(out);
    return bad ? 3 : 0;
}

int main(void) {
    static const int shapes[][2] = {{1, 1}, {3, 7}, {63, 63}, {65, 80}, {130, 131}, {257, 300}};
    static const int encs[] = {QPSK_IN_S16, QPSK_IN_ALAW, QPSK_IN_ULAW};
    int cases = 0;
    for (unsigned s = 0; s < sizeof shapes / sizeof shapes[0]; s++)
        for (int e = 0; e < 3; e++)
            for (int lay = 0; lay <= QPSK_IN_INTERLEAVED; lay += QPSK_IN_INTERLEAVED)
                for (int nf = 1; nf <= 3; nf += 2)
                    for (int off = 0; off <= 3; off += (e == 0 ? 2 : 1)) {
                        const int fmt = encs[e] | lay;
                        const int r = one(fmt, shapes[s][0], shapes[s][1], nf, off, 1 + 3 * (cases & 1));
                        if (r) {
                            fprintf(stderr, "fmt %#x nch %d ld %d frames %d offset %d: %d\n", fmt,
                                    shapes[s][0], shapes[s][1], nf, off, r);
                            return 1;
                        }
                        cases++;
                    }
    /* the refusals touch nothing */
    int16_t o;
    uint8_t b = 0;
    if (qpsk_input_convert_host(3, &b, 1, 1, 1, &o, 1) != QPSK_EINVAL ||
        qpsk_input_convert_host(QPSK_IN_ALAW | QPSK_IN_INTERLEAVED, &b, 2, 3, 1, &o, 1) != QPSK_EINVAL ||
        qpsk_input_convert_host(QPSK_IN_ALAW, NULL, 1, 1, 1, &o, 1) != QPSK_EINVAL ||
        qpsk_input_convert_host(QPSK_IN_ALAW, &b, 1, 1, -1, &o, 1) != QPSK_EINVAL ||
        qpsk_input_convert_host(QPSK_IN_ALAW, &b, 1, 1 << 14, 1 << 14, &o, 1) != QPSK_EINVAL ||
        qpsk_input_convert_host(QPSK_IN_ALAW, NULL, 1, 1, 0, NULL, 1) != QPSK_OK)
        return 2;
    printf("ok %d\n", cases);
    return 0;
}
