/*
 * output_caller.c -- qpsk_output_convert_host (csrc/qpsk_output_host.c) as a
 * stand-alone program, for the AddressSanitizer + UBSan build of
 * tests/test_output_host.py.  Every format over the edge shapes of the tests,
 * with the source in a heap block of exactly (nch - 1) * src_ld + n int16 and
 * the destination in one of exactly qpsk_output_bytes() bytes behind an odd
 * byte offset: a read or a write one element too far is a report.  The result
 * is compared with the compression of include/qpsk_output.h written out here,
 * and the block's own gaps (row tails, foreign columns) must keep their
 * sentinel.
 *
 *   output_caller            exit 0 and "ok <cases>" when every case matched
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_output.h"

static int msb(unsigned v) {
    int i = 0;
    while (v >>= 1) i++;
    return i;
}

static unsigned ulaw(int x) {
    unsigned m = (unsigned)(x < 0 ? ~x : x) >> 2;
    unsigned a = m + 33 < 0x1FFF ? m + 33 : 0x1FFF;
    int s = msb(a) - 4;
    unsigned code = ((unsigned)(8 - s) << 4) | (15 - ((a >> s) & 15));
    return x >= 0 ? code | 0x80 : code;
}

static unsigned alaw(int x) {
    unsigned m = (unsigned)(x < 0 ? ~x : x) >> 4, v = m;
    if (m >= 16) {
        int e = msb(m) - 3;
        v = (m >> (e - 1)) - 16 + ((unsigned)e << 4);
    }
    if (x >= 0) v |= 0x80;
    return v ^ 0x55;
}

static unsigned lcg = 12345;
static unsigned rnd(void) {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg >> 16;
}

#define SENTINEL 0xC3

static int one(int fmt, int nch, long n, long src_pad, long pad, int offset, int nthreads) {
    const int enc = fmt & 0x0f, inter = (fmt & ~0x0f) == QPSK_OUT_INTERLEAVED;
    const size_t es = enc == QPSK_OUT_S16 ? 2 : 1;
    const long src_ld = n + src_pad, ld = (inter ? nch : n) + pad;
    const size_t bytes = qpsk_output_bytes(fmt, nch, n, ld);
    const size_t want = (inter ? (size_t)(n - 1) * (size_t)ld + (size_t)nch
                               : (size_t)(nch - 1) * (size_t)ld + (size_t)n) * es;
    if (bytes != want) return 1;
    const size_t nsrc = (size_t)(nch - 1) * (size_t)src_ld + (size_t)n;
    int16_t *src = malloc(sizeof(int16_t) * nsrc);
    uint8_t *block = malloc(bytes + (size_t)offset);
    if (!src || !block) return 2;
    for (size_t i = 0; i < nsrc; i++) src[i] = (int16_t)rnd();
    src[0] = -32768;
    src[nsrc - 1] = 32767;
    uint8_t *dst = block + offset;
    memset(dst, SENTINEL, bytes);
    int bad = qpsk_output_convert_host(fmt, src, src_ld, nch, n, dst, ld, nthreads) != QPSK_OK;
    /* every element of the block, and every byte of it that is no element */
    const size_t rows = inter ? (size_t)n : (size_t)nch, cols = inter ? (size_t)nch : (size_t)n;
    for (size_t r = 0; r < rows && !bad; r++) {
        for (size_t k = 0; k < cols && !bad; k++) {
            const int x = inter ? src[k * (size_t)src_ld + r] : src[r * (size_t)src_ld + k];
            const uint8_t *p = dst + (r * (size_t)ld + k) * es;
            if (enc == QPSK_OUT_S16) {
                int16_t v;
                memcpy(&v, p, 2);
                bad = v != x;
            } else {
                bad = *p != (enc == QPSK_OUT_ALAW ? alaw(x) : ulaw(x));
            }
        }
        if (r + 1 < rows)
            for (size_t b = cols * es; b < (size_t)ld * es && !bad; b++) bad = dst[r * (size_t)ld * es + b] != SENTINEL;
    }
    free(src);
    free(block);
    return bad ? 3 : 0;
}

int main(void) {
    static const int nchs[] = {1, 63, 64, 65, 130};
    static const long ns[] = {1, 127, 128, 129, 2783};
    static const int encs[] = {QPSK_OUT_S16, QPSK_OUT_ALAW, QPSK_OUT_ULAW};
    static const long pads[] = {0, 1, 3};
    int cases = 0;
    for (unsigned a = 0; a < 5; a++)
        for (unsigned b = 0; b < 5; b++)
            for (int e = 0; e < 3; e++)
                for (int lay = 0; lay <= QPSK_OUT_INTERLEAVED; lay += QPSK_OUT_INTERLEAVED)
                    for (unsigned p = 0; p < 3; p++) {
                        const int fmt = encs[e] | lay, off = e == 0 ? 2 * (cases & 1) : cases % 4;
                        const int r = one(fmt, nchs[a], ns[b], pads[(p + 1) % 3], pads[p], off, 1 + 2 * (cases & 1));
                        if (r) {
                            fprintf(stderr, "fmt %#x nch %d n %ld pad %ld offset %d: %d\n", fmt, nchs[a], ns[b],
                                    pads[p], off, r);
                            return 1;
                        }
                        cases++;
                    }
    /* the refusals touch nothing */
    int16_t s = 0;
    uint8_t d = SENTINEL;
    const int A = QPSK_OUT_ALAW, AI = QPSK_OUT_ALAW | QPSK_OUT_INTERLEAVED;
    if (qpsk_output_convert_host(3, &s, 1, 1, 1, &d, 1, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(AI, &s, 1, 3, 1, &d, 2, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(A, &s, 2, 1, 2, &d, 1, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(A, &s, 1, 1, 2, &d, 2, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(A, NULL, 1, 1, 1, &d, 1, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(A, &s, 1, 1, 1, NULL, 1, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(A, &s, 1, 0, 1, &d, 1, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(A, &s, 1, 1, -1, &d, 1, 1) != QPSK_EINVAL ||
        qpsk_output_convert_host(A, NULL, 0, 1, 0, NULL, 0, 1) != QPSK_OK || d != SENTINEL)
        return 2;
    printf("ok %d\n", cases);
    return 0;
}
