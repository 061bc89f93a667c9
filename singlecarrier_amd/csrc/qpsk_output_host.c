/*
 * qpsk_output_host.c -- qpsk_output_bytes and qpsk_output_convert_host
 * (include/qpsk_output.h): the output conversion's contract on the host.  G.711
 * codes by the integer compression of qpsk_fmt.h; threads over channels
 * (qpsk_fanout), like qpsk_input_host.c.  One self-contained source: the
 * sanitizer build of the tests takes it alone.
 */
#include <string.h>

#include "qpsk_fanout.h"
#include "qpsk_fmt.h"

size_t qpsk_output_bytes(int fmt, int nch, long n, long ld) {
    if (qpsk_output_check(fmt, nch, n, n, ld) != QPSK_OK || n == 0) return 0;
    return qpsk_output_elems(fmt, nch, n, ld) * (size_t)qpsk_fmt_esize(fmt);
}

typedef struct {
    const int16_t *src;
    uint8_t *dst;   /* bytes: codes may start at any address, and so may int16
                       samples as far as this file goes (memcpy) */
    size_t n, src_ld, cstride, tstride;   /* element (p, c) is dst[c * cstride + p * tstride] */
    int enc;
} job_t;

/* channels [lo, hi): time in blocks, so an interleaved destination's rows are
 * written once per block of channels they are in cache for */
static void share(void *arg, int lo, int hi) {
    const job_t *j = (const job_t *)arg;
    enum { TB = 256 };
    for (size_t p0 = 0; p0 < j->n; p0 += TB) {
        const size_t p1 = p0 + TB < j->n ? p0 + TB : j->n;
        for (int c = lo; c < hi; c++) {
            const int16_t *s = j->src + (size_t)c * j->src_ld;
            const size_t base = (size_t)c * j->cstride;
            if (j->enc == QPSK_OUT_S16) {
                for (size_t p = p0; p < p1; p++) memcpy(j->dst + 2 * (base + p * j->tstride), &s[p], 2);
            } else if (j->enc == QPSK_OUT_ALAW) {
                for (size_t p = p0; p < p1; p++) j->dst[base + p * j->tstride] = (uint8_t)qpsk_alaw_encode(s[p]);
            } else {
                for (size_t p = p0; p < p1; p++) j->dst[base + p * j->tstride] = (uint8_t)qpsk_ulaw_encode(s[p]);
            }
        }
    }
}

int qpsk_output_convert_host(int fmt, const int16_t *src, long src_ld, int nch, long n, void *dst,
                             long ld, int nthreads) {
    if (qpsk_output_check(fmt, nch, n, src_ld, ld) != QPSK_OK) return QPSK_EINVAL;
    if (n == 0) return QPSK_OK;
    if (!src || !dst) return QPSK_EINVAL;
    job_t job;
    job.src = src;
    job.dst = (uint8_t *)dst;
    job.n = (size_t)n;
    job.src_ld = (size_t)src_ld;
    job.enc = QPSK_FMT_ENC(fmt);
    if (QPSK_FMT_LAYOUT(fmt) == QPSK_OUT_INTERLEAVED) {
        job.cstride = 1;
        job.tstride = (size_t)ld;
    } else {
        job.cstride = (size_t)ld;
        job.tstride = 1;
    }
    return qpsk_fanout(nch, nthreads, share, &job) == 0 ? QPSK_OK : QPSK_ENOMEM;
}
