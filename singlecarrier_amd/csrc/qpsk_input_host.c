/*
 * qpsk_input_host.c -- qpsk_input_bytes and qpsk_input_convert_host
 * (include/qpsk_input.h): the input conversion's contract on the host.  G.711
 * codes through a 256-entry table made from the expansion in qpsk_fmt.h;
 * threads over channels (qpsk_fanout), like qpsk_tx_host.c.  One
 * self-contained source: the sanitizer build of tests/callers takes it alone.
 */
#include <string.h>

#include "qpsk_fanout.h"
#include "qpsk_fmt.h"

size_t qpsk_input_bytes(int fmt, int nch, int nframes, long ld) {
    if (qpsk_input_check(fmt, nch, nframes, ld) != QPSK_OK || nframes == 0) return 0;
    return qpsk_input_elems(fmt, nch, nframes, ld) * (size_t)qpsk_fmt_esize(fmt);
}

typedef struct {
    const uint8_t *src;   /* bytes: 8-bit codes may start at any address, and so may
                             int16 samples as far as this file goes (memcpy) */
    int16_t *out;
    size_t T, cstride, tstride;   /* element (t, c) is src[c * cstride + t * tstride] */
    int enc;
    int16_t tab[256];
} job_t;

/* channels [lo, hi): time in blocks, so an interleaved source's rows are read
 * once per block of channels they are in cache for */
static void share(void *arg, int lo, int hi) {
    const job_t *j = (const job_t *)arg;
    enum { TB = 256 };
    for (size_t t0 = 0; t0 < j->T; t0 += TB) {
        const size_t t1 = t0 + TB < j->T ? t0 + TB : j->T;
        for (int c = lo; c < hi; c++) {
            int16_t *o = j->out + (size_t)c * j->T;
            const size_t base = (size_t)c * j->cstride;
            if (j->enc == QPSK_IN_S16) {
                for (size_t t = t0; t < t1; t++)
                    memcpy(&o[t], j->src + 2 * (base + t * j->tstride), 2);
            } else {
                for (size_t t = t0; t < t1; t++) o[t] = j->tab[j->src[base + t * j->tstride]];
            }
        }
    }
}

int qpsk_input_convert_host(int fmt, const void *src, long ld, int nch, int nframes,
                            int16_t *out, int nthreads) {
    if (qpsk_input_check(fmt, nch, nframes, ld) != QPSK_OK) return QPSK_EINVAL;
    if (nframes == 0) return QPSK_OK;
    if (!src || !out) return QPSK_EINVAL;
    job_t job;
    job.src = (const uint8_t *)src;
    job.out = out;
    job.T = (size_t)nframes * QK_FRAME;
    job.enc = QPSK_FMT_ENC(fmt);
    if (QPSK_FMT_LAYOUT(fmt) == QPSK_IN_INTERLEAVED) {
        job.cstride = 1;
        job.tstride = (size_t)ld;
    } else {
        job.cstride = job.T;
        job.tstride = 1;
    }
    for (unsigned k = 0; k < 256; k++)
        job.tab[k] = (int16_t)(job.enc == QPSK_IN_ALAW ? qpsk_alaw_decode(k) : qpsk_ulaw_decode(k));
    return qpsk_fanout(nch, nthreads, share, &job) == 0 ? QPSK_OK : QPSK_ENOMEM;
}
