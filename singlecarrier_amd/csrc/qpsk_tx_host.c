/*
 * qpsk_tx_host.c -- qpsk_tx_batch_host (include/qpsk_tx.h): the batched
 * transmitter's contract on the host.  Per channel the packet order of the
 * reference's main() (src/qpsk.c:380-413) over the reentrant transmitter
 * qpsk_tx_frame_state(); pthreads over channels, like qpsk_synth.c.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_consts.h"
#include "qpsk_tx.h"

#define TX_PACKET (QK_CYCLES * (QK_NPRE + 8 * QK_NDSYM))   /* 1880 */
#define PACKET_BITS (8 * QK_NBITS)                          /* 496 */

static void tx_channel(qpsk_tx_state *st, const uint8_t *bits, int npackets, int gap,
                       int16_t *out) {
    float pre[QK_NPRE * 2], dsym[QK_NDSYM * 2];
    for (int i = 0; i < QK_NPRE; i++) pre[2 * i] = pre[2 * i + 1] = (float)QK_PRE[i];
    for (int k = 0; k < npackets; k++) {
        out += qpsk_tx_frame_state(st, out, pre, QK_NPRE, true);
        for (int f = 0; f < 8; f++) {
            const uint8_t *b = bits + (size_t)k * PACKET_BITS + (size_t)f * QK_NBITS;
            for (int i = 0; i < QK_NDSYM; i++) {   /* qpsk_mod, src/qpsk.c:251-256 */
                dsym[2 * i] = (b[2 * i + 1] == 1) ? -1.0f : 1.0f;
                dsym[2 * i + 1] = (b[2 * i] == 1) ? -1.0f : 1.0f;
            }
            out += qpsk_tx_frame_state(st, out, dsym, QK_NDSYM, false);
        }
        memset(out, 0, sizeof(int16_t) * (size_t)gap);   /* not modulated, src/qpsk.c:410-412 */
        out += gap;
    }
}

typedef struct {
    qpsk_tx_state *st;
    const uint8_t *bits;
    int16_t *out;
    long ld;
    int lo, hi, npackets, gap;
} job_t;

static void *worker(void *arg) {
    job_t *j = (job_t *)arg;
    for (int c = j->lo; c < j->hi; c++)
        tx_channel(&j->st[c], j->bits + (size_t)c * j->npackets * PACKET_BITS, j->npackets,
                   j->gap, j->out + (size_t)c * j->ld);
    return NULL;
}

int qpsk_tx_batch_host(qpsk_tx_state *st, int nch, const uint8_t *bits, int npackets, int gap,
                       int16_t *out, long ld, int nthreads) {
    if (!st || nch < 1 || gap < 0 || npackets < 0) return QPSK_EINVAL;
    if (npackets == 0) return QPSK_OK;
    if (!bits || !out || (long)nch * npackets >= (1L << 28) ||
        ld < (long)npackets * (TX_PACKET + (long)gap))
        return QPSK_EINVAL;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > nch) nthreads = nch;
    job_t *jobs = (job_t *)calloc((size_t)nthreads, sizeof(job_t));
    pthread_t *th = (pthread_t *)calloc((size_t)nthreads, sizeof(pthread_t));
    if (!jobs || !th) {
        free(jobs);
        free(th);
        return QPSK_ENOMEM;
    }
    int started = 0, rc = QPSK_OK;
    for (int t = 0; t < nthreads; t++) {
        jobs[t] = (job_t){st, bits, out, ld, (int)((long)nch * t / nthreads),
                          (int)((long)nch * (t + 1) / nthreads), npackets, gap};
        if (t == nthreads - 1 || pthread_create(&th[t], NULL, worker, &jobs[t]) != 0) {
            /* the last share (or any whose thread did not start) runs here */
            for (int u = t; u < nthreads; u++) {
                jobs[u] = (job_t){st, bits, out, ld, (int)((long)nch * u / nthreads),
                                  (int)((long)nch * (u + 1) / nthreads), npackets, gap};
                worker(&jobs[u]);
            }
            break;
        }
        started++;
    }
    for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
    free(jobs);
    free(th);
    return rc;
}
