/*
 * qpsk_tx_host.c -- qpsk_tx_batch_host and qpsk_tx_batch_masked_host
 * (include/qpsk_tx.h): the batched transmitter's contract on the host.  Per
 * channel the packet order of the reference's main() (src/qpsk.c:380-413) over
 * the reentrant transmitter qpsk_tx_frame_state(); threads over channels
 * (qpsk_fanout), like qpsk_synth.c.  An idle slot writes zeros and leaves the
 * channel's state alone, so the state a channel carries is that of a fresh
 * reference transmitter fed its active packets only.
 */
#include <string.h>

#include "qpsk_consts.h"
#include "qpsk_fanout.h"
#include "qpsk_tx.h"

#define TX_PACKET (QK_CYCLES * (QK_NPRE + 8 * QK_NDSYM))   /* 1880 */
#define PACKET_BITS (8 * QK_NBITS)                          /* 496 */

static void tx_channel(qpsk_tx_state *st, const uint8_t *bits, const uint8_t *active, int npackets,
                       int gap, int16_t *out) {
    float pre[QK_NPRE * 2], dsym[QK_NDSYM * 2];
    for (int i = 0; i < QK_NPRE; i++) pre[2 * i] = pre[2 * i + 1] = (float)QK_PRE[i];
    for (int k = 0; k < npackets; k++) {
        if (active && !active[k]) {   /* idle slot: the payload is not read */
            memset(out, 0, sizeof(int16_t) * (size_t)(TX_PACKET + gap));
            out += TX_PACKET + gap;
            continue;
        }
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
    const uint8_t *bits, *active;
    int16_t *out;
    long ld;
    int npackets, gap;
} job_t;

static void share(void *arg, int lo, int hi) {
    const job_t *j = (const job_t *)arg;
    for (int c = lo; c < hi; c++)
        tx_channel(&j->st[c], j->bits + (size_t)c * j->npackets * PACKET_BITS,
                   j->active ? j->active + (size_t)c * j->npackets : NULL, j->npackets, j->gap,
                   j->out + (size_t)c * j->ld);
}

int qpsk_tx_batch_masked_host(qpsk_tx_state *st, int nch, const uint8_t *bits, const uint8_t *active,
                              int npackets, int gap, int16_t *out, long ld, int nthreads) {
    if (!st || nch < 1 || gap < 0 || npackets < 0) return QPSK_EINVAL;
    if (npackets == 0) return QPSK_OK;
    if (!bits || !out || (long)nch * npackets >= (1L << 28) ||
        ld < (long)npackets * (TX_PACKET + (long)gap))
        return QPSK_EINVAL;
    job_t job = {st, bits, active, out, ld, npackets, gap};
    return qpsk_fanout(nch, nthreads, share, &job) == 0 ? QPSK_OK : QPSK_ENOMEM;
}

int qpsk_tx_batch_host(qpsk_tx_state *st, int nch, const uint8_t *bits, int npackets, int gap,
                       int16_t *out, long ld, int nthreads) {
    return qpsk_tx_batch_masked_host(st, nch, bits, NULL, npackets, gap, out, ld, nthreads);
}
