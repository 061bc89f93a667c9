/*
 * qpsk_tx.h -- batched, multi-channel transmitter for caller-supplied payload
 * bits: the transmit half of the batched C-ABI (qpsk_batch.h is the receive
 * half).
 *
 * Every channel is the reference transmitter (qpsk_tx_frame, src/qpsk.c:278-322)
 * driven in the packet order of its main() (src/qpsk.c:380-413): per packet the
 * 128-symbol preamble at half amplitude, 8 x 31 QPSK data symbols, then `gap`
 * zero samples.  The int16 samples are those of the unmodified reference.  The
 * state the reference carries in statics (tx_filter, fbb_tx_phase) lives in
 * the context and persists across calls, so a stream may be sent in any number
 * of calls: five packets in one call equal calls of 1 + 3 + 1 packets.
 * Contexts are independent and may be used from different host threads; one
 * context must not be used concurrently.  Error codes are qpsk_batch.h's.
 */
#pragma once

#include <stdint.h>

#include "qpsk_batch.h"
#include "qpsk_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qpsk_tx_ctx qpsk_tx_ctx;

/* nch channels on HIP device `device`, in main()'s TX start state
 * (tx_filter zero, fbb_tx_phase = 1+0i, src/qpsk.c:375).
 * gap = zero samples written after each packet (the reference writes 903,
 * src/qpsk.c:410-412; 0 = continuous).
 * nch < 1 or gap < 0: QPSK_EINVAL, checked before any HIP call.  Returns NULL
 * on failure; *err (if non-NULL) receives the error code. */
qpsk_tx_ctx *qpsk_tx_create(int device, int nch, int gap, int *err);
void qpsk_tx_destroy(qpsk_tx_ctx *ctx);
/* Back to the start state; waits for the context's calls in flight. */
int qpsk_tx_reset(qpsk_tx_ctx *ctx);
int qpsk_tx_channels(const qpsk_tx_ctx *ctx);
int qpsk_tx_gap(const qpsk_tx_ctx *ctx);
/* Packets sent so far by every channel. */
uint64_t qpsk_tx_packets(const qpsk_tx_ctx *ctx);

/* bits  uint8 [nch][npackets][8][62], in qpsk_rx_batch's output layout and
 *       meaning: bits[2s] = Q, bits[2s+1] = I.  A byte == 1 maps to -1; every
 *       other value maps to +1 (qpsk_mod's `== 1` test, src/qpsk.c:252-253).
 * out   int16 [nch][ld], ld >= npackets * (1880 + gap).  Per channel the call
 *       writes exactly npackets * (1880 + gap) samples: 640 preamble samples at
 *       x8192, then 8 x 155 data samples at x16384, then gap zeros, for each
 *       packet.  It touches nothing else: out[c][npackets*(1880+gap) .. ld)
 *       keeps its contents.  out is 2-byte aligned; any ld is accepted.
 * npackets == 0 is a no-op returning 0.
 * QPSK_EINVAL for: npackets < 0; ld too small; nch * npackets >= 2^28; NULL
 * bits or out with npackets > 0 (and a NULL context).
 *
 * qpsk_tx_batch: host memory; copies in, modulates, copies the written
 * samples back and synchronises.  It runs on a stream of the context's own,
 * which a caller cannot chain behind theirs, so it orders itself: a
 * qpsk_tx_batch_device call still pending on a caller's stream is waited for
 * first (as qpsk_tx_reset does), and the call continues the stream from the
 * state that one leaves.  qpsk_tx_batch_fmt (qpsk_output.h) does the same. */
int qpsk_tx_batch(qpsk_tx_ctx *ctx, const uint8_t *bits, int npackets, int16_t *out, long ld);
/* Device memory on the context's device; the work is enqueued on `stream` (a
 * hipStream_t, NULL = default stream) and the call does not wait for the
 * kernel.  Calls on one context depend on each other through the carried
 * state, so the caller orders them (one stream, or streams it chains).
 * Two things can make a call wait.  The carrier of a call's samples is built
 * on the host in one of two pinned staging slots and uploaded on `stream`: a
 * call finds a free slot as long as at most one earlier call's upload is
 * still pending, so two calls in a row never wait for each other, and a third
 * waits until the first one's upload has run.  And a call of more packets
 * than any before it on the context reallocates the carrier table and the
 * slot, which waits for the whole device (earlier calls may still read them);
 * a first call of the largest size leaves every later call free of that. */
int qpsk_tx_batch_device(qpsk_tx_ctx *ctx, const uint8_t *d_bits, int npackets,
                         int16_t *d_out, long ld, void *stream);
/* Waits for the context's latest qpsk_tx_batch_device call. */
int qpsk_tx_sync(qpsk_tx_ctx *ctx);

/* The same contract on the host, over the explicit states of qpsk_synth.h.
 * st[nch] is advanced; nthreads host threads split the channels (< 1: one).
 * QPSK_EINVAL also for NULL st, nch < 1 or gap < 0. */
int qpsk_tx_batch_host(qpsk_tx_state *st, int nch, const uint8_t *bits, int npackets, int gap,
                       int16_t *out, long ld, int nthreads);

#ifdef __cplusplus
}
#endif
