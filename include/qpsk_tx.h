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

#include <stddef.h>
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

/* Channels that come and go (INTEGRATION.md "Transmit channels that come and
 * go"): the transmit counterpart of qpsk_rx_reset_channels and
 * qpsk_rx_state_save/join.
 *
 * Own packet index.  Every channel has a 64-bit packet index of its own: the
 * number of packets of its current stream it has sent.  It is the context's
 * (qpsk_tx_packets) until one of the calls below gives the channel another
 * course.  A channel always behaves exactly like a fresh run of the reference
 * transmitter (src/qpsk.c:278-322 in the order of :380-413) fed its own
 * packets, and its line carries runs of zeros wherever it was idle.
 *
 * Slots.  A call covers npackets slots of P = 1880 + gap samples per channel.
 *   active  uint8 [nch][npackets]; nonzero = the channel sends in that slot.
 *           NULL = every slot is active (the plain call).
 * An active slot holds the 1880 samples of the channel's next packet, bits
 * row [c][slot]: filtered over the last 9 dibits of the channel's previous
 * active packet, whatever lies between the two and whether that packet was in
 * this call or an earlier one (zero filter memory before the channel's first
 * packet), on the carrier of the channel's own index (1+0i before its first
 * packet); then gap zeros.  The own index advances by one.
 * An idle slot holds P zeros (the encoded zero in the G.711 formats, as the gap
 * does).  Its bits row is not read, and the channel's state, its 9 dibits and
 * its own index, does not move.
 * Per row a call writes exactly npackets * P elements, as the plain call does.
 * qpsk_tx_packets() stays the context's count of slots since create / reset.
 *
 * The plain calls (qpsk_tx_batch, _device, and qpsk_output.h's _fmt forms) keep
 * working after any of the calls below: they mean "every slot active" over the
 * channels' own indices.  Masked, plain and format calls may alternate, and
 * calls of 1 + 3 + 1 slots equal one call of 5 with the same mask rows.  A
 * context that uses none of the calls below (a NULL mask counts as none) is as
 * before in every respect.
 *
 * Errors: every argument check runs before any HIP call.  QPSK_EINVAL for what
 * the plain calls refuse, for a NULL context, and for c0 < 0, n < 0 or
 * c0 + n > channels, a NULL out with n > 0, and for qpsk_tx_state_save / _load
 * n < 1, a NULL buf, size < qpsk_tx_state_size(n), and for _load a snapshot
 * that is foreign, of another version or of another n.  For
 * qpsk_tx_reset_channels and qpsk_tx_channel_packets n == 0 is a no-op
 * returning 0 (they still wait for the calls in flight).  A device allocation
 * that fails on a call's way out of the uniform state is QPSK_ENOMEM.
 *
 *   qpsk_tx_batch_masked(ctx, bits, active, npackets, out, ld)
 *       qpsk_tx_batch with a mask; host memory, synchronises.
 *   qpsk_tx_batch_masked_device(ctx, d_bits, d_active, npackets, d_out, ld, stream)
 *       qpsk_tx_batch_device with a mask in device memory (any address), read
 *       in stream order on `stream` like d_bits; the call synchronises
 *       nothing beyond what qpsk_tx_batch_device's contract names (here only
 *       a call of more slots than any masked one before it, which reallocates
 *       the per-slot plan).
 *   qpsk_tx_reset_channels(ctx, c0, n)
 *       channels [c0, c0 + n) back to the start state (zero filter memory,
 *       carrier 1+0i) at own index 0; every other channel is untouched.
 *       Waits for the context's calls in flight.
 *   qpsk_tx_channel_packets(ctx, c0, n, out)
 *       out[i] = own index of channel c0 + i.  Waits for the context's calls
 *       in flight (the indices live on the device once a masked call has run).
 *   qpsk_tx_state_size(n)
 *       bytes of a snapshot of n channels: 16 + 12 n; 0 for n < 1.
 *   qpsk_tx_state_save(ctx, c0, n, buf, size)
 *       channels [c0, c0 + n) -> buf (host memory, size >= state_size(n)).
 *   qpsk_tx_state_load(ctx, c0, n, buf, size)
 *       buf -> channels [c0, c0 + n) of ctx, with the receive side's *join*
 *       meaning: the channels continue at the snapshot's indices, in a context
 *       at any other index, with any gap (gap is not state), on any device, in
 *       any process, while the context's other channels go on.
 *   Save and load wait for the context's calls in flight.
 *
 * Snapshot layout, little endian, version 1:
 *   offset 0   uint32  magic 0x53585451 ("QTXS")
 *          4   uint32  version = 1
 *          8   uint32  n
 *         12   uint32  0
 *         16   uint64  own index of channel c0 + i, i = 0 .. n-1
 *   16 + 8 n   uint32  the channel's last 9 dibits: bit j = I sign (1: -1) of
 *                      data symbol 239 + j of its latest packet, bit 16 + j its
 *                      Q sign, j = 0 .. 8; every other bit 0, and the whole word
 *                      0 when the index is 0
 * A snapshot is a function of the channels' state alone: equal states give equal
 * bytes wherever and however they were reached.  qpsk_tx_state_load refuses
 * words with other bits set and a nonzero word at index 0. */
int qpsk_tx_batch_masked(qpsk_tx_ctx *ctx, const uint8_t *bits, const uint8_t *active, int npackets,
                         int16_t *out, long ld);
int qpsk_tx_batch_masked_device(qpsk_tx_ctx *ctx, const uint8_t *d_bits, const uint8_t *d_active,
                                int npackets, int16_t *d_out, long ld, void *stream);
int qpsk_tx_reset_channels(qpsk_tx_ctx *ctx, int c0, int n);
int qpsk_tx_channel_packets(qpsk_tx_ctx *ctx, int c0, int n, uint64_t *out);
size_t qpsk_tx_state_size(int n);
int qpsk_tx_state_save(qpsk_tx_ctx *ctx, int c0, int n, void *buf, size_t size);
int qpsk_tx_state_load(qpsk_tx_ctx *ctx, int c0, int n, const void *buf, size_t size);

/* The masked call on the host, as qpsk_tx_batch_host is for the plain call:
 * an idle slot writes P zeros and leaves st[c] alone.  The yardstick of every
 * GPU result.  active NULL: qpsk_tx_batch_host. */
int qpsk_tx_batch_masked_host(qpsk_tx_state *st, int nch, const uint8_t *bits, const uint8_t *active,
                              int npackets, int gap, int16_t *out, long ld, int nthreads);

#ifdef __cplusplus
}
#endif
