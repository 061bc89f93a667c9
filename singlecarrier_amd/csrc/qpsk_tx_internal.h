// qpsk_tx_internal.h -- shared between the transmit-side translation units
// (qpsk_synth_dev.hip, qpsk_tx.hip, and qpsk_output.hip for the transmitter's
// formats); not part of the public surface.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A packet of the batched transmitter (include/qpsk_tx.h): its transmitted
 * samples and its payload bytes.  qpsk_tx_batch and the format entry points
 * refuse nch * npackets from QPSK_TX_MAX_CHANNEL_PACKETS on. */
enum { QPSK_TX_PACKET = 1880, QPSK_TX_PACKET_BITS = 496 };
#define QPSK_TX_MAX_CHANNEL_PACKETS (1L << 28)

/* The loop of qpsk_tx_phase_table() (include/qpsk_synth.h) from a carried
 * phase: ph[2] is fbb_tx_phase (re, im) before the first of these samples and,
 * on return, after the last call's renormalisation.  The call sequence starts
 * at a packet's preamble, so a carried phase is only meaningful when ntx is a
 * multiple of 1880. */
void qpsk_tx_phase_run(float *out2, long ntx, float ph[2]);

/* Output in another format than planar int16 (include/qpsk_output.h).  The
 * transmitter knows nothing of formats: qpsk_output.hip, which has the
 * conversions, builds the format entry points on the hooks below, and
 * qpsk_tx.hip refers to no symbol of it.
 *
 * A grow-only device buffer of n int16 the context owns, which the modulator
 * writes and the conversion reads (a call larger than every earlier one waits
 * for the device before the buffer is reallocated). */
struct qpsk_tx_ctx;
int qpsk_tx_fmt_conv(struct qpsk_tx_ctx *c, size_t n, int16_t **p);
/* the context's device, and the stream its host calls run on (a hipStream_t) */
int qpsk_tx_device(const struct qpsk_tx_ctx *c);
void *qpsk_tx_host_stream(const struct qpsk_tx_ctx *c);
/* qpsk_tx_batch_device() with the element tx_batch_kernel's store pass writes
 * named by an encoding of the format word: int16 (QPSK_OUT_S16, the plain
 * call), or the sample's G.711 code (QPSK_OUT_ALAW, QPSK_OUT_ULAW) into d_out as
 * uint8 [nch][ld], any address: the planar G.711 formats without a pre-pass. */
int qpsk_tx_batch_device_enc(struct qpsk_tx_ctx *c, const uint8_t *d_bits, int npackets, void *d_out,
                             long ld, void *stream, int enc);
/* the same for qpsk_tx_batch_masked_device(); d_active NULL = every slot
 * active, which is the call above */
int qpsk_tx_batch_masked_device_enc(struct qpsk_tx_ctx *c, const uint8_t *d_bits, const uint8_t *d_active,
                                    int npackets, void *d_out, long ld, void *stream, int enc);
/* what qpsk_tx_sync() and qpsk_tx_destroy() wait for moves behind the work
 * enqueued on `stream` so far: the conversion that follows the modulator */
int qpsk_tx_mark(struct qpsk_tx_ctx *c, void *stream);

#ifdef __cplusplus
}
#endif
