// qpsk_tx_internal.h -- shared between the two transmit-side translation units
// (qpsk_synth_dev.hip, qpsk_tx.hip); not part of the public surface.
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

/* The loop of qpsk_tx_phase_table() (include/qpsk_synth.h) from a carried
 * phase: ph[2] is fbb_tx_phase (re, im) before the first of these samples and,
 * on return, after the last call's renormalisation.  The call sequence starts
 * at a packet's preamble, so a carried phase is only meaningful when ntx is a
 * multiple of 1880. */
void qpsk_tx_phase_run(float *out2, long ntx, float ph[2]);

#ifdef __cplusplus
}
#endif
