/* qpsk_level_tile.h -- the tiling of qpsk_level.hip's meter launch and the
 * argument checks the host twin (qpsk_level_host.c) and the device calls
 * share, in one place.  C and C++. */
#pragma once

#include <stddef.h>
#include <stdint.h>

/* rows (frames of 1880 samples) of one workgroup of the meter: a wave a row */
#define QPSK_LEVEL_BLOCK_ROWS 4
/* nch * nframes of a call stays below this (qpsk_batch.h: QPSK_EINVAL) */
#define QPSK_LEVEL_MAX_ROWS (1ull << 28)
/* sumsq of a frame of -32768: full scale */
#define QPSK_LEVEL_FULL_SUMSQ (1880ull << 30)

#ifdef __cplusplus
extern "C" {
#endif
/* the argument checks of the meter and squelch calls (no HIP call) */
int qpsk_level_check(const void *in, size_t nrows, const void *out);
int qpsk_squelch_check(const void *level, int nch, int nframes, const void *valid_in, const void *valid_out);
#ifdef __cplusplus
}
#endif
