/* qpsk_compact_tile.h -- the tiling of qpsk_compact.hip's three launches, in
 * one place: the kernels, the size of the work area (qpsk_compact_host.c) and
 * the tests' shapes (qpsk_compact_tiling) all read it here.  C and C++. */
#pragma once

#include <stddef.h>

/* items (channel-frames in the order) one wave ranks: one count in the work area */
#define QPSK_COMPACT_RUN_ITEMS 256
/* items of one workgroup of the count and scatter launches: 4 waves' runs */
#define QPSK_COMPACT_BLOCK_ITEMS 1024
/* counts the scan's one workgroup takes in one trip of its loop */
#define QPSK_COMPACT_SCAN_TRIP 1024
/* nch * nframes of a call stays below this (qpsk_batch.h: QPSK_EINVAL) */
#define QPSK_COMPACT_MAX_ITEMS (1ull << 28)

#ifdef __cplusplus
extern "C" {
#endif
/* the argument checks the host twin and the device call share (no HIP call) */
int qpsk_compact_check(const void *bits, const void *valid, int nch, int nframes, int order, size_t cap,
                       const void *rec, const void *count);
#ifdef __cplusplus
}
#endif
