/* qpsk_output_internal.h -- entry points of qpsk_output.hip that are not part of
 * the C-ABI in include/: the measurement (profiles/output_bench.py) and the
 * tests reach them through the library's symbol table. */
#pragma once

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* qpsk_output_convert_device that also reports which kernel it enqueued:
 * *width (nullable) is the bytes of a lane's global store in the interleaved
 * kernel, 16, 8, 4, 2 or 1, and 0 for a planar block or a refused call */
int qpsk_output_convert_device_w(int fmt, const int16_t *d_src, long src_ld, int nch, long n,
                                 void *d_dst, long ld, void *stream, int *width);

/* bytes of a lane's global store for an interleaved block at d_dst with row
 * stride ld elements of esize bytes: 16, 8, 4, 2 or 1 */
int qpsk_output_store_width(const void *d_dst, long ld, int esize);

/* how qpsk_tx_batch_device_fmt makes a block */
enum {
    QPSK_OUT_PATH_PREPASS = 0,   /* the modulator writes int16 into the context's buffer, a conversion follows */
    QPSK_OUT_PATH_FUSED = 1,     /* planar G.711 only: tx_batch_kernel's store pass writes the codes */
    /* what qpsk_tx_batch_device_fmt uses: the fused store for planar G.711 (the
     * faster one as measured, profiles/output_bench.json), the pre-pass otherwise */
    QPSK_OUT_PATH_DEFAULT = -1,
};

/* qpsk_tx_batch_device_fmt with the path named; QPSK_EINVAL for a path the
 * format has not */
struct qpsk_tx_ctx;
int qpsk_tx_batch_device_fmt_path(struct qpsk_tx_ctx *c, const uint8_t *d_bits, int npackets, void *d_out,
                                  int fmt, long ld, void *stream, int path);

#ifdef __cplusplus
}
#endif
