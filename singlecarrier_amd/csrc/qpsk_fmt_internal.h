/* qpsk_fmt_internal.h -- entry points of qpsk_input.hip and qpsk_output.hip
 * that are not part of the C-ABI in include/: the measurements
 * (profiles/input_bench.py, profiles/output_bench.py) and the tests reach them
 * through the library's symbol table. */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qpsk_level.h"

#ifdef __cplusplus
extern "C" {
#endif

/* how the input kernels expand a G.711 code */
enum {
    QPSK_IN_DEC_ARITH = 0,   /* the integer expansion of qpsk_fmt.h */
    QPSK_IN_DEC_TABLE = 1,   /* a 256-entry int16 table in LDS, made by each block */
    /* what qpsk_input_convert_device uses, the faster one of each kernel as
     * measured (profiles/input_bench.json): the table in the planar kernel, the
     * expansion in the interleaved one */
    QPSK_IN_DEC_DEFAULT = -1,
};

/* qpsk_input_convert_device with the decoder named */
int qpsk_input_convert_device_dec(int fmt, const void *d_src, long ld, int nch, int nframes,
                                  int16_t *d_out, void *stream, int dec);

/* qpsk_input_convert_level_device with the decoder named and the grid capped
 * at grid_cap workgroups (0: the launch's own limit).  With a cap below the
 * tiles (interleaved) or the groups of 4 rows (planar) of a small block one
 * workgroup takes several, which the product reaches only past 2^20 of them:
 * the accumulators of that loop must start anew each time. */
int qpsk_input_convert_level_device_grid(int fmt, const void *d_src, long ld, int nch, int nframes,
                                         int16_t *d_out, qpsk_frame_level *d_level, void *d_work, size_t work_bytes,
                                         void *stream, int dec, unsigned grid_cap);

/* qpsk_output_convert_device that also reports which kernel it enqueued:
 * *width (nullable) is the bytes of a lane's global store in the interleaved
 * kernel, 16, 8, 4, 2 or 1, and 0 for a planar block or a refused call */
int qpsk_output_convert_device_w(int fmt, const int16_t *d_src, long src_ld, int nch, long n,
                                 void *d_dst, long ld, void *stream, int *width);

/* bytes of a lane's global load (input) or store (output) for an interleaved
 * block at d_src / d_dst with row stride ld elements of esize bytes: 16, 8, 4,
 * 2 or 1.  One rule (fmt_access_width, qpsk_fmt_dev.h) under both names. */
int qpsk_input_load_width(const void *d_src, long ld, int esize);
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
