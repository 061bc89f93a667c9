/* qpsk_input_internal.h -- entry points of qpsk_input.hip that are not part of
 * the C-ABI in include/: the measurement (profiles/input_bench.py) and the
 * tests reach them through the library's symbol table. */
#pragma once

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* how the kernels expand a G.711 code */
enum {
    QPSK_IN_DEC_ARITH = 0,   /* the integer expansion of qpsk_input_fmt.h */
    QPSK_IN_DEC_TABLE = 1,   /* a 256-entry int16 table in LDS, made by each block */
    /* what qpsk_input_convert_device uses, the faster one of each kernel as
     * measured (profiles/input_bench.json): the table in the planar kernel, the
     * expansion in the interleaved one */
    QPSK_IN_DEC_DEFAULT = -1,
};

/* qpsk_input_convert_device with the decoder named */
int qpsk_input_convert_device_dec(int fmt, const void *d_src, long ld, int nch, int nframes,
                                  int16_t *d_out, void *stream, int dec);

/* bytes of a lane's global load for an interleaved block at d_src with row
 * stride ld elements of esize bytes: 16, 8, 4, 2 or 1 */
int qpsk_input_load_width(const void *d_src, long ld, int esize);

#ifdef __cplusplus
}
#endif
