/* qpsk_meter_host.c -- the host twin of the conversion with the level meter in
 * its pass (include/qpsk_input.h: qpsk_input_convert_level_host), and the size
 * of the device call's work area.  The twin is the two twins it is defined by,
 * one after the other: qpsk_input_convert_host (qpsk_input_host.c) and
 * qpsk_level_host (qpsk_level_host.c).  Host C (gcc). */
#include "qpsk_fmt.h"
#include "qpsk_level.h"

size_t qpsk_input_level_work_bytes(int fmt, int nch, int nframes, long ld) {
    return qpsk_input_level_work(fmt, nch, nframes, ld);
}

int qpsk_input_convert_level_host(int fmt, const void *src, long ld, int nch, int nframes,
                                  int16_t *out, qpsk_frame_level *level, int nthreads) {
    if (qpsk_input_check(fmt, nch, nframes, ld) != QPSK_OK) return QPSK_EINVAL;
    if (nframes == 0) return QPSK_OK;
    if (!src || !out || !level) return QPSK_EINVAL;
    const int r = qpsk_input_convert_host(fmt, src, ld, nch, nframes, out, nthreads);
    if (r != QPSK_OK) return r;
    return qpsk_level_host(out, (size_t)nch * (size_t)nframes, level);
}
