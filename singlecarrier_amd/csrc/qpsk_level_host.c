/* qpsk_level_host.c -- the host twin of the level meter and the squelch
 * (include/qpsk_level.h) in plain C, and the dB helpers.  Every GPU result of
 * qpsk_level.hip is compared with this file.  Host C (gcc), so the sanitizer
 * build covers it. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "qpsk_consts.h"
#include "qpsk_level.h"
#include "qpsk_level_tile.h"

int qpsk_level_check(const void *in, size_t nrows, const void *out) {
    if ((uint64_t)nrows >= QPSK_LEVEL_MAX_ROWS) return QPSK_EINVAL;
    if (nrows > 0 && (!in || !out)) return QPSK_EINVAL;
    return QPSK_OK;
}

int qpsk_squelch_check(const void *level, int nch, int nframes, const void *valid_in, const void *valid_out) {
    if (nch < 0 || nframes < 0) return QPSK_EINVAL;
    const uint64_t n = (uint64_t)nch * (uint64_t)nframes;
    if (n >= QPSK_LEVEL_MAX_ROWS) return QPSK_EINVAL;
    if (n > 0 && (!level || !valid_in || !valid_out)) return QPSK_EINVAL;
    return QPSK_OK;
}

void qpsk_level_tiling(int *rows_per_block) {
    if (rows_per_block) *rows_per_block = QPSK_LEVEL_BLOCK_ROWS;
}

int qpsk_level_host(const int16_t *in, size_t nrows, qpsk_frame_level *out) {
    const int r = qpsk_level_check(in, nrows, out);
    if (r != QPSK_OK) return r;
    for (size_t k = 0; k < nrows; k++) {
        const int16_t *x = in + k * QK_FRAME;
        uint64_t sumsq = 0;
        int32_t sum = 0, peak = 0, clipped = 0;
        for (int i = 0; i < QK_FRAME; i++) {
            const int32_t v = x[i], a = v < 0 ? -v : v;
            sumsq += (uint64_t)((uint32_t)a * (uint32_t)a);
            sum += v;
            if (a > peak) peak = a;
            clipped += v == INT16_MAX || v == INT16_MIN;
        }
        out[k].sumsq = sumsq;
        out[k].sum = sum;
        out[k].peak = (uint16_t)peak;
        out[k].clipped = (uint16_t)clipped;
    }
    return QPSK_OK;
}

static double dbfs_of(uint64_t sumsq) {
    if (sumsq == 0) return -INFINITY;
    return 10.0 * log10((double)sumsq / (double)QPSK_LEVEL_FULL_SUMSQ);
}

double qpsk_level_dbfs(const qpsk_frame_level *level) { return level ? dbfs_of(level->sumsq) : -INFINITY; }

uint64_t qpsk_level_sumsq_of_dbfs(double db) {
    if (isnan(db) || db == -INFINITY) return 0;
    if (db >= 0.0) return QPSK_LEVEL_FULL_SUMSQ;
    /* a guess from the inverse, then the definition itself: the smallest s
     * with dbfs_of(s) >= db (dbfs_of does not decrease with s) */
    const double g = ceil((double)QPSK_LEVEL_FULL_SUMSQ * pow(10.0, db / 10.0));
    uint64_t s = g < 1.0 ? 1 : g >= (double)QPSK_LEVEL_FULL_SUMSQ ? QPSK_LEVEL_FULL_SUMSQ : (uint64_t)g;
    while (s > 1 && dbfs_of(s - 1) >= db) s--;
    while (s < QPSK_LEVEL_FULL_SUMSQ && dbfs_of(s) < db) s++;
    return s;
}

int qpsk_squelch_host(const qpsk_frame_level *level, const qpsk_frame_level *prev, int nch, int nframes,
                      uint64_t min_sumsq, const uint8_t *valid_in, uint8_t *valid_out, uint8_t *bits, float *soft,
                      qpsk_frame_level *last) {
    const int r = qpsk_squelch_check(level, nch, nframes, valid_in, valid_out);
    if (r != QPSK_OK) return r;
    const size_t soft_row = (size_t)QK_NDSYM * 2;
    for (int c = 0; c < nch; c++) {
        qpsk_frame_level end;   /* what the channel carries into the next call */
        if (prev) end = prev[c];
        else memset(&end, 0, sizeof end);
        uint64_t p = end.sumsq;
        for (int f = 0; f < nframes; f++) {
            const size_t i = (size_t)c * (size_t)nframes + (size_t)f;
            const uint64_t cur = level[i].sumsq, w = cur > p ? cur : p;
            const uint8_t v = valid_in[i];
            p = cur;
            if (w >= min_sumsq) {
                valid_out[i] = v;
                continue;
            }
            valid_out[i] = 0;
            if (!v) continue;
            if (bits) memset(bits + i * QK_NBITS, 0, QK_NBITS);
            if (soft) memset(soft + i * soft_row, 0, soft_row * sizeof(float));
        }
        if (nframes > 0) end = level[(size_t)c * (size_t)nframes + (size_t)nframes - 1];
        if (last) last[c] = end;
    }
    return QPSK_OK;
}
