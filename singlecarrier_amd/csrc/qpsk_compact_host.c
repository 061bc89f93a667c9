/* qpsk_compact_host.c -- the host twin of the receive output's format layer
 * (include/qpsk_compact.h): bit packing and the compaction of the dense
 * receive outputs into records, in plain C.  Every GPU result of
 * qpsk_compact.hip is compared with this file, and it is the path of a machine
 * without a GPU.  Host C (gcc), so the sanitizer build covers it. */
#include <stdint.h>
#include <string.h>

#include "qpsk_compact.h"
#include "qpsk_compact_tile.h"
#include "qpsk_consts.h"

static uint64_t pack_row(const uint8_t *row) {
    uint64_t w = 0;
    for (int i = 0; i < QK_NBITS; i++) w |= (uint64_t)(row[i] == 1) << i;
    return w;
}

int qpsk_bits_pack_host(const uint8_t *bits, size_t n, uint64_t *words) {
    if (n > 0 && (!bits || !words)) return QPSK_EINVAL;
    for (size_t k = 0; k < n; k++) words[k] = pack_row(bits + k * QK_NBITS);
    return QPSK_OK;
}

int qpsk_bits_unpack_host(const uint64_t *words, size_t n, uint8_t *bits) {
    if (n > 0 && (!bits || !words)) return QPSK_EINVAL;
    for (size_t k = 0; k < n; k++)
        for (int i = 0; i < QK_NBITS; i++) bits[k * QK_NBITS + i] = (uint8_t)((words[k] >> i) & 1u);
    return QPSK_OK;
}

int qpsk_compact_check(const void *bits, const void *valid, int nch, int nframes, int order, size_t cap,
                       const void *rec, const void *count) {
    if (order != QPSK_REC_BY_CHANNEL && order != QPSK_REC_BY_FRAME) return QPSK_EINVAL;
    if (nch < 0 || nframes < 0 || !count || (cap > 0 && !rec)) return QPSK_EINVAL;
    const uint64_t n = (uint64_t)nch * (uint64_t)nframes;
    if (n >= QPSK_COMPACT_MAX_ITEMS) return QPSK_EINVAL;
    if (n > 0 && (!bits || !valid)) return QPSK_EINVAL;
    return QPSK_OK;
}

size_t qpsk_compact_work_bytes(int nch, int nframes) {
    if (nch < 0 || nframes < 0) return 0;
    const uint64_t n = (uint64_t)nch * (uint64_t)nframes;
    if (n >= QPSK_COMPACT_MAX_ITEMS) return 0;
    const uint64_t runs = (n + QPSK_COMPACT_RUN_ITEMS - 1) / QPSK_COMPACT_RUN_ITEMS;
    return sizeof(uint32_t) * (size_t)(runs ? runs : 1);
}

void qpsk_compact_tiling(int *run_items, int *block_items, int *scan_trip) {
    if (run_items) *run_items = QPSK_COMPACT_RUN_ITEMS;
    if (block_items) *block_items = QPSK_COMPACT_BLOCK_ITEMS;
    if (scan_trip) *scan_trip = QPSK_COMPACT_SCAN_TRIP;
}

int qpsk_compact_host(const uint8_t *bits, const uint8_t *valid, const int32_t *trace, const float *soft,
                      int nch, int nframes, int order, size_t cap, qpsk_frame_rec *rec, int32_t *rec_trace,
                      float *rec_soft, uint32_t *groups, uint32_t *count) {
    const int r = qpsk_compact_check(bits, valid, nch, nframes, order, cap, rec, count);
    if (r != QPSK_OK) return r;
    const int by_frame = order == QPSK_REC_BY_FRAME;
    /* the order walks `outer` groups of `inner` items each */
    const int outer = by_frame ? nframes : nch, inner = by_frame ? nch : nframes;
    const size_t soft_row = (size_t)QK_NDSYM * 2;
    uint32_t rank = 0;
    for (int g = 0; g < outer; g++) {
        if (groups) groups[g] = rank;
        for (int k = 0; k < inner; k++) {
            const int c = by_frame ? k : g, f = by_frame ? g : k;
            const size_t src = (size_t)c * (size_t)nframes + (size_t)f;
            if (!valid[src]) continue;
            if (rank < cap) {
                if (rec) {
                    rec[rank].channel = (uint32_t)c;
                    rec[rank].frame = (uint32_t)f;
                    rec[rank].bits = pack_row(bits + src * QK_NBITS);
                }
                if (rec_trace && trace) memcpy(rec_trace + (size_t)rank * 4, trace + src * 4, 4 * sizeof(int32_t));
                if (rec_soft && soft)
                    memcpy(rec_soft + (size_t)rank * soft_row, soft + src * soft_row, soft_row * sizeof(float));
            }
            rank++;
        }
    }
    if (groups) groups[outer] = rank;
    *count = rank;
    return QPSK_OK;
}
