/*
 * qpsk_rx_raw.c -- the reference RX driver loop (src/qpsk.c:420-461) built
 * against the drop-in library instead of the reference sources.
 *
 *   qpsk_rx_raw in.raw out.bin            single channel, qpsk_rx_frame() per frame
 *                                          (unchanged reference call pattern)
 *   qpsk_rx_raw -b [-m MODE] [-f FMT] [-q DBFS] in1.raw [in2.raw ...] -o PREFIX
 *                                          every file is one channel; all channels are
 *                                          demodulated together through qpsk_rx_batch()
 *                                          and PREFIX<i>.bin is written per channel;
 *                                          MODE = QPSK_MODE_* (qpsk_batch.h, default 0:
 *                                          the reference; 1 dec752, 2 FFT hunt, 3 both);
 *                                          FMT = s16 (default), alaw or ulaw: the files
 *                                          hold 8-bit G.711 codes, 1880 to a frame, which
 *                                          cross PCIe as they are and are expanded on the
 *                                          GPU (qpsk_rx_batch_fmt, qpsk_input.h);
 *                                          -q DBFS squelches at that input level (dB
 *                                          relative to full scale, e.g. -60): frames of
 *                                          idle channels, which the reference calls
 *                                          valid, give no record (qpsk_level.h: the
 *                                          meter, the squelch and the compaction run on
 *                                          the GPU, qpsk_rx_batch_records_squelch_fmt)
 *   qpsk_rx_raw -f FMT in.g711 out.bin     one channel of G.711 codes, the same way
 * Output: one 496-byte record per valid frame, bits in bytes 0..61 (the
 * reference's /tmp/databits.txt format, src/qpsk.c:455-457).
 * Build: gcc -O2 -Iinclude qpsk_rx_raw.c -Lsinglecarrier_amd -lqpsk_hip -Wl,-rpath,...
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_batch.h"
#include "qpsk_compact.h"
#include "qpsk_input.h"
#include "qpsk_internal.h"
#include "qpsk_level.h"

/* the whole frames of a file whose samples are `es` bytes each */
static void *read_frames(const char *path, size_t es, int *nframes) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    *nframes = (int)(bytes / (long)(es * FRAME_SIZE));  /* short tail dropped */
    void *buf = malloc(es * (size_t)(*nframes > 0 ? *nframes : 1) * FRAME_SIZE);
    if (buf && fread(buf, es * FRAME_SIZE, (size_t)*nframes, f) != (size_t)*nframes) {
        free(buf);
        buf = NULL;
    }
    fclose(f);
    return buf;
}

static int single(const char *in, const char *out) {
    FILE *fin = fopen(in, "rb"), *fout = fopen(out, "wb");
    if (!fin || !fout) return 1;
    int16_t frame[FRAME_SIZE];
    uint8_t ibits[BITS_PER_FRAME];
    qpsk_rx_init();
    if (qpsk_surface_error()) {
        fprintf(stderr, "qpsk: %s\n", qpsk_strerror(qpsk_surface_error()));
        return 3;
    }
    while (fread(frame, sizeof(int16_t), FRAME_SIZE, fin) == FRAME_SIZE) {   /* src/qpsk.c:442 */
        memset(ibits, 0, sizeof ibits);
        int valid = qpsk_rx_frame(frame, ibits);                              /* src/qpsk.c:447 */
        if (qpsk_surface_error()) {
            fprintf(stderr, "qpsk: %s\n", qpsk_strerror(qpsk_surface_error()));
            return 3;
        }
        if (valid) fwrite(ibits, sizeof(uint8_t), BITS_PER_FRAME, fout);        /* src/qpsk.c:455 */
    }
    fclose(fin);
    fclose(fout);
    return 0;
}

/* The same output files behind the squelch: the receive, the level meter, the
 * squelch at min_sumsq and the compaction on the GPU; the records that come
 * back are the frames to write, by channel.  G.711 codes cross PCIe as they
 * are here too: the conversion on the GPU takes the levels in its own pass. */
static int squelched(qpsk_ctx *ctx, int nch, int nf, const char *in, int fmt, uint64_t min_sumsq,
                     const char *prefix) {
    const size_t cf = (size_t)nch * nf;
    qpsk_frame_rec *recs = malloc(sizeof *recs * cf);
    uint32_t *groups = malloc(sizeof *groups * ((size_t)nch + 1)), count = 0;
    const int err = qpsk_rx_batch_records_squelch_fmt(ctx, in, fmt | QPSK_IN_PLANAR, 0, nf, min_sumsq, NULL,
                                                      QPSK_REC_BY_CHANNEL, cf, recs, NULL, NULL, groups, &count,
                                                      NULL);
    if (err) {
        fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
        return 3;
    }
    uint8_t rec[BITS_PER_FRAME];
    for (int c = 0; c < nch; c++) {
        char name[4096];
        snprintf(name, sizeof name, "%s%d.bin", prefix, c);
        FILE *fo = fopen(name, "wb");
        if (!fo) return 1;
        for (uint32_t k = groups[c]; k < groups[c + 1]; k++) {
            memset(rec, 0, sizeof rec);
            qpsk_bits_unpack_host(&recs[k].bits, 1, rec);
            fwrite(rec, 1, sizeof rec, fo);
        }
        fclose(fo);
    }
    free(recs), free(groups);
    return 0;
}

/* prefix: PREFIX<i>.bin per channel; else one channel to the file `single_out`;
 * squelch_db: NULL, or the level of -q */
static int batch(int nch, char **paths, const char *prefix, const char *single_out, int mode, int fmt,
                 const char *squelch_db) {
    int nf = -1;
    const size_t es = fmt == QPSK_IN_S16 ? sizeof(int16_t) : 1;
    void **ch = calloc((size_t)nch, sizeof(void *));
    for (int c = 0; c < nch; c++) {
        int n;
        ch[c] = read_frames(paths[c], es, &n);
        if (!ch[c]) return 1;
        if (nf < 0 || n < nf) nf = n;   /* common length: frames every channel has */
    }
    if (nf <= 0) return 1;
    char *in = malloc(es * (size_t)nch * nf * FRAME_SIZE);
    for (int c = 0; c < nch; c++)
        memcpy(in + es * (size_t)c * nf * FRAME_SIZE, ch[c], es * (size_t)nf * FRAME_SIZE);
    uint8_t *bits = malloc((size_t)nch * nf * 62), *valid = malloc((size_t)nch * nf);
    int err;
    qpsk_ctx *ctx = qpsk_rx_create_mode(0, nch, mode, &err);
    if (!ctx) {
        fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
        return 3;
    }
    if (squelch_db) {
        err = squelched(ctx, nch, nf, in, fmt, qpsk_level_sumsq_of_dbfs(atof(squelch_db)), prefix);
        qpsk_rx_destroy(ctx);
        return err;
    }
    err = qpsk_rx_batch_fmt(ctx, in, fmt | QPSK_IN_PLANAR, 0, nf, bits, valid, NULL, NULL);
    if (err) {
        fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
        return 3;
    }
    uint8_t rec[BITS_PER_FRAME];
    for (int c = 0; c < nch; c++) {
        char name[4096];
        if (prefix) snprintf(name, sizeof name, "%s%d.bin", prefix, c);
        else snprintf(name, sizeof name, "%s", single_out);
        FILE *fo = fopen(name, "wb");
        if (!fo) return 1;
        for (int n = 0; n < nf; n++) {
            if (!valid[(size_t)c * nf + n]) continue;
            memset(rec, 0, sizeof rec);
            memcpy(rec, bits + ((size_t)c * nf + n) * 62, 62);
            fwrite(rec, 1, sizeof rec, fo);
        }
        fclose(fo);
    }
    qpsk_rx_destroy(ctx);
    return 0;
}

static int format_of(const char *name) {
    return !strcmp(name, "s16") ? QPSK_IN_S16 : !strcmp(name, "alaw") ? QPSK_IN_ALAW
         : !strcmp(name, "ulaw") ? QPSK_IN_ULAW : -1;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "-f") && format_of(argv[2]) >= 0)
        return batch(1, argv + 3, NULL, argv[4], QPSK_MODE_REFERENCE, format_of(argv[2]), NULL);
    if (argc >= 3 && strcmp(argv[1], "-b") != 0 && strcmp(argv[1], "-f") != 0) return single(argv[1], argv[2]);
    if (argc >= 5 && !strcmp(argv[1], "-b") && !strcmp(argv[argc - 2], "-o")) {
        int first = 2, mode = QPSK_MODE_REFERENCE, fmt = QPSK_IN_S16;
        if (argc >= first + 5 && !strcmp(argv[first], "-m")) {
            mode = atoi(argv[first + 1]);
            first += 2;
        }
        if (argc >= first + 5 && !strcmp(argv[first], "-f")) {
            fmt = format_of(argv[first + 1]);
            first += 2;
        }
        const char *squelch_db = NULL;
        if (argc >= first + 5 && !strcmp(argv[first], "-q")) {
            squelch_db = argv[first + 1];
            first += 2;
        }
        if (fmt >= 0) return batch(argc - 2 - first, argv + first, argv[argc - 1], NULL, mode, fmt, squelch_db);
    }
    fprintf(stderr, "usage: %s in.raw out.bin | -f FMT in.g711 out.bin | -b [-m MODE] [-f FMT] [-q DBFS] in1.raw "
                    "[in2.raw ...] -o PREFIX   (FMT: s16, alaw, ulaw)\n", argv[0]);
    return 2;
}
