/*
 * qpsk_rx_stream.c -- the reference RX driver loop (src/qpsk.c:420-461) for
 * many channels at once, streaming: every input file is one channel's .raw
 * stream (int16 LE, 1880-sample frames), read chunk by chunk straight into the
 * pinned slots of a qpsk_stream (include/qpsk_stream.h); the receive of one
 * chunk overlaps the file reads and PCIe copies of the next.  Each channel's
 * 496-byte records go to PREFIX<i>.bin, as the reference writes them
 * (src/qpsk.c:455-457).
 *
 *   qpsk_rx_stream [-f FRAMES_PER_CHUNK] [-f FMT] in1.raw [in2.raw ...] -o PREFIX
 *   qpsk_rx_stream [-f FRAMES_PER_CHUNK] [-f FMT] -i NCH trunk.raw -o PREFIX
 *   qpsk_rx_stream ... -p FILE      (in place of -o PREFIX)
 *   qpsk_rx_stream -q DBFS ... -p FILE
 *
 * -p FILE: one file of 16-byte records (qpsk_frame_rec, include/qpsk_compact.h:
 * channel, frame, the 62 bits in one word) of all channels in time order,
 * instead of the per-channel files: the stream is one of records in by-frame
 * order (qpsk_stream_create_records), only the valid frames cross PCIe, and a
 * record's frame is its position in the whole stream (the chunk's first frame
 * added).  -q DBFS (with -p FILE): the records pass the squelch at that input
 * level, in dB relative to full scale (e.g. -60): frames of idle channels,
 * which the reference calls valid, give no record, and the file holds only the
 * records the squelch keeps (qpsk_stream_create_records_squelch,
 * include/qpsk_level.h; the levels are carried from chunk to chunk).
 *
 * FMT = s16 (default), alaw or ulaw: the files hold 8-bit G.711 codes, which go
 * into the pinned slots and over PCIe as they are and are expanded on the GPU
 * (qpsk_stream_create_fmt, include/qpsk_input.h).  -i NCH: the one input file
 * is a timeslot-interleaved trunk, one sample of each of the NCH channels after
 * another; a chunk of it is a slot's block as it stands, de-interleaved on the
 * GPU.
 * Channels end at the shortest file (whole frames only, as the reference).
 * Build: make -C examples
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_batch.h"
#include "qpsk_compact.h"
#include "qpsk_input.h"
#include "qpsk_internal.h"
#include "qpsk_level.h"
#include "qpsk_stream.h"

static void drain(qpsk_stream *s, int nch, int frames, int nf_chunk, FILE **out, uint8_t *rec) {
    const uint8_t *bits, *valid;
    int err = qpsk_stream_retrieve(s, &bits, &valid);
    if (err) {
        fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
        exit(3);
    }
    for (int c = 0; c < nch; c++) {
        size_t n = qpsk_records(bits + (size_t)c * frames * 62, valid + (size_t)c * frames,
                                nf_chunk, rec);
        if (n && fwrite(rec, 1, n, out[c]) != n) exit(1);
    }
}

/* a chunk of a record stream: the records of its first nf_chunk frames (by-frame
 * order: the first groups[nf_chunk] of them), at first_frame of the stream */
static void drain_records(qpsk_stream *s, int nf_chunk, long first_frame, FILE *out) {
    const qpsk_frame_rec *rec;
    const uint32_t *groups;
    uint32_t count;
    int err = qpsk_stream_retrieve_records(s, &rec, &count, &groups);
    if (err) {
        fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
        exit(3);
    }
    for (uint32_t k = 0; k < groups[nf_chunk]; k++) {
        qpsk_frame_rec r = rec[k];
        r.frame += (uint32_t)first_frame;
        if (fwrite(&r, sizeof r, 1, out) != 1) exit(1);
    }
}

static void usage(const char *argv0) {
    fprintf(stderr, "usage: %s [-f FRAMES_PER_CHUNK] [-f s16|alaw|ulaw] [-q DBFS] (in1.raw [in2.raw ...] | "
                    "-i NCH trunk.raw) (-o PREFIX | -p FILE)   (-q needs -p)\n", argv0);
}

int main(int argc, char **argv) {
    int frames = 8, a = 1, fmt = QPSK_IN_S16, trunk = 0;
    const char *squelch_db = NULL;
    while (a + 1 < argc && (!strcmp(argv[a], "-f") || !strcmp(argv[a], "-i") || !strcmp(argv[a], "-q"))) {
        const char *v = argv[a + 1];
        if (!strcmp(argv[a], "-i")) trunk = atoi(v);
        else if (!strcmp(argv[a], "-q")) squelch_db = v;
        else if (!strcmp(v, "s16")) fmt = QPSK_IN_S16;
        else if (!strcmp(v, "alaw")) fmt = QPSK_IN_ALAW;
        else if (!strcmp(v, "ulaw")) fmt = QPSK_IN_ULAW;
        else frames = atoi(v);
        a += 2;
    }
    const int packed = argc >= 2 && !strcmp(argv[argc - 2], "-p");
    if (argc - a < 3 || (!packed && strcmp(argv[argc - 2], "-o")) || frames < 1 || trunk < 0 ||
        (trunk && argc - a != 3) || (squelch_db && !packed)) {
        usage(argv[0]);
        return 2;
    }
    const int nfile = argc - a - 2, nch = trunk ? trunk : nfile;
    const size_t es = fmt == QPSK_IN_S16 ? sizeof(int16_t) : 1;
    if (trunk) fmt |= QPSK_IN_INTERLEAVED;
    const char *prefix = argv[argc - 1];
    FILE **in = calloc((size_t)nfile, sizeof(FILE *)), **out = calloc((size_t)nch, sizeof(FILE *));
    FILE *pout = packed ? fopen(prefix, "wb") : NULL;
    if (packed && !pout) return 1;
    for (int c = 0; c < nch; c++) {
        char name[4096];
        snprintf(name, sizeof name, "%s%d.bin", prefix, c);
        if (c < nfile && !(in[c] = fopen(argv[a + c], "rb"))) return 1;
        if (packed) continue;
        out[c] = fopen(name, "wb");
        if (!out[c]) return 1;
    }
    const int nslot = 3;
    int err;
    /* (planar int16 is the plain stream: qpsk_stream_create) */
    const size_t cap = (size_t)nch * (size_t)frames;
    qpsk_stream *s = squelch_db ? qpsk_stream_create_records_squelch(0, nch, frames, nslot, QPSK_MODE_REFERENCE, fmt,
                                                                     QPSK_REC_BY_FRAME, cap,
                                                                     qpsk_level_sumsq_of_dbfs(atof(squelch_db)), &err)
                   : packed     ? qpsk_stream_create_records(0, nch, frames, nslot, QPSK_MODE_REFERENCE, fmt,
                                                             QPSK_REC_BY_FRAME, cap, &err)
                                : qpsk_stream_create_fmt(0, nch, frames, nslot, QPSK_MODE_REFERENCE, fmt, &err);
    if (!s) {
        fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
        return 3;
    }
    uint8_t *rec = malloc((size_t)frames * BITS_PER_FRAME);
    int sizes[4] = {0};   /* frames in each slot's chunk (slots are used in order) */
    long submitted = 0, retrieved = 0;
    for (int done = 0; !done;) {
        if (qpsk_stream_pending(s) == nslot) {
            if (packed) drain_records(s, sizes[retrieved % nslot], retrieved * frames, pout);
            else drain(s, nch, frames, sizes[retrieved % nslot], out, rec);
            retrieved++;
        }
        char *buf = qpsk_stream_acquire_raw(s, &err);
        if (!buf) {
            fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
            return 3;
        }
        /* every channel contributes the same number of whole frames */
        int nf = frames;
        if (trunk) {   /* FRAME_SIZE rows of nch samples make a frame of every channel */
            nf = (int)fread(buf, es * FRAME_SIZE * (size_t)nch, (size_t)frames, in[0]);
        } else {
            for (int c = 0; c < nch; c++) {
                size_t got = fread(buf + es * (size_t)c * frames * FRAME_SIZE, es * FRAME_SIZE,
                                   (size_t)nf, in[c]);                       /* src/qpsk.c:442 */
                if ((int)got < nf) nf = (int)got;
            }
        }
        if (nf < frames) done = 1;   /* the shortest stream ended inside this chunk */
        if (nf == 0) break;
        /* frames past nf of a short chunk are received too but never written out */
        if ((err = qpsk_stream_submit(s))) {
            fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
            return 3;
        }
        sizes[submitted % nslot] = nf;
        submitted++;
    }
    while (retrieved < submitted) {
        if (packed) drain_records(s, sizes[retrieved % nslot], retrieved * frames, pout);
        else drain(s, nch, frames, sizes[retrieved % nslot], out, rec);
        retrieved++;
    }
    qpsk_stream_destroy(s);
    for (int c = 0; c < nch; c++) {
        if (c < nfile) fclose(in[c]);
        if (out[c]) fclose(out[c]);
    }
    if (pout) fclose(pout);
    free(rec);
    return 0;
}
