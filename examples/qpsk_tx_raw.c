/*
 * qpsk_tx_raw.c -- the reference TX loop (src/qpsk.c:380-413) with the payload
 * read from a file instead of rand(), through the batched transmitter
 * (include/qpsk_tx.h, include/qpsk_output.h).
 *
 *   qpsk_tx_raw [-g GAP] [-f FMT] in.bits out.raw     one channel
 *   qpsk_tx_raw -b [-g GAP] [-f FMT] in1.bits [in2.bits ...] -o PREFIX
 *                                            every file is one channel; all channels are
 *                                            modulated together through qpsk_tx_batch_fmt()
 *                                            and PREFIX<i>.raw is written per channel
 *   qpsk_tx_raw -b -i [-g GAP] [-f FMT] in1.bits [in2.bits ...] -o TRUNK
 *                                            the batch as one timeslot-interleaved trunk file:
 *                                            one sample of every channel after another, what
 *                                            qpsk_rx_stream -i NCH reads
 *   -a    with -b: send every file to its own end.  A channel whose file has ended goes idle
 *         (zeros on its line, qpsk_tx_batch_masked_fmt) while the others keep sending, instead
 *         of all stopping at the shortest file
 *   -f s16|alaw|ulaw   int16 samples (default) or 8-bit G.711 codes, made on the GPU
 *   -c    modulate on the host (qpsk_tx_batch_host, qpsk_output_convert_host) instead of the GPU
 *
 * Input: 0/1 bytes, 496 per packet (8 frames of 62 bits, bits[2s] = Q,
 * bits[2s+1] = I: the layout qpsk_rx_raw writes); a short tail is dropped, and
 * -b sends the packets every file has (-a: the packets any file has).  Output: the reference's .raw framing,
 * samples at 8 kHz: per packet 640 preamble samples, 8 x 155 data samples, GAP
 * zeros (default 903, as the reference writes).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpsk_output.h"
#include "qpsk_tx.h"

#define PACKET_BITS 496
#define TX_PACKET 1880

static uint8_t *read_packets(const char *path, int *npackets) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    *npackets = (int)(bytes / PACKET_BITS);
    uint8_t *buf = malloc((size_t)(*npackets > 0 ? *npackets : 1) * PACKET_BITS);
    if (buf && fread(buf, PACKET_BITS, (size_t)*npackets, f) != (size_t)*npackets) {
        free(buf);
        buf = NULL;
    }
    fclose(f);
    return buf;
}

static int fail(int err) {
    fprintf(stderr, "qpsk: %s\n", qpsk_strerror(err));
    return 3;
}

/* names[c] is channel c's output file; with QPSK_OUT_INTERLEAVED in fmt,
 * names[0] is the trunk's */
static int run(int nch, char **paths, char **names, int gap, int host, int fmt, int all) {
    int npk = -1;
    uint8_t **ch = calloc((size_t)nch, sizeof(uint8_t *));
    int *have = calloc((size_t)nch, sizeof(int));
    if (!ch || !have) return 1;
    for (int c = 0; c < nch; c++) {
        ch[c] = read_packets(paths[c], &have[c]);
        if (!ch[c]) {
            fprintf(stderr, "cannot read %s\n", paths[c]);
            return 1;
        }
        if (npk < 0 || (all ? have[c] > npk : have[c] < npk)) npk = have[c];
    }
    if (npk <= 0) return 1;
    const long n = (long)npk * (TX_PACKET + (long)gap);
    const int trunk = (fmt & QPSK_OUT_INTERLEAVED) != 0;
    const long ld = trunk ? nch : n;
    const size_t es = (fmt & 0x0f) == QPSK_OUT_S16 ? sizeof(int16_t) : 1;
    uint8_t *bits = calloc((size_t)nch * npk, PACKET_BITS);
    uint8_t *out = malloc(es * (size_t)nch * (size_t)n);
    /* -a: slot k of channel c is active while its file lasts; the rows of idle slots are not read */
    uint8_t *active = all ? calloc((size_t)nch, (size_t)npk) : NULL;
    if (!bits || !out || (all && !active)) return 1;
    for (int c = 0; c < nch; c++) {
        const int mine = have[c] < npk ? have[c] : npk;
        memcpy(bits + (size_t)c * npk * PACKET_BITS, ch[c], (size_t)mine * PACKET_BITS);
        if (all) memset(active + (size_t)c * npk, 1, (size_t)mine);
    }
    int err = QPSK_OK;
    if (host) {
        qpsk_tx_state *st = malloc(sizeof(qpsk_tx_state) * (size_t)nch);
        int16_t *lin = malloc(sizeof(int16_t) * (size_t)nch * (size_t)n);
        if (!st || !lin) return 1;
        for (int c = 0; c < nch; c++) qpsk_tx_state_init(&st[c]);
        err = qpsk_tx_batch_masked_host(st, nch, bits, active, npk, gap, lin, n, 4);
        if (!err) err = qpsk_output_convert_host(fmt, lin, n, nch, n, out, ld, 4);
        free(lin);
        free(st);
    } else {
        qpsk_tx_ctx *ctx = qpsk_tx_create(0, nch, gap, &err);
        if (!ctx) return fail(err);
        err = qpsk_tx_batch_masked_fmt(ctx, bits, active, npk, out, fmt, ld);
        qpsk_tx_destroy(ctx);
    }
    if (err) return fail(err);
    for (int c = 0; c < (trunk ? 1 : nch); c++) {
        FILE *fo = fopen(names[c], "wb");
        if (!fo) return 1;
        const size_t count = trunk ? (size_t)nch * (size_t)n : (size_t)n;
        const int bad = fwrite(out + es * (size_t)c * (size_t)n, es, count, fo) != count;
        if (fclose(fo) || bad) return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    int gap = 903, host = 0, batch = 0, all = 0, fmt = QPSK_OUT_S16, i = 1;
    for (; i < argc && argv[i][0] == '-' && argv[i][1] != 'o'; i++) {
        if (!strcmp(argv[i], "-b")) batch = 1;
        else if (!strcmp(argv[i], "-c")) host = 1;
        else if (!strcmp(argv[i], "-a")) all = 1;
        else if (!strcmp(argv[i], "-i")) fmt |= QPSK_OUT_INTERLEAVED;
        else if (!strcmp(argv[i], "-g") && i + 1 < argc) gap = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-f") && i + 1 < argc) {
            const char *v = argv[++i];
            const int enc = !strcmp(v, "s16") ? QPSK_OUT_S16 : !strcmp(v, "alaw") ? QPSK_OUT_ALAW :
                            !strcmp(v, "ulaw") ? QPSK_OUT_ULAW : -1;
            if (enc < 0) break;
            fmt = (fmt & QPSK_OUT_INTERLEAVED) | enc;
        } else break;
    }
    const int trunk = (fmt & QPSK_OUT_INTERLEAVED) != 0;
    if (!batch && !trunk && argc - i == 2) {
        char *name = argv[i + 1];
        return run(1, argv + i, &name, gap, host, fmt, 0);
    }
    if (batch && argc - i >= 3 && !strcmp(argv[argc - 2], "-o")) {
        const int nch = argc - 2 - i;
        if (trunk) return run(nch, argv + i, &argv[argc - 1], gap, host, fmt, all);
        char **names = calloc((size_t)nch, sizeof(char *));
        for (int c = 0; names && c < nch; c++) {
            names[c] = malloc(strlen(argv[argc - 1]) + 32);
            if (!names[c]) return 1;
            sprintf(names[c], "%s%d.raw", argv[argc - 1], c);
        }
        return names ? run(nch, argv + i, names, gap, host, fmt, all) : 1;
    }
    fprintf(stderr, "usage: %s [-c] [-g GAP] [-f s16|alaw|ulaw] in.bits out.raw\n"
                    "       %s -b [-a] [-c] [-g GAP] [-f s16|alaw|ulaw] in1.bits [in2.bits ...] -o PREFIX\n"
                    "       %s -b -i [-a] [-c] [-g GAP] [-f s16|alaw|ulaw] in1.bits [in2.bits ...] -o TRUNK\n",
            argv[0], argv[0], argv[0]);
    return 2;
}
