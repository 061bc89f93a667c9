/*
 * qpsk_tx_raw.c -- the reference TX loop (src/qpsk.c:380-413) with the payload
 * read from a file instead of rand(), through the batched transmitter
 * (include/qpsk_tx.h).
 *
 *   qpsk_tx_raw [-g GAP] in.bits out.raw     one channel
 *   qpsk_tx_raw -b [-g GAP] in1.bits [in2.bits ...] -o PREFIX
 *                                            every file is one channel; all channels are
 *                                            modulated together through qpsk_tx_batch()
 *                                            and PREFIX<i>.raw is written per channel
 *   -c    modulate on the host (qpsk_tx_batch_host) instead of the GPU
 *
 * Input: 0/1 bytes, 496 per packet (8 frames of 62 bits, bits[2s] = Q,
 * bits[2s+1] = I: the layout qpsk_rx_raw writes); a short tail is dropped, and
 * -b sends the packets every file has.  Output: the reference's .raw framing,
 * int16 samples at 8 kHz: per packet 640 preamble samples, 8 x 155 data
 * samples, GAP zeros (default 903, as the reference writes).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

/* names[c] is channel c's output file */
static int run(int nch, char **paths, char **names, int gap, int host) {
    int npk = -1;
    uint8_t **ch = calloc((size_t)nch, sizeof(uint8_t *));
    if (!ch) return 1;
    for (int c = 0; c < nch; c++) {
        int n;
        ch[c] = read_packets(paths[c], &n);
        if (!ch[c]) {
            fprintf(stderr, "cannot read %s\n", paths[c]);
            return 1;
        }
        if (npk < 0 || n < npk) npk = n;
    }
    if (npk <= 0) return 1;
    const long ld = (long)npk * (TX_PACKET + (long)gap);
    uint8_t *bits = malloc((size_t)nch * npk * PACKET_BITS);
    int16_t *out = malloc(sizeof(int16_t) * (size_t)nch * (size_t)ld);
    if (!bits || !out) return 1;
    for (int c = 0; c < nch; c++)
        memcpy(bits + (size_t)c * npk * PACKET_BITS, ch[c], (size_t)npk * PACKET_BITS);
    int err = QPSK_OK;
    if (host) {
        qpsk_tx_state *st = malloc(sizeof(qpsk_tx_state) * (size_t)nch);
        if (!st) return 1;
        for (int c = 0; c < nch; c++) qpsk_tx_state_init(&st[c]);
        err = qpsk_tx_batch_host(st, nch, bits, npk, gap, out, ld, 4);
        free(st);
    } else {
        qpsk_tx_ctx *ctx = qpsk_tx_create(0, nch, gap, &err);
        if (!ctx) return fail(err);
        err = qpsk_tx_batch(ctx, bits, npk, out, ld);
        qpsk_tx_destroy(ctx);
    }
    if (err) return fail(err);
    for (int c = 0; c < nch; c++) {
        FILE *fo = fopen(names[c], "wb");
        if (!fo) return 1;
        fwrite(out + (size_t)c * ld, sizeof(int16_t), (size_t)ld, fo);
        fclose(fo);
    }
    return 0;
}

int main(int argc, char **argv) {
    int gap = 903, host = 0, batch = 0, i = 1;
    for (; i < argc && argv[i][0] == '-' && argv[i][1] != 'o'; i++) {
        if (!strcmp(argv[i], "-b")) batch = 1;
        else if (!strcmp(argv[i], "-c")) host = 1;
        else if (!strcmp(argv[i], "-g") && i + 1 < argc) gap = atoi(argv[++i]);
        else break;
    }
    if (!batch && argc - i == 2) {
        char *name = argv[i + 1];
        return run(1, argv + i, &name, gap, host);
    }
    if (batch && argc - i >= 3 && !strcmp(argv[argc - 2], "-o")) {
        const int nch = argc - 2 - i;
        char **names = calloc((size_t)nch, sizeof(char *));
        for (int c = 0; names && c < nch; c++) {
            names[c] = malloc(strlen(argv[argc - 1]) + 32);
            if (!names[c]) return 1;
            sprintf(names[c], "%s%d.raw", argv[argc - 1], c);
        }
        return names ? run(nch, argv + i, names, gap, host) : 1;
    }
    fprintf(stderr, "usage: %s [-c] [-g GAP] in.bits out.raw | -b [-c] [-g GAP] in1.bits [in2.bits ...] -o PREFIX\n",
            argv[0]);
    return 2;
}
