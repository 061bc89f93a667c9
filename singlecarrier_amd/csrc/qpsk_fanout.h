/* qpsk_fanout.h -- the host generators' fan-out over channels (qpsk_synth.c,
 * qpsk_tx_host.c); internal to the library.  A static function in a header:
 * each of the two files stays one self-contained source, as the stand-alone
 * builds of the tests and the callers take them. */
#pragma once

#include <pthread.h>
#include <stdlib.h>

typedef void (*qpsk_share_fn)(void *arg, int lo, int hi);

typedef struct {
    qpsk_share_fn fn;
    void *arg;
    int lo, hi;
} qpsk_share_t;

static void *qpsk_share_run(void *p) {
    qpsk_share_t *s = (qpsk_share_t *)p;
    s->fn(s->arg, s->lo, s->hi);
    return NULL;
}

/* fn(arg, lo, hi) over [0, n) in up to nthreads contiguous shares, one thread
 * each; the last share, and any whose thread did not start, run in the
 * caller.  Returns 0 when every share has run, -1 when the bookkeeping could
 * not be allocated (then none has). */
static int qpsk_fanout(int n, int nthreads, qpsk_share_fn fn, void *arg) {
    if (n < 1) return 0;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > n) nthreads = n;
    qpsk_share_t *sh = (qpsk_share_t *)calloc((size_t)nthreads, sizeof(qpsk_share_t));
    pthread_t *th = (pthread_t *)calloc((size_t)nthreads, sizeof(pthread_t));
    if (!sh || !th) {
        free(sh);
        free(th);
        return -1;
    }
    for (int t = 0; t < nthreads; t++)
        sh[t] = (qpsk_share_t){fn, arg, (int)((long)n * t / nthreads), (int)((long)n * (t + 1) / nthreads)};
    int started = 0;
    while (started < nthreads - 1 && pthread_create(&th[started], NULL, qpsk_share_run, &sh[started]) == 0)
        started++;
    for (int t = started; t < nthreads; t++) qpsk_share_run(&sh[t]);
    for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
    free(sh);
    free(th);
    return 0;
}
