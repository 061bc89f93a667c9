// qpsk_fft.hip -- batched GPU kiss_fft (include/qpsk_fft.h): one wave per
// transform, the points in LDS, the reference's stages (qpsk_fft_dev.h).
#include <hip/hip_runtime.h>

#include <new>
#include <stdint.h>
#include <stdlib.h>

#include "qpsk_fft.h"
#include "qpsk_fft_dev.h"
#include "qpsk_fft_tables.h"
#include "qpsk_hip_host.h"

namespace {

// in [batch][N] -> out [batch][N]; a copy through LDS first, so in may be out
__global__ void __launch_bounds__(64) fft_kernel(const qfft::cf* in, qfft::cf* out, const int* perm,
                                                 const qfft::cf* tw, int N, int inverse) {
    extern __shared__ qfft::cf buf[];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    for (int pos = lane; pos < N; pos += 64) buf[pos] = in[b * N + perm[pos]];   // kf_work leaves
    qfft::lds_sync();
    qfft::stages(lane, N, buf, tw, inverse != 0);
    for (int pos = lane; pos < N; pos += 64) out[b * N + pos] = buf[pos];
}

}  // namespace

struct qpsk_fft_plan {
    int device = 0, nfft = 0, inverse = 0;
    qhip::Stream stream;           // first: released last
    qhip::DevBuf<int> d_perm;
    qhip::DevBuf<qfft::cf> d_tw;
    qhip::DevBuf<qfft::cf> s_buf;   // staging of the host entry point
};

extern "C" qpsk_fft_plan* qpsk_fft_alloc(int device, int nfft, int inverse, int* err) {
    if (nfft < 4 || nfft > 4096 || (nfft & (nfft - 1)) != 0) return qhip::fail(err, QPSK_EINVAL);
    if (!qhip::device_ok(device)) return qhip::fail(err, QPSK_ENODEV);
    qpsk_fft_plan* p = new (std::nothrow) qpsk_fft_plan();
    int* perm = (int*)malloc(sizeof(int) * nfft);
    float* tw = (float*)malloc(sizeof(float) * 2 * nfft);
    if (!p || !perm || !tw) {
        delete p;
        free(perm);
        free(tw);
        return qhip::fail(err, QPSK_ENOMEM);
    }
    p->device = device;
    p->nfft = nfft;
    p->inverse = inverse != 0;
    qpsk_fft_perm_table(nfft, perm);
    qpsk_fft_twiddle_table(nfft, p->inverse, tw);
    int r = herr(hipSetDevice(device));
    if (r == QPSK_OK) r = herr(p->stream.create());
    if (r == QPSK_OK) r = herr(p->d_perm.reserve(nfft));
    if (r == QPSK_OK) r = herr(p->d_tw.reserve(nfft));
    if (r == QPSK_OK) r = herr(hipMemcpy(p->d_perm, perm, sizeof(int) * nfft, hipMemcpyHostToDevice));
    if (r == QPSK_OK) r = herr(hipMemcpy(p->d_tw, tw, sizeof(qfft::cf) * nfft, hipMemcpyHostToDevice));
    free(perm);
    free(tw);
    if (r != QPSK_OK) {
        delete p;
        return qhip::fail(err, r);
    }
    qhip::set_err(err, QPSK_OK);
    return p;
}

extern "C" void qpsk_fft_free(qpsk_fft_plan* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);
    delete p;
}

extern "C" int qpsk_fft_device(qpsk_fft_plan* p, const float* d_in, float* d_out, int batch,
                               void* stream) {
    if (!p || batch < 0 || (batch > 0 && (!d_in || !d_out))) return QPSK_EINVAL;
    if (batch == 0) return QPSK_OK;
    // the kernel loads and stores whole complex values (qfft::cf, 8 bytes)
    if (((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & (sizeof(qfft::cf) - 1)) != 0)
        return QPSK_EINVAL;
    HCHECK(hipSetDevice(p->device));
    hipLaunchKernelGGL(fft_kernel, dim3(batch), dim3(64), sizeof(qfft::cf) * p->nfft,
                       (hipStream_t)stream, reinterpret_cast<const qfft::cf*>(d_in),
                       reinterpret_cast<qfft::cf*>(d_out), p->d_perm, p->d_tw, p->nfft, p->inverse);
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

extern "C" int qpsk_fft(qpsk_fft_plan* p, const float* in, float* out, int batch) {
    if (!p || batch < 0 || (batch > 0 && (!in || !out))) return QPSK_EINVAL;
    if (batch == 0) return QPSK_OK;
    HCHECK(hipSetDevice(p->device));
    const size_t n = (size_t)batch * p->nfft;
    HCHECK(p->s_buf.reserve(n));   // growing: the release waits for the stream's earlier work
    HCHECK(hipMemcpyAsync(p->s_buf, in, sizeof(qfft::cf) * n, hipMemcpyHostToDevice, p->stream));
    int r = qpsk_fft_device(p, reinterpret_cast<const float*>(p->s_buf.get()),
                            reinterpret_cast<float*>(p->s_buf.get()), batch, p->stream);
    if (r != QPSK_OK) return r;
    HCHECK(hipMemcpyAsync(out, p->s_buf, sizeof(qfft::cf) * n, hipMemcpyDeviceToHost, p->stream));
    HCHECK(hipStreamSynchronize(p->stream));
    return QPSK_OK;
}
