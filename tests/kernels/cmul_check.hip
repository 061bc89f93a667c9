// cmul_check.hip -- TEST ONLY: the receive kernels' exact complex products
// cmul_g / cmulc_g (qpsk_cmul.h: the inline form plus the Annex G recovery) on
// caller-supplied operands, for comparison with the oracle's qc_cmul.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qpsk_cmul.h"

#pragma clang fp contract(off)

// in [n][4] = (a, b, c, d); out [n][4] = (a+bi)(c+di), (a+bi)conj(c+di)
__global__ void cmul_check_kernel(const float4* in, float4* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 v = in[i];
    const f2 p = cmul_g(f2{v.x, v.y}, f2{v.z, v.w});
    const f2 q = cmulc_g(f2{v.x, v.y}, f2{v.z, v.w});
    out[i] = make_float4(p.x, p.y, q.x, q.y);
}

// returns 0 on success
extern "C" int cmul_check(const float* in, float* out, int n) {
    float4 *d_in = nullptr, *d_out = nullptr;
    const size_t bytes = (size_t)n * sizeof(float4);
    if (n <= 0) return -1;
    if (hipMalloc(&d_in, bytes) != hipSuccess) return -1;
    if (hipMalloc(&d_out, bytes) != hipSuccess) {
        (void)hipFree(d_in);
        return -1;
    }
    int rc = 0;
    if (hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -2;
    if (rc == 0) {
        cmul_check_kernel<<<(n + 255) / 256, 256>>>(d_in, d_out, n);
        if (hipDeviceSynchronize() != hipSuccess) rc = -3;
    }
    if (rc == 0 && hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = -4;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}
