// spin_delay.hip -- TEST ONLY: a bounded delay on a stream (tests/gpu_delay.py,
// tests/test_gpu_async.py).  One wave waits until the device's wall clock has
// advanced by a number of ticks.  wall_clock64() is the constant-rate counter
// (hipDeviceAttributeWallClockRate, 100 MHz here), not the shader clock, which
// moves with the device's power state: a delay sized in shader cycles from one
// calibration comes out short whenever the clock is faster than it was then.
// The loop also ends after `cap` iterations, so the kernel cannot run unbounded
// whatever the counter does.
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ void spin_delay_kernel(long long ticks, long long cap) {
    const long long t0 = wall_clock64();
    for (long long i = 0; i < cap && wall_clock64() - t0 < ticks; i++)
        __builtin_amdgcn_s_sleep(32);   // 32 x 64 cycles: about 1 us an iteration
}

// the wall clock's rate in kHz (< 0: a HIP error, negated)
extern "C" long long spin_delay_clock_khz(int device) {
    int khz = 0;
    const hipError_t e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device);
    return e == hipSuccess ? (long long)khz : -(long long)e;
}

// one wave on `stream` (a hipStream_t) that ends after `ticks` of the wall
// clock or `cap` iterations, whichever comes first; 0, or the HIP error
extern "C" int spin_delay(void* stream, long long ticks, long long cap) {
    if (ticks < 0 || cap < 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spin_delay_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ticks, cap);
    return (int)hipGetLastError();
}
