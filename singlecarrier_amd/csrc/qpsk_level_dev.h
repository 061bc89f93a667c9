// qpsk_level_dev.h -- the level accumulator of the device units that meter
// int16 samples: qpsk_level.hip's level_kernel, and the conversion kernels of
// qpsk_input.hip that take the level while the samples are in registers.  A
// level as it is stored, the accumulator of a lane, the two samples of a dword,
// and the reduction over a wave.  Integer arithmetic throughout, so the order
// of any reduction does not matter.  The kernels stay in their units; nothing
// here is one.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qpsk_level.h"

namespace qlevel {

constexpr int kWave = 64;

// a level as it is stored: two 8-byte words at the array's 8-byte alignment
struct alignas(8) LevelWords {
    unsigned long long sumsq, rest;   // rest: sum | peak << 32 | clipped << 48
};
static_assert(sizeof(LevelWords) == sizeof(qpsk_frame_level), "level layout");

struct Acc {
    unsigned long long sumsq = 0;
    int sum = 0;
    unsigned peak = 0, clipped = 0;
};

// the two samples of a word
__device__ __forceinline__ void take2(Acc& a, int w) {
    const int lo = (int)(short)(w & 0xffff), hi = w >> 16;
    const unsigned alo = (unsigned)(lo < 0 ? -lo : lo), ahi = (unsigned)(hi < 0 ? -hi : hi);
    a.sumsq += alo * alo + ahi * ahi;   // <= 2^31: an unsigned word holds the pair
    a.sum += lo + hi;
    a.peak = max(a.peak, max(alo, ahi));
    // v ^ (v >> 31) is v for v >= 0 and -v - 1 below: 32767 at either rail
    a.clipped += (unsigned)((lo ^ (lo >> 31)) == 32767) + (unsigned)((hi ^ (hi >> 31)) == 32767);
}

// b into a
__device__ __forceinline__ void merge(Acc& a, const Acc& b) {
    a.sumsq += b.sumsq;
    a.sum += b.sum;
    a.peak = max(a.peak, b.peak);
    a.clipped += b.clipped;
}

// every lane's a becomes the wave's (all 64 lanes take part).  level_kernel
// keeps this loop and pack() written out in its own body: called from here the
// compiler orders the operands of its 64-bit adds the other way round, and the
// kernel is to stay, instruction for instruction, the one that was measured
// (profiles/meter_fused_disasm.txt).
__device__ __forceinline__ void wave_reduce(Acc& a) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        a.sumsq += __shfl_xor(a.sumsq, d, kWave);
        a.sum += __shfl_xor(a.sum, d, kWave);
        a.peak = max(a.peak, (unsigned)__shfl_xor(a.peak, d, kWave));
        a.clipped += __shfl_xor(a.clipped, d, kWave);
    }
}

__device__ __forceinline__ LevelWords pack(const Acc& a) {
    return LevelWords{a.sumsq, (unsigned long long)(unsigned)a.sum | (unsigned long long)a.peak << 32 |
                                   (unsigned long long)a.clipped << 48};
}

__device__ __forceinline__ Acc unpack(const LevelWords& w) {
    Acc a;
    a.sumsq = w.sumsq;
    a.sum = (int)(unsigned)w.rest;
    a.peak = (unsigned)(w.rest >> 32) & 0xffffu;
    a.clipped = (unsigned)(w.rest >> 48);
    return a;
}

}  // namespace qlevel
