// qpsk_input.hip -- qpsk_input_convert_device (include/qpsk_input.h): G.711
// codes and timeslot-interleaved blocks to the receive path's int16
// [nch][nframes][1880], on the GPU.  Two kernels, both bound by memory:
//
//   planar_kernel       [nch][T] codes -> [nch][T] int16, a flat pass: a lane
//                       takes 16 codes and stores 2 x 16 bytes.  Groups follow
//                       the output, which is 16-byte aligned, so every store is;
//                       a source at any byte address is read as the two aligned
//                       16-byte words around a group, shifted by the call's one
//                       byte offset.  The groups whose aligned words would reach
//                       outside the block (the first, the last ones) and the
//                       tail go per element.
//   interleaved_kernel  src[t * ld + c] -> [nch][T]: a tile of 64 channels x 128
//                       samples through LDS.  Global loads run along the channel
//                       axis, W bytes a lane (W chosen per call from the
//                       alignment of the source and of ld); the tile is kept as
//                       it was read, rows of 64 elements padded by one dword.
//                       Then a lane gathers 8 samples of one channel down the
//                       rows, decodes, and stores 16 bytes along time: a wave
//                       stores 128-byte runs of 8 channels.  LDS banking of both
//                       sides: DESIGN.md (f2).
//
// qpsk_input_convert_level_device is the same conversion with the level meter
// (include/qpsk_level.h) in its pass, on the samples a lane has in registers:
// interleaved_kernel with one more argument, which keeps a level per lane in
// LDS, folds them per channel and tile part and stores partial levels that
// fold_kernel, a second launch, sums per frame; and planar_level_kernel, a
// wave a frame, which needs no partials.  The kernels without the level are
// the code they were (profiles/meter_fused_disasm.txt).
//
// G.711 is decoded either with the integer expansion (qpsk_fmt.h) or
// through a 256-entry table in LDS that each block makes with it;
// qpsk_input_convert_device_dec names one, profiles/input_bench.py times both,
// and the default is the faster of each kernel (qpsk_fmt_internal.h).
// What the kernels share with the output's is qpsk_fmt_dev.h.
// The format entry points of the receive path and of the streams are here
// too, on the hooks of qpsk_rx_internal.h: the receive and stream units refer
// to nothing of this file.
// Not part of the receive kernels' hash (csrc/Makefile KSRC: the kernel unit's
// sources and compile command, not the list of objects).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qpsk_consts.h"
#include "qpsk_fmt_dev.h"
#include "qpsk_herr.h"
#include "qpsk_level.h"
#include "qpsk_level_dev.h"
#include "qpsk_rx_internal.h"
#include "qpsk_rx_plan.h"
#include "qpsk_stream.h"

namespace {

using namespace qfmt;
using namespace qlevel;   // LevelWords, Acc, take2, merge, wave_reduce, pack, unpack

// the block's decode table (QPSK_IN_DEC_TABLE), ready after the next __syncthreads()
template <int ENC, int DEC>
__device__ __forceinline__ void fill_table(int16_t* tab) {
    if constexpr (ENC != QPSK_IN_S16 && DEC == QPSK_IN_DEC_TABLE) {
        if (threadIdx.x < 256)
            tab[threadIdx.x] = (int16_t)(ENC == QPSK_IN_ALAW ? qpsk_alaw_decode(threadIdx.x)
                                                             : qpsk_ulaw_decode(threadIdx.x));
    }
}

// 16 codes in 4 dwords -> 16 int16 in 2 x int4
template <int ENC, int DEC>
__device__ __forceinline__ void decode16(const unsigned d[4], const int16_t* tab, int16_t* o) {
    unsigned p[8];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        p[2 * j] = decode<ENC, DEC>(d[j] & 0xffu, tab) | decode<ENC, DEC>((d[j] >> 8) & 0xffu, tab) << 16;
        p[2 * j + 1] = decode<ENC, DEC>((d[j] >> 16) & 0xffu, tab) | decode<ENC, DEC>(d[j] >> 24, tab) << 16;
    }
    uint4* o4 = reinterpret_cast<uint4*>(o);
    o4[0] = make_uint4(p[0], p[1], p[2], p[3]);
    o4[1] = make_uint4(p[4], p[5], p[6], p[7]);
}

template <int ENC, int DEC>
__global__ __launch_bounds__(kBlock) void planar_kernel(const uint8_t* __restrict__ src,
                                                        int16_t* __restrict__ out, size_t n) {
    __shared__ int16_t tab[256];
    fill_table<ENC, DEC>(tab);
    __syncthreads();
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u);   // the call's byte offset
    const uint4* words = reinterpret_cast<const uint4*>(src - a);
    const size_t ngroups = (n + 15) / 16;
    for (size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * kBlock) {
        const size_t e0 = g * 16;
        // word g holds source bytes [e0 - a, e0 - a + 16), word g + 1 the next 16
        const bool wide = e0 + 16 <= n && (a == 0 || (g > 0 && e0 + 32 - a <= n));
        if (wide) {
            const uint4 lo = words[g];
            const uint4 hi = a ? words[g + 1] : make_uint4(0, 0, 0, 0);
            const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            unsigned d[4];
            switch (a >> 2) {   // the same in every lane
                case 0: shifted<0, 4>(w, a & 3u, d); break;
                case 1: shifted<1, 4>(w, a & 3u, d); break;
                case 2: shifted<2, 4>(w, a & 3u, d); break;
                default: shifted<3, 4>(w, a & 3u, d); break;
            }
            decode16<ENC, DEC>(d, tab, out + e0);
        } else {
            for (size_t e = e0; e < e0 + 16 && e < n; e++) out[e] = (int16_t)decode<ENC, DEC>(src[e], tab);
        }
    }
}

// the level of a lane's 8 samples as the tile keeps it in LDS: one 16-byte word
__device__ __forceinline__ uint4 lds_pack(const Acc& a) {
    return make_uint4((unsigned)a.sumsq, (unsigned)(a.sumsq >> 32), (unsigned)a.sum, a.peak | a.clipped << 16);
}

__device__ __forceinline__ Acc lds_unpack(const uint4& w) {
    Acc a;
    a.sumsq = (unsigned long long)w.x | (unsigned long long)w.y << 32;
    a.sum = (int)w.z;
    a.peak = w.w & 0xffffu;
    a.clipped = w.w >> 16;
    return a;
}

// lv[tq][c] of a tile with levels; a tile without them has no such array
template <bool LVL> struct TileLevels {
    static __device__ __forceinline__ uint4* get() { return nullptr; }
};
template <> struct TileLevels<true> {
    static __device__ __forceinline__ uint4* get() {
        __shared__ __attribute__((aligned(16))) uint4 lv[(kTT / 8) * kTC];
        return lv;
    }
};

// interleaved_kernel with one more argument, LevelWords* part (LVL): the
// store phase also takes the level of each lane's 8 samples (a group of 8 lies
// inside one frame: 1880 = 8 * 235) into lv[tq][c]; behind the tile's last
// barrier two waves fold them per channel, one for the part of the tile in
// front of the frame boundary it holds and one for the part behind it (at most
// one boundary in 128 samples, at a multiple of 8), and store the two partial
// levels to part[frame][tile of the frame][channel].  The accumulators start
// anew with every tile of the grid-stride loop.  LDS: ds_write_b128 goes by
// groups of 8 lanes, which here write the 128 contiguous bytes of 8 channels,
// and the fold reads 16 bytes a lane along the channels: both free of conflicts.
template <int ENC, int W, int DEC, class... Part>
__global__ __launch_bounds__(kBlock) void interleaved_kernel(const uint8_t* __restrict__ src, size_t ld,
                                                             unsigned nch, size_t T,
                                                             int16_t* __restrict__ out, unsigned ctiles,
                                                             size_t ntiles, Part... part_arg) {
    constexpr bool LVL = sizeof...(Part) != 0;   // one more argument: LevelWords* part
    constexpr int ES = ENC == QPSK_IN_S16 ? 2 : 1;   // bytes of an element
    constexpr int RS = kTC * ES + 4;                 // bytes of a tile row in LDS: one dword of padding
    constexpr int LPR = kTC * ES / W;                // lanes that load a row
    constexpr int RPP = kBlock / LPR;                // rows per pass of the block
    constexpr int NP = kTT / RPP;                    // passes
    constexpr int V = W / ES;                        // elements of a lane's load
    constexpr int DW = W >= 4 ? W / 4 : 1;
    static_assert(W >= ES && LPR >= 1 && RPP <= kTT && NP * RPP == kTT, "tile shape");
    __shared__ __attribute__((aligned(16))) uint8_t raw[kTT * RS];
    __shared__ int16_t tab[256];
    uint4* const lv = TileLevels<LVL>::get();
    fill_table<ENC, DEC>(tab);
    const unsigned k = threadIdx.x % LPR, r0 = threadIdx.x / LPR;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned c0 = (unsigned)(tile % ctiles) * kTC;
        const size_t t0 = (tile / ctiles) * kTT;
        // rows of the source into registers, then into the tile as they are
        const unsigned cl = c0 + k * V;   // the first channel of this lane's loads
        unsigned v[NP][DW];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const size_t t = t0 + r0 + p * RPP;
#pragma unroll
            for (int j = 0; j < DW; j++) v[p][j] = 0;
            if (t < T && cl < nch) {
                const uint8_t* row = src + (t * ld + cl) * ES;
                if (cl + V <= nch) {
                    load_wide<W>(row, v[p]);
                } else {   // the tile's last channels: only those there are
#pragma unroll
                    for (int j = 0; j < V; j++)
                        if (cl + j < nch) {
                            const unsigned x = ES == 1 ? row[j] : reinterpret_cast<const uint16_t*>(row)[j];
                            v[p][(j * ES) / 4] |= x << (8 * ((j * ES) % 4));
                        }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const unsigned b = (r0 + p * RPP) * RS + k * W;
            if constexpr (W >= 4) {
#pragma unroll
                for (int j = 0; j < DW; j++) reinterpret_cast<unsigned*>(raw)[b / 4 + j] = v[p][j];
            } else if constexpr (W == 2) {
                *reinterpret_cast<uint16_t*>(raw + b) = (uint16_t)v[p][0];
            } else {
                raw[b] = (uint8_t)v[p][0];
            }
        }
        __syncthreads();
        // a lane: 8 samples of one channel down the rows -> 16 bytes along time
#pragma unroll
        for (int it = 0; it < kTC * (kTT / 8) / kBlock; it++) {
            const unsigned s = threadIdx.x + it * kBlock;
            const unsigned c = (s % 8) + 8 * (s / 128), tq = (s / 8) % (kTT / 8);
            const size_t t = t0 + tq * 8;
            if (c0 + c < nch && t < T) {   // T is a multiple of 8: all 8 samples or none
                unsigned x[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const unsigned b = (tq * 8 + i) * RS + c * ES;
                    const unsigned code = ES == 1 ? raw[b] : *reinterpret_cast<const uint16_t*>(raw + b);
                    x[i] = decode<ENC, DEC>(code, tab);
                }
                const uint4 o = make_uint4(x[0] | x[1] << 16, x[2] | x[3] << 16, x[4] | x[5] << 16, x[6] | x[7] << 16);
                *reinterpret_cast<uint4*>(out + (size_t)(c0 + c) * T + t) = o;
                if constexpr (LVL) {
                    Acc a;
                    take2(a, (int)o.x);
                    take2(a, (int)o.y);
                    take2(a, (int)o.z);
                    take2(a, (int)o.w);
                    lv[tq * kTC + c] = lds_pack(a);
                }
            } else if constexpr (LVL) {
                lv[tq * kTC + c] = make_uint4(0, 0, 0, 0);   // nothing there: adds nothing to any field
            }
        }
        __syncthreads();   // the tile is rewritten by the next round
        if constexpr (LVL) {
            // (lv is written again only behind the next tile's first barrier)
            if (threadIdx.x < 2 * kTC) {
                const unsigned c = threadIdx.x % kTC, behind = threadIdx.x / kTC;   // a wave each
                const size_t f0 = t0 / QK_FRAME, edge = (f0 + 1) * QK_FRAME;        // the frame of the tile's first sample
                const unsigned b = edge - t0 < (size_t)kTT ? (unsigned)(edge - t0) / 8 : kTT / 8;
                const unsigned lo = behind ? b : 0, hi = behind ? kTT / 8 : b;
                if (c0 + c < nch && lo < hi && t0 + lo * 8 < T) {
                    Acc a;
                    for (unsigned tq = lo; tq < hi; tq++) merge(a, lds_unpack(lv[tq * kTC + c]));
                    const size_t f = f0 + behind, first = f * QK_FRAME / kTT;   // the first tile of frame f
                    LevelWords* const part = (part_arg, ...);
                    part[((f * QPSK_IN_LEVEL_FRAME_TILES + (t0 / kTT - first)) * nch) + c0 + c] = pack(a);
                }
            }
        }
    }
}

// The partial levels of frame f of channel c, part[f][k][c] for the k tiles
// the frame has samples in, into level[c][f]: one plain 16-byte store each.
__global__ __launch_bounds__(kBlock) void fold_kernel(const LevelWords* __restrict__ part, unsigned nch, unsigned F,
                                                      LevelWords* __restrict__ level) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;   // < nch * F < 2^28
    if (i >= (size_t)nch * F) return;
    const size_t f = i / nch, c = i % nch;
    const unsigned n = (unsigned)(((f + 1) * QK_FRAME - 1) / kTT - f * QK_FRAME / kTT) + 1;   // 15 or 16
    Acc a;
    for (unsigned k = 0; k < n; k++) merge(a, unpack(part[(f * QPSK_IN_LEVEL_FRAME_TILES + k) * nch + c]));
    level[c * F + f] = pack(a);
}

// Planar G.711 with the level: a wave takes one frame (row) of 1880 codes as
// level_kernel (qpsk_level.hip) takes one of samples.  A lane takes 8 codes,
// 235 groups a row in 4 passes, all loads in flight before the first is used,
// and stores 16 bytes; a wave reads 512 and writes 1024 contiguous bytes a
// pass.  A row is 1880 = 8 * 235 bytes, so every row has the source's byte
// offset in an 8-byte word: a group is the two aligned words around it,
// shifted.  The first group of the block and the last one, whose aligned words
// would reach outside it, go per element.  Then the wave reduces, and lane 0
// stores the row's level at once: no partials, no second launch.
constexpr int kRowVec = QK_FRAME / 8;                       // 235 groups a row
constexpr int kRowLoads = (kRowVec + kWave - 1) / kWave;   // 4 a lane
constexpr int kRows = kBlock / kWave;                       // rows of a block at a time
static_assert(QK_FRAME % 8 == 0 && QPSK_IN_LEVEL_FRAME_TILES * kTT >= QK_FRAME + kTT - 8, "frames and tiles");

template <int ENC, int DEC>
__global__ __launch_bounds__(kBlock) void planar_level_kernel(const uint8_t* __restrict__ src,
                                                              int16_t* __restrict__ out, size_t nrows,
                                                              LevelWords* __restrict__ level) {
    __shared__ int16_t tab[256];
    fill_table<ENC, DEC>(tab);
    __syncthreads();
    const unsigned lane = threadIdx.x % kWave;
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(src) & 7u);   // the call's byte offset, every row's
    const unsigned r = a & 3u;
    // (whole waves leave the loop: no shuffle below has a lane missing)
    for (size_t row = (size_t)blockIdx.x * kRows + threadIdx.x / kWave; row < nrows; row += (size_t)gridDim.x * kRows) {
        const uint8_t* p = src + row * QK_FRAME;
        const uint2* words = reinterpret_cast<const uint2*>(p - a);
        unsigned d[kRowLoads][2];
#pragma unroll
        for (int k = 0; k < kRowLoads; k++) {
            const unsigned j = k * kWave + lane;
            d[k][0] = d[k][1] = 0;
            if (j >= (unsigned)kRowVec) continue;
            // word j holds the row's bytes [8j - a, 8j - a + 8), word j + 1 the next 8
            const bool outside = a != 0 && ((row == 0 && j == 0) || (row == nrows - 1 && j == (unsigned)kRowVec - 1));
            if (!outside) {
                const uint2 lo = words[j];
                const uint2 hi = a ? words[j + 1] : make_uint2(0, 0);
                if (a < 4) {
                    d[k][0] = __builtin_amdgcn_alignbyte(lo.y, lo.x, r);
                    d[k][1] = __builtin_amdgcn_alignbyte(hi.x, lo.y, r);
                } else {
                    d[k][0] = __builtin_amdgcn_alignbyte(hi.x, lo.y, r);
                    d[k][1] = __builtin_amdgcn_alignbyte(hi.y, hi.x, r);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) d[k][i / 4] |= (unsigned)p[8 * j + i] << (8 * (i % 4));
            }
        }
        Acc acc;
#pragma unroll
        for (int k = 0; k < kRowLoads; k++) {
            const unsigned j = k * kWave + lane;
            if (j >= (unsigned)kRowVec) continue;   // (a code of zeros is not a sample of zero)
            unsigned x[4];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                x[2 * q] = decode<ENC, DEC>(d[k][q] & 0xffu, tab) | decode<ENC, DEC>((d[k][q] >> 8) & 0xffu, tab) << 16;
                x[2 * q + 1] = decode<ENC, DEC>((d[k][q] >> 16) & 0xffu, tab) | decode<ENC, DEC>(d[k][q] >> 24, tab) << 16;
            }
            *reinterpret_cast<uint4*>(out + row * QK_FRAME + 8 * (size_t)j) = make_uint4(x[0], x[1], x[2], x[3]);
            take2(acc, (int)x[0]);
            take2(acc, (int)x[1]);
            take2(acc, (int)x[2]);
            take2(acc, (int)x[3]);
        }
        wave_reduce(acc);
        if (lane == 0) level[row] = pack(acc);
    }
}

template <int ENC, int DEC>
void launch_planar(const uint8_t* src, int16_t* out, size_t n, hipStream_t s) {
    const size_t groups = (n + 15) / 16;
    hipLaunchKernelGGL((planar_kernel<ENC, DEC>), dim3(grid_of((groups + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       src, out, n);
}

template <int ENC, int W, int DEC>
void launch_tile(const uint8_t* src, size_t ld, unsigned nch, size_t T, int16_t* out, hipStream_t s) {
    const unsigned ctiles = (nch + kTC - 1) / kTC;
    const size_t ntiles = (size_t)ctiles * ((T + kTT - 1) / kTT);
    hipLaunchKernelGGL((interleaved_kernel<ENC, W, DEC>), dim3(grid_of(ntiles)), dim3(kBlock), 0, s, src, ld, nch, T,
                       out, ctiles, ntiles);
}

// f(Const<enc>, Const<dec>): int16 has no decoder, so only its QPSK_IN_DEC_ARITH kernels exist
template <class F>
void with_decoder(int enc, bool table, F&& f) {
    with_encoding(enc, [&](auto e) {
        if constexpr (e() != QPSK_IN_S16) {
            if (table) return f(e, Const<QPSK_IN_DEC_TABLE>{});
        }
        f(e, Const<QPSK_IN_DEC_ARITH>{});
    });
}

}  // namespace

extern "C" int qpsk_input_load_width(const void* d_src, long ld, int esize) {
    return fmt_access_width(d_src, ld, esize);
}

extern "C" int qpsk_input_convert_device_dec(int fmt, const void* d_src, long ld, int nch, int nframes,
                                             int16_t* d_out, void* stream, int dec) {
    if (qpsk_input_check(fmt, nch, nframes, ld) != QPSK_OK) return QPSK_EINVAL;
    if (dec == QPSK_IN_DEC_DEFAULT)
        dec = QPSK_FMT_LAYOUT(fmt) == QPSK_IN_PLANAR ? QPSK_IN_DEC_TABLE : QPSK_IN_DEC_ARITH;
    if (dec != QPSK_IN_DEC_ARITH && dec != QPSK_IN_DEC_TABLE) return QPSK_EINVAL;
    if (nframes == 0) return QPSK_OK;
    const int es = qpsk_fmt_esize(fmt), enc = QPSK_FMT_ENC(fmt);
    if (!d_src || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_src) & (uintptr_t)(es - 1)) != 0)
        return QPSK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* src = static_cast<const uint8_t*>(d_src);
    const size_t T = (size_t)nframes * QK_FRAME, n = (size_t)nch * T;
    const bool table = dec == QPSK_IN_DEC_TABLE;
    if (QPSK_FMT_LAYOUT(fmt) == QPSK_IN_PLANAR) {
        if (enc == QPSK_IN_S16) {
            HCHECK(hipMemcpyAsync(d_out, d_src, n * sizeof(int16_t), hipMemcpyDeviceToDevice, s));
            return QPSK_OK;
        }
        with_decoder(enc, table, [&](auto e, auto d) {
            if constexpr (e() != QPSK_IN_S16) launch_planar<e(), d()>(src, d_out, n, s);
        });
    } else {
        const int w = qpsk_input_load_width(d_src, ld, es);
        with_decoder(enc, table, [&](auto e, auto d) {
            with_width<esize_of(e())>(w, [&](auto wc) {
                launch_tile<e(), wc(), d()>(src, (size_t)ld, (unsigned)nch, T, d_out, s);
            });
        });
    }
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

extern "C" int qpsk_input_convert_device(int fmt, const void* d_src, long ld, int nch, int nframes,
                                         int16_t* d_out, void* stream) {
    return qpsk_input_convert_device_dec(fmt, d_src, ld, nch, nframes, d_out, stream, QPSK_IN_DEC_DEFAULT);
}

// ---------------------------------------------------------------- the conversion with the level in its pass
namespace {

template <int ENC, int DEC>
void launch_planar_level(const uint8_t* src, int16_t* out, size_t nrows, LevelWords* level, unsigned cap,
                         hipStream_t s) {
    hipLaunchKernelGGL((planar_level_kernel<ENC, DEC>), dim3(grid_of((nrows + kRows - 1) / kRows, cap)), dim3(kBlock),
                       0, s, src, out, nrows, level);
}

template <int ENC, int W, int DEC>
void launch_tile_level(const uint8_t* src, size_t ld, unsigned nch, size_t T, int16_t* out, LevelWords* part,
                       unsigned cap, hipStream_t s) {
    const unsigned ctiles = (nch + kTC - 1) / kTC;
    const size_t ntiles = (size_t)ctiles * ((T + kTT - 1) / kTT);
    hipLaunchKernelGGL((interleaved_kernel<ENC, W, DEC, LevelWords*>), dim3(grid_of(ntiles, cap)), dim3(kBlock), 0, s, src, ld,
                       nch, T, out, ctiles, ntiles, part);
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int qpsk_input_convert_level_device_grid(int fmt, const void* d_src, long ld, int nch, int nframes,
                                                    int16_t* d_out, qpsk_frame_level* d_level, void* d_work,
                                                    size_t work_bytes, void* stream, int dec, unsigned grid_cap) {
    if (qpsk_input_check(fmt, nch, nframes, ld) != QPSK_OK) return QPSK_EINVAL;
    const bool planar = QPSK_FMT_LAYOUT(fmt) == QPSK_IN_PLANAR;
    if (dec == QPSK_IN_DEC_DEFAULT) dec = planar ? QPSK_IN_DEC_TABLE : QPSK_IN_DEC_ARITH;
    if (dec != QPSK_IN_DEC_ARITH && dec != QPSK_IN_DEC_TABLE) return QPSK_EINVAL;
    if (nframes == 0) return QPSK_OK;
    const int es = qpsk_fmt_esize(fmt), enc = QPSK_FMT_ENC(fmt);
    if (!d_src || !d_out || !aligned_to(d_out, 16) || !aligned_to(d_src, (uintptr_t)es)) return QPSK_EINVAL;
    const size_t need = qpsk_input_level_work(fmt, nch, nframes, ld);
    if (!d_level || !aligned_to(d_level, 8) || !aligned_to(d_work, 16) || work_bytes < need || (need > 0 && !d_work))
        return QPSK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* src = static_cast<const uint8_t*>(d_src);
    const size_t T = (size_t)nframes * QK_FRAME, nrows = (size_t)nch * (size_t)nframes;
    const bool table = dec == QPSK_IN_DEC_TABLE;
    const unsigned cap = grid_cap ? grid_cap : kMaxGrid;
    LevelWords* level = reinterpret_cast<LevelWords*>(d_level);
    if (planar) {
        if (enc == QPSK_IN_S16) {   // no conversion pass: the copy, then the meter's own kernel on what it wrote
            HCHECK(hipMemcpyAsync(d_out, d_src, nrows * QK_FRAME * sizeof(int16_t), hipMemcpyDeviceToDevice, s));
            return qpsk_level_device(d_out, nrows, d_level, s);
        }
        with_decoder(enc, table, [&](auto e, auto d) {
            if constexpr (e() != QPSK_IN_S16) launch_planar_level<e(), d()>(src, d_out, nrows, level, cap, s);
        });
    } else {
        LevelWords* part = static_cast<LevelWords*>(d_work);
        const int w = qpsk_input_load_width(d_src, ld, es);
        with_decoder(enc, table, [&](auto e, auto d) {
            with_width<esize_of(e())>(w, [&](auto wc) {
                launch_tile_level<e(), wc(), d()>(src, (size_t)ld, (unsigned)nch, T, d_out, part, cap, s);
            });
        });
        hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((nrows + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, part,
                           (unsigned)nch, (unsigned)nframes, level);
    }
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

extern "C" int qpsk_input_convert_level_device(int fmt, const void* d_src, long ld, int nch, int nframes,
                                               int16_t* d_out, qpsk_frame_level* d_level, void* d_work,
                                               size_t work_bytes, void* stream) {
    return qpsk_input_convert_level_device_grid(fmt, d_src, ld, nch, nframes, d_out, d_level, d_work, work_bytes,
                                                stream, QPSK_IN_DEC_DEFAULT, 0);
}

// ---------------------------------------------------------------- the receive path behind it
namespace {

struct HostFeed {
    qpsk_ctx* c;
    const void* in;
    int fmt, nch, F;
    long ld;
};

// the source block over PCIe as it is, then converted into the staging block's input
int feed_fmt(void* arg, int16_t* d_in, hipStream_t s) {
    const HostFeed* f = static_cast<const HostFeed*>(arg);
    const size_t nraw = qpsk_input_bytes(f->fmt, f->nch, f->F, f->ld);
    char* raw = nullptr;
    const int r = qpsk_rx_fmt_raw(f->c, nraw, &raw);
    if (r != QPSK_OK) return r;
    HCHECK(hipMemcpyAsync(raw, f->in, nraw, hipMemcpyHostToDevice, s));
    return qpsk_input_convert_device(f->fmt, raw, f->ld, f->nch, f->F, d_in, s);
}

}  // namespace

extern "C" int qpsk_rx_batch_fmt(qpsk_ctx* c, const void* in, int fmt, long ld, int F, uint8_t* bits,
                                 uint8_t* valid, int32_t* trace, float* soft) {
    if (fmt == (QPSK_IN_S16 | QPSK_IN_PLANAR))
        return qpsk_rx_batch(c, static_cast<const int16_t*>(in), F, bits, valid, trace, soft);
    const int nch = qpsk_rx_channels(c);   // 0 for a null context
    if (qpsk_input_check(fmt, nch, F, ld) != QPSK_OK || (F > 0 && !in)) return QPSK_EINVAL;
    HostFeed f{c, in, fmt, nch, F, ld};
    return qpsk_rx_batch_fed(c, feed_fmt, &f, F, bits, valid, trace, soft);
}

extern "C" int qpsk_rx_batch_device_fmt(qpsk_ctx* c, const void* d_in, int fmt, long ld, int F,
                                        uint8_t* d_bits, uint8_t* d_valid, int32_t* d_trace,
                                        float* d_soft, void* stream) {
    if (fmt == (QPSK_IN_S16 | QPSK_IN_PLANAR))
        return qpsk_rx_batch_device(c, static_cast<const int16_t*>(d_in), F, d_bits, d_valid, d_trace, d_soft, stream);
    const int nch = qpsk_rx_channels(c);
    if (qpsk_input_check(fmt, nch, F, ld) != QPSK_OK || (F > 0 && (!d_in || !d_bits || !d_valid)))
        return QPSK_EINVAL;
    // the receive's own refusal of misaligned outputs (qpsk_rx_plan.h), in front of the conversion
    if (F > 0 && !rx_ptrs_aligned(nullptr, d_bits, d_valid, d_trace, d_soft)) return QPSK_EINVAL;
    if (F == 0) return qpsk_rx_batch_device(c, nullptr, 0, d_bits, d_valid, d_trace, d_soft, stream);
    int16_t* conv = nullptr;
    int r = qpsk_rx_fmt_conv(c, (size_t)nch * (size_t)F * QK_FRAME, &conv);
    if (r != QPSK_OK) return r;
    r = qpsk_input_convert_device(fmt, d_in, ld, nch, F, conv, stream);
    if (r != QPSK_OK) return r;
    return qpsk_rx_batch_device(c, conv, F, d_bits, d_valid, d_trace, d_soft, stream);
}

extern "C" qpsk_stream* qpsk_stream_create_fmt(int device, int nch, int frames, int nslot, int mode, int fmt,
                                               int* err) {
    if (fmt == (QPSK_IN_S16 | QPSK_IN_PLANAR)) return qpsk_stream_create_mode(device, nch, frames, nslot, mode, err);
    if (frames < 1 || qpsk_input_check(fmt, nch, frames, nch) != QPSK_OK) {
        if (err) *err = QPSK_EINVAL;
        return nullptr;
    }
    return qpsk_stream_create_raw(device, nch, frames, nslot, mode, fmt, qpsk_input_bytes(fmt, nch, frames, nch),
                                  qpsk_input_convert_device, err);
}
