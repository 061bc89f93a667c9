// qpsk_output.hip -- qpsk_output_convert_device (include/qpsk_output.h): the
// transmit path's planar int16 rows to G.711 codes and timeslot-interleaved
// blocks, on the GPU.  The mirror of qpsk_input.hip; two kernels, both bound by
// memory:
//
//   planar_kernel       int16 [nch][src_ld] -> codes [nch][ld], a flat pass per
//                       row: a lane takes 16 samples and stores 16 codes in one
//                       16-byte store.  Groups follow the destination row, so
//                       every wide store is aligned whatever the row's address;
//                       the 32 source bytes of a group are read as the aligned
//                       16-byte words around them (two, or three when the row's
//                       source and destination do not line up) and shifted by
//                       the row's one byte offset.  The groups at a row's head
//                       and tail that do not fill an aligned store, and those
//                       whose aligned source words would reach outside the
//                       row, go per element.  src_ld == n == ld is one flat row.
//   interleaved_kernel  int16 planar -> dst[p * ld + c]: a tile of 64 channels x
//                       128 samples through LDS.  Global loads run along time,
//                       8 samples a lane; the samples are compressed before the
//                       tile is written, so the tile holds bytes for G.711 (and
//                       int16 for QPSK_OUT_S16), rows along time.  Then a lane
//                       gathers W bytes down the channel rows and stores them
//                       along the channel axis, W = 16, 8, 4, 2 or 1 chosen per
//                       call from the alignment of the destination and of ld.
//                       LDS banking of both sides: DESIGN.md (f2).
//
// Every store is inside the block: no wider word that reaches outside it is
// read, modified and written back.
// G.711 is the integer compression of qpsk_fmt.h; what the kernels share with
// the input's is qpsk_fmt_dev.h.
// The format entry points of the transmitter are here too, on the hooks of
// qpsk_tx_internal.h: qpsk_tx.hip refers to nothing of this file.  They run the
// modulator into the context's int16 block and one of the kernels behind it,
// except for planar G.711, which tx_batch_kernel's store pass writes itself
// (the faster of the two as measured: DESIGN.md "Batched transmitter").
// Not part of the receive kernels' hash (csrc/Makefile KSRC: the kernel unit's
// sources and compile command, not the list of objects).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qpsk_consts.h"
#include "qpsk_fmt_dev.h"
#include "qpsk_herr.h"
#include "qpsk_hip_host.h"
#include "qpsk_tx_internal.h"

namespace {

using namespace qfmt;

constexpr int kChunk = 8;        // samples of a lane's global load in the tile kernel

// grid.y strides over rows, grid.x * kBlock over a row's aligned 16-byte units
template <int ENC>
__global__ __launch_bounds__(kBlock) void planar_kernel(const int16_t* __restrict__ src, size_t src_ld,
                                                        uint8_t* __restrict__ dst, size_t ld, unsigned nch,
                                                        size_t n) {
    for (unsigned c = blockIdx.y; c < nch; c += gridDim.y) {
        const int16_t* srow = src + (size_t)c * src_ld;
        uint8_t* drow = dst + (size_t)c * ld;
        const unsigned off = (unsigned)(reinterpret_cast<uintptr_t>(drow) & 15u);
        // unit u is the 16 destination bytes at drow - off + 16 u: elements [16 u - off, 16 u - off + 16)
        const size_t nunits = (off + n + 15) / 16;
        const uintptr_t s_lo = reinterpret_cast<uintptr_t>(srow), s_hi = reinterpret_cast<uintptr_t>(srow + n);
        // bytes from an aligned source word to a unit's first sample: one value per row
        const unsigned r = (unsigned)((s_lo - 2 * (uintptr_t)off) & 15u);
        for (size_t u = (size_t)blockIdx.x * kBlock + threadIdx.x; u < nunits; u += (size_t)gridDim.x * kBlock) {
            const long long e0 = (long long)(16 * u) - (long long)off;
            const uintptr_t w0 = s_lo + 2 * (uintptr_t)e0 - r;   // the aligned word the unit's samples start in
            const bool wide = e0 >= 0 && (size_t)e0 + 16 <= n && w0 >= s_lo && w0 + (r ? 48 : 32) <= s_hi;
            if (wide) {
                const uint4* words = reinterpret_cast<const uint4*>(w0);
                const uint4 a = words[0], b = words[1];
                const uint4 x = r ? words[2] : make_uint4(0, 0, 0, 0);
                const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, x.x, x.y, x.z, x.w};
                unsigned d[8];
                switch (r >> 2) {   // the same in every lane of the block
                    case 0: shifted<0, 8>(w, r & 3u, d); break;
                    case 1: shifted<1, 8>(w, r & 3u, d); break;
                    case 2: shifted<2, 8>(w, r & 3u, d); break;
                    default: shifted<3, 8>(w, r & 3u, d); break;
                }
                *reinterpret_cast<uint4*>(drow + e0) =
                    make_uint4(encode4<ENC>(d[0], d[1]), encode4<ENC>(d[2], d[3]), encode4<ENC>(d[4], d[5]),
                               encode4<ENC>(d[6], d[7]));
            } else {
                const size_t lo = e0 > 0 ? (size_t)e0 : 0;
                const size_t hi = (size_t)(e0 + 16) < n ? (size_t)(e0 + 16) : n;
                for (size_t e = lo; e < hi; e++) drow[e] = (uint8_t)encode<ENC>(srow[e]);
            }
        }
    }
}

// The tile in LDS: element (c, p) at c * RS + skew(c) + p * ES.  Rows along time
// padded by one dword, and the upper 32 channels 3 dwords further on: DESIGN.md
// (f2) has what that does to the banks.
template <int ES>
__device__ __forceinline__ unsigned tile_at(unsigned c, unsigned p) {
    constexpr unsigned RS = kTT * ES + 4;
    return c * RS + (c >= 32u ? 12u : 0u) + p * ES;
}

template <int ENC, int W>
__global__ __launch_bounds__(kBlock) void interleaved_kernel(const int16_t* __restrict__ src, size_t src_ld,
                                                             unsigned nch, size_t n, uint8_t* __restrict__ dst,
                                                             size_t ld, unsigned ctiles, size_t ntiles) {
    constexpr int ES = ENC == QPSK_OUT_S16 ? 2 : 1;   // bytes of an element
    constexpr int RS = kTT * ES + 4;                 // bytes of a tile row in LDS
    constexpr int V = W / ES;                        // elements of a lane's store
    constexpr int LPR = kTC / V;                     // lanes that store a destination row of the tile
    constexpr int NST = kTT * LPR / kBlock;          // store passes
    constexpr int NLD = kTC * (kTT / kChunk) / kBlock;   // load passes
    constexpr int CD = kChunk * ES / 4;              // dwords a loaded chunk takes in the tile
    constexpr int DW = W >= 4 ? W / 4 : 1;
    static_assert(W >= ES && V >= 1 && V <= 16 && NST * kBlock == kTT * LPR && NLD * kBlock == kTC * kTT / kChunk,
                  "tile shape");
    __shared__ __attribute__((aligned(16))) uint8_t tile[kTC * RS + 16];
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned c0 = (unsigned)(t % ctiles) * kTC;
        const size_t p0 = (t / ctiles) * kTT;
        // 8 samples of one channel along time per lane: a wave reads 4 channels x 256 bytes
        unsigned v[NLD][4];
#pragma unroll
        for (int it = 0; it < NLD; it++) {
            const unsigned idx = threadIdx.x + it * kBlock;
            const unsigned chunk = idx % (kTT / kChunk), c = idx / (kTT / kChunk);
            const size_t p = p0 + chunk * kChunk;
#pragma unroll
            for (int j = 0; j < 4; j++) v[it][j] = 0;
            if (c0 + c < nch && p < n) {
                const int16_t* s = src + (size_t)(c0 + c) * src_ld + p;
                if (p + kChunk <= n && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
                    const uint4 x = *reinterpret_cast<const uint4*>(s);
                    v[it][0] = x.x, v[it][1] = x.y, v[it][2] = x.z, v[it][3] = x.w;
                } else {   // a row that is not 16-byte aligned, or the block's last samples
#pragma unroll
                    for (int j = 0; j < kChunk; j++)
                        if (p + j < n) v[it][j / 2] |= (unsigned)(uint16_t)s[j] << (16 * (j % 2));
                }
            }
        }
#pragma unroll
        for (int it = 0; it < NLD; it++) {
            const unsigned idx = threadIdx.x + it * kBlock;
            const unsigned chunk = idx % (kTT / kChunk), c = idx / (kTT / kChunk);
            unsigned* q = reinterpret_cast<unsigned*>(tile + tile_at<ES>(c, chunk * kChunk));
            if constexpr (ES == 2) {
#pragma unroll
                for (int j = 0; j < CD; j++) q[j] = v[it][j];
            } else {
                q[0] = encode4<ENC>(v[it][0], v[it][1]);
                q[1] = encode4<ENC>(v[it][2], v[it][3]);
            }
        }
        __syncthreads();
        // a lane: V elements down the channel rows -> W bytes along the channel axis
#pragma unroll
        for (int it = 0; it < NST; it++) {
            const unsigned s = threadIdx.x + it * kBlock;
            const unsigned cl = (s % LPR) * V, pr = s / LPR;
            const size_t p = p0 + pr;
            if (p < n && c0 + cl < nch) {
                uint8_t* o = dst + (p * ld + c0 + cl) * ES;
                unsigned x[DW];
#pragma unroll
                for (int j = 0; j < DW; j++) x[j] = 0;
                unsigned e[V];
#pragma unroll
                for (int j = 0; j < V; j++) {
                    const unsigned b = tile_at<ES>(cl + j, pr);
                    e[j] = ES == 1 ? tile[b] : *reinterpret_cast<const uint16_t*>(tile + b);
                    x[(j * ES) / 4] |= e[j] << (8 * ((j * ES) % 4));
                }
                if (c0 + cl + V <= nch) {
                    store_wide<W>(o, x);
                } else {   // the block's last channels: only those there are
#pragma unroll
                    for (int j = 0; j < V; j++)
                        if (c0 + cl + j < nch) {
                            if constexpr (ES == 1) o[j] = (uint8_t)e[j];
                            else reinterpret_cast<uint16_t*>(o)[j] = (uint16_t)e[j];
                        }
                }
            }
        }
        __syncthreads();   // the tile is rewritten by the next round
    }
}

template <int ENC>
void launch_planar(const int16_t* src, size_t src_ld, uint8_t* dst, size_t ld, unsigned nch, size_t n,
                   hipStream_t s) {
    const size_t units = (n + 30) / 16;   // of the row with the longest head
    hipLaunchKernelGGL((planar_kernel<ENC>), dim3(grid_of((units + kBlock - 1) / kBlock), grid_of(nch, 65535u)),
                       dim3(kBlock), 0, s, src, src_ld, dst, ld, nch, n);
}

template <int ENC, int W>
void launch_tile(const int16_t* src, size_t src_ld, unsigned nch, size_t n, uint8_t* dst, size_t ld,
                 hipStream_t s) {
    const unsigned ctiles = (nch + kTC - 1) / kTC;
    const size_t ntiles = (size_t)ctiles * ((n + kTT - 1) / kTT);
    hipLaunchKernelGGL((interleaved_kernel<ENC, W>), dim3(grid_of(ntiles)), dim3(kBlock), 0, s, src, src_ld,
                       nch, n, dst, ld, ctiles, ntiles);
}

}  // namespace

extern "C" int qpsk_output_store_width(const void* d_dst, long ld, int esize) {
    return fmt_access_width(d_dst, ld, esize);
}

extern "C" int qpsk_output_convert_device_w(int fmt, const int16_t* d_src, long src_ld, int nch, long n,
                                            void* d_dst, long ld, void* stream, int* width) {
    if (width) *width = 0;
    if (qpsk_output_check(fmt, nch, n, src_ld, ld) != QPSK_OK) return QPSK_EINVAL;
    if (n == 0) return QPSK_OK;
    const int es = qpsk_fmt_esize(fmt), enc = QPSK_FMT_ENC(fmt);
    if (!d_src || !d_dst || (reinterpret_cast<uintptr_t>(d_src) & 1u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_dst) & (uintptr_t)(es - 1)) != 0)
        return QPSK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* dst = static_cast<uint8_t*>(d_dst);
    const unsigned uc = (unsigned)nch;
    if (QPSK_FMT_LAYOUT(fmt) == QPSK_OUT_PLANAR) {
        if (enc == QPSK_OUT_S16) {   // rows of n samples, ld apart
            HCHECK(hipMemcpy2DAsync(d_dst, sizeof(int16_t) * (size_t)ld, d_src, sizeof(int16_t) * (size_t)src_ld,
                                    sizeof(int16_t) * (size_t)n, (size_t)nch, hipMemcpyDeviceToDevice, s));
            return QPSK_OK;
        }
        // rows that follow each other without a seam are one row
        const bool flat = src_ld == n && ld == n;
        const unsigned rows = flat ? 1u : uc;
        const size_t len = flat ? (size_t)nch * (size_t)n : (size_t)n;
        with_encoding(enc, [&](auto e) {
            if constexpr (e() != QPSK_OUT_S16) launch_planar<e()>(d_src, (size_t)src_ld, dst, (size_t)ld, rows, len, s);
        });
    } else {
        const int w = qpsk_output_store_width(d_dst, ld, es);
        if (width) *width = w;
        with_encoding(enc, [&](auto e) {
            with_width<esize_of(e())>(w, [&](auto wc) {
                launch_tile<e(), wc()>(d_src, (size_t)src_ld, uc, (size_t)n, dst, (size_t)ld, s);
            });
        });
    }
    HCHECK(hipGetLastError());
    return QPSK_OK;
}

extern "C" int qpsk_output_convert_device(int fmt, const int16_t* d_src, long src_ld, int nch, long n, void* d_dst,
                                          long ld, void* stream) {
    return qpsk_output_convert_device_w(fmt, d_src, src_ld, nch, n, d_dst, ld, stream, nullptr);
}

// ---------------------------------------------------------------- the transmitter in front of it
namespace {

// what qpsk_tx_batch refuses, and the block's own checks; *N = samples of a row
int tx_fmt_check(const qpsk_tx_ctx* c, const void* bits, int npackets, const void* out, int fmt, long ld, long* N) {
    const int nch = qpsk_tx_channels(c), gap = qpsk_tx_gap(c);   // QPSK_EINVAL for a null context
    if (nch < 1 || gap < 0 || npackets < 0 || qpsk_fmt_esize(fmt) == 0) return QPSK_EINVAL;
    *N = (long)npackets * ((long)QPSK_TX_PACKET + gap);
    if (npackets == 0) return QPSK_OK;
    if (!bits || !out || (long)nch * npackets >= QPSK_TX_MAX_CHANNEL_PACKETS) return QPSK_EINVAL;
    return qpsk_output_check(fmt, nch, *N, *N, ld);
}

// the modulator's rows in the context's buffer start 16-byte aligned
long conv_ld(long N) { return (N + 7) & ~7L; }

// qpsk_tx_batch_masked_device_fmt on a chosen path; d_active NULL = the plain call
int tx_device_fmt(qpsk_tx_ctx* c, const uint8_t* d_bits, const uint8_t* d_active, int npackets, void* d_out,
                  int fmt, long ld, void* stream, int path) {
    if (fmt == (QPSK_OUT_S16 | QPSK_OUT_PLANAR))
        return qpsk_tx_batch_masked_device(c, d_bits, d_active, npackets, static_cast<int16_t*>(d_out), ld, stream);
    long N = 0;
    const int chk = tx_fmt_check(c, d_bits, npackets, d_out, fmt, ld, &N);
    const bool fusable = QPSK_FMT_LAYOUT(fmt) == QPSK_OUT_PLANAR && QPSK_FMT_ENC(fmt) != QPSK_OUT_S16;
    if (path == QPSK_OUT_PATH_DEFAULT) path = fusable ? QPSK_OUT_PATH_FUSED : QPSK_OUT_PATH_PREPASS;
    if ((path != QPSK_OUT_PATH_PREPASS && path != QPSK_OUT_PATH_FUSED) || (path == QPSK_OUT_PATH_FUSED && !fusable))
        return QPSK_EINVAL;
    if (chk != QPSK_OK || npackets == 0) return chk;
    if (path == QPSK_OUT_PATH_FUSED)   // the modulator's store pass writes the codes
        return qpsk_tx_batch_masked_device_enc(c, d_bits, d_active, npackets, d_out, ld, stream, QPSK_FMT_ENC(fmt));
    const int nch = qpsk_tx_channels(c);
    const long sld = conv_ld(N);
    int16_t* conv = nullptr;
    int r = qpsk_tx_fmt_conv(c, (size_t)nch * (size_t)sld, &conv);
    if (r != QPSK_OK) return r;
    r = qpsk_tx_batch_masked_device(c, d_bits, d_active, npackets, conv, sld, stream);
    if (r != QPSK_OK) return r;
    r = qpsk_output_convert_device(fmt, conv, sld, nch, N, d_out, ld, stream);
    if (r != QPSK_OK) return r;
    return qpsk_tx_mark(c, stream);
}

}  // namespace

extern "C" int qpsk_tx_batch_device_fmt_path(qpsk_tx_ctx* c, const uint8_t* d_bits, int npackets, void* d_out,
                                             int fmt, long ld, void* stream, int path) {
    return tx_device_fmt(c, d_bits, nullptr, npackets, d_out, fmt, ld, stream, path);
}

extern "C" int qpsk_tx_batch_device_fmt(qpsk_tx_ctx* c, const uint8_t* d_bits, int npackets, void* d_out, int fmt,
                                        long ld, void* stream) {
    return tx_device_fmt(c, d_bits, nullptr, npackets, d_out, fmt, ld, stream, QPSK_OUT_PATH_DEFAULT);
}

extern "C" int qpsk_tx_batch_masked_device_fmt(qpsk_tx_ctx* c, const uint8_t* d_bits, const uint8_t* d_active,
                                               int npackets, void* d_out, int fmt, long ld, void* stream) {
    return tx_device_fmt(c, d_bits, d_active, npackets, d_out, fmt, ld, stream, QPSK_OUT_PATH_DEFAULT);
}

extern "C" int qpsk_tx_batch_fmt(qpsk_tx_ctx* c, const uint8_t* bits, int npackets, void* out, int fmt, long ld) {
    return qpsk_tx_batch_masked_fmt(c, bits, nullptr, npackets, out, fmt, ld);
}

extern "C" int qpsk_tx_batch_masked_fmt(qpsk_tx_ctx* c, const uint8_t* bits, const uint8_t* active, int npackets,
                                        void* out, int fmt, long ld) {
    if (fmt == (QPSK_OUT_S16 | QPSK_OUT_PLANAR))
        return qpsk_tx_batch_masked(c, bits, active, npackets, static_cast<int16_t*>(out), ld);
    long N = 0;
    const int chk = tx_fmt_check(c, bits, npackets, out, fmt, ld, &N);
    if (chk != QPSK_OK || npackets == 0) return chk;
    HCHECK(hipSetDevice(qpsk_tx_device(c)));
    // a device call still pending on a caller's stream (qpsk_tx_batch waits alike)
    const int pend = qpsk_tx_sync(c);
    if (pend != QPSK_OK) return pend;
    hipStream_t s = (hipStream_t)qpsk_tx_host_stream(c);
    const int nch = qpsk_tx_channels(c);
    const size_t es = (size_t)qpsk_fmt_esize(fmt);
    const bool inter = QPSK_FMT_LAYOUT(fmt) == QPSK_OUT_INTERLEAVED;
    // the block on the device is dense: rows of `width` bytes, `rows` of them
    const size_t width = (inter ? (size_t)nch : (size_t)N) * es, rows = inter ? (size_t)N : (size_t)nch;
    const size_t nbits = (size_t)nch * (size_t)npackets * QPSK_TX_PACKET_BITS;
    const size_t nact = active ? (size_t)nch * (size_t)npackets : 0;
    qhip::DevBuf<uint8_t> d_bits, d_active, d_block;   // released on return, after the synchronisation
    int r = herr(d_bits.reserve(nbits));
    if (r == QPSK_OK) r = herr(d_active.reserve(nact));
    if (r == QPSK_OK) r = herr(d_block.reserve(width * rows));
    if (r == QPSK_OK) r = herr(hipMemcpyAsync(d_bits, bits, nbits, hipMemcpyHostToDevice, s));
    if (r == QPSK_OK && active) r = herr(hipMemcpyAsync(d_active, active, nact, hipMemcpyHostToDevice, s));
    if (r == QPSK_OK)
        r = qpsk_tx_batch_masked_device_fmt(c, d_bits, d_active, npackets, d_block, fmt, inter ? (long)nch : N, s);
    // only the block's bytes come back: the caller's row tails and foreign columns keep their contents
    if (r == QPSK_OK) {
        if ((size_t)ld * es == width)
            r = herr(hipMemcpyAsync(out, d_block, width * rows, hipMemcpyDeviceToHost, s));
        else
            r = herr(hipMemcpy2DAsync(out, (size_t)ld * es, d_block, width, width, rows, hipMemcpyDeviceToHost, s));
    }
    const int r2 = herr(hipStreamSynchronize(s));
    if (r == QPSK_OK) r = r2;
    return r == QPSK_EHIP - (int)hipErrorOutOfMemory ? QPSK_ENOMEM : r;
}
