// qpsk_fmt_dev.h -- what the device units of the formats (qpsk_input.hip,
// qpsk_output.hip, and qpsk_tx.hip for its fused store pass) share beside
// qpsk_fmt.h: the tile geometry and launch constants of the conversion
// kernels, wide loads and stores, the byte-align shift, a sample's code in an
// encoding and back, the access width of an interleaved block, and the
// dispatch from a run-time encoding or width to a kernel's template arguments.
// The kernels stay in their units; nothing here is one.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "qpsk_fmt.h"
#include "qpsk_fmt_internal.h"

namespace qfmt {

constexpr int kBlock = 256;
constexpr int kTC = 64;          // channels of a tile
constexpr int kTT = 128;         // samples of a tile
constexpr unsigned kMaxGrid = 1u << 20;

// blocks of a grid dimension: what there is to do, at least 1, at most cap
inline unsigned grid_of(size_t blocks, unsigned cap = kMaxGrid) {
    return (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap);
}

// bytes of an element of the encoding
constexpr int esize_of(int enc) { return enc == QPSK_FMT_S16 ? 2 : 1; }

template <int W> struct Wide;
template <> struct Wide<1> { using type = uint8_t; };
template <> struct Wide<2> { using type = uint16_t; };
template <> struct Wide<4> { using type = uint32_t; };
template <> struct Wide<8> { using type = uint2; };
template <> struct Wide<16> { using type = uint4; };

// W bytes at p (W-aligned) as dwords
template <int W>
__device__ __forceinline__ void load_wide(const uint8_t* p, unsigned* v) {
    const auto x = *reinterpret_cast<const typename Wide<W>::type*>(p);
    if constexpr (W == 16) v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    else if constexpr (W == 8) v[0] = x.x, v[1] = x.y;
    else v[0] = x;
}

// W bytes in dwords to p (W-aligned)
template <int W>
__device__ __forceinline__ void store_wide(uint8_t* p, const unsigned* v) {
    using T = typename Wide<W>::type;
    if constexpr (W == 16) *reinterpret_cast<T*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    else if constexpr (W == 8) *reinterpret_cast<T*>(p) = make_uint2(v[0], v[1]);
    else *reinterpret_cast<T*>(p) = (T)v[0];
}

// dwords Q .. Q+N-1 of the N+4 in w, taken r bytes further on
template <int Q, int N>
__device__ __forceinline__ void shifted(const unsigned (&w)[N + 4], unsigned r, unsigned (&d)[N]) {
#pragma unroll
    for (int j = 0; j < N; j++) d[j] = __builtin_amdgcn_alignbyte(w[Q + j + 1], w[Q + j], r);
}

// a 16-bit sample as an element of the encoding
template <int ENC>
__device__ __forceinline__ unsigned encode(int x) {
    if constexpr (ENC == QPSK_FMT_S16) return (unsigned)x & 0xffffu;
    else if constexpr (ENC == QPSK_FMT_ALAW) return qpsk_alaw_encode(x);
    else return qpsk_ulaw_encode(x);
}

__device__ __forceinline__ int lo16(unsigned d) { return (int)(int16_t)(d & 0xffffu); }
__device__ __forceinline__ int hi16(unsigned d) { return (int)d >> 16; }

// 4 int16 in two dwords -> 4 codes in one
template <int ENC>
__device__ __forceinline__ unsigned encode4(unsigned a, unsigned b) {
    return encode<ENC>(lo16(a)) | encode<ENC>(hi16(a)) << 8 | encode<ENC>(lo16(b)) << 16 |
           encode<ENC>(hi16(b)) << 24;
}

// an element of the encoding as the low 16 bits of its sample; tab: the block's
// 256-entry table, read for QPSK_IN_DEC_TABLE only
template <int ENC, int DEC>
__device__ __forceinline__ unsigned decode(unsigned code, const int16_t* tab) {
    if constexpr (ENC == QPSK_FMT_S16) return code;
    else if constexpr (DEC == QPSK_IN_DEC_TABLE) return (unsigned)(uint16_t)tab[code];
    else if constexpr (ENC == QPSK_FMT_ALAW) return (unsigned)qpsk_alaw_decode(code) & 0xffffu;
    else return (unsigned)qpsk_ulaw_decode(code) & 0xffffu;
}

// The widest access every row of an interleaved block allows: a tile's rows
// start at ptr + (t * ld + 64 * i) * esize, so the address of the block and the
// byte stride of its rows decide for the whole call; the run's last channels,
// where nch is no multiple of the lane's elements, go per element.
inline int fmt_access_width(const void* ptr, long ld, int esize) {
    const uintptr_t m = reinterpret_cast<uintptr_t>(ptr) | (uintptr_t)ld * (uintptr_t)esize;
    int w = 16;
    while (w > esize && (m & (uintptr_t)(w - 1)) != 0) w >>= 1;
    return w;
}

// A run-time encoding or width as a template argument: f gets it as a Const,
// whose value is a constant expression (e()), and names its kernel once.
template <int V> using Const = std::integral_constant<int, V>;

// f(Const<enc>) for a format word's encoding (checked: one of the three)
template <class F>
void with_encoding(int enc, F&& f) {
    if (enc == QPSK_FMT_S16) f(Const<QPSK_FMT_S16>{});
    else if (enc == QPSK_FMT_ALAW) f(Const<QPSK_FMT_ALAW>{});
    else f(Const<QPSK_FMT_ULAW>{});
}

// f(Const<w>) for w of fmt_access_width(.., ES): no kernel is narrower than an element
template <int ES, class F>
void with_width(int w, F&& f) {
    switch (w) {
        case 16: return f(Const<16>{});
        case 8: return f(Const<8>{});
        case 4: return f(Const<4>{});
        case 2: return f(Const<2>{});
        default:
            if constexpr (ES == 1) f(Const<1>{});
            return;
    }
}

}  // namespace qfmt
