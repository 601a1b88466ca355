// MS-Numpress decode (linear MS:1002312, pic MS:1002313, slof MS:1002314) of one stream: the bytes of an mzML binary array after
// base64 (and zlib, for the combined terms) -> float64 values.  DESIGN.md "MS-Numpress" states the format; parity with outside
// encoders is UNPINNED.  Every read is bounded by the stream's length, every write by out_cap.  Pure functions, shared by
// peakdecode.hip's numpress kernel and the host build of the CPU tests (tests/hostbuild_numpress.py).
//   half-byte integer: a head nibble h, then the 8 - n low nibbles of a signed 32-bit value, least significant first, where the
//   n = h (h <= 8) most significant nibbles are 0 or the n = h - 8 (h > 8) most significant are 0xF.  Nibbles are packed high
//   nibble first; a stream of an odd number of nibbles ends with a low nibble of 0.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/falcon_hip.h"
#ifndef __HIPCC__            // plain host compiler (the CPU tests' shim): the qualifiers mean nothing there
#ifndef __host__
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#endif

namespace fal {

// the longest stream of `count` values (a value is at most 9 nibbles): the inflate capacity of a zlib + numpress array
__host__ __device__ __forceinline__ int64_t numpress_max_bytes(int64_t codec, int64_t count) {
    if (codec == FAL_PEAK_NUMPRESS_LINEAR) return count <= 0 ? 8 : count == 1 ? 12 : 16 + (9 * (count - 2) + 1) / 2;
    if (codec == FAL_PEAK_NUMPRESS_PIC) return (9 * count + 1) / 2;
    return 8 + 2 * count;
}

__host__ __device__ __forceinline__ int np_nibble(const uint8_t* in, int64_t pos) { return (in[pos >> 1] >> ((~pos & 1) * 4)) & 15; }

// the end of a half-byte stream of n_nib = 2 x bytes nibbles: behind the last byte, or at its low nibble when that is 0
__host__ __device__ __forceinline__ bool np_at_end(const uint8_t* in, int64_t n_nib, int64_t pos) {
    return pos >= n_nib || (pos == n_nib - 1 && (in[pos >> 1] & 15) == 0);
}

// one half-byte integer at nibble *pos; false when the head or a data nibble lies beyond the last byte
__host__ __device__ __forceinline__ bool np_half_byte_int(const uint8_t* in, int64_t n_nib, int64_t* pos, int32_t* x) {
    int64_t p = *pos;
    if (p >= n_nib) return false;
    const int h = np_nibble(in, p++);
    const int n = h <= 8 ? h : h - 8;                                   // filled nibbles: 0..8 of 0x0, 1..7 of 0xF
    if (8 - n > n_nib - p) return false;
    uint32_t v = h <= 8 ? 0u : 0xFFFFFFFFu << (4 * (8 - n));
    for (int i = 0; i < 8 - n; ++i) v |= (uint32_t)np_nibble(in, p++) << (4 * i);
    *pos = p;
    *x = (int32_t)v;
    return true;
}

// the fixed point of linear / slof: bytes 0-7, a float64 in big-endian order; false unless finite and > 0
__host__ __device__ __forceinline__ bool np_fixed_point(const uint8_t* in, double* fp) {
    uint64_t u = 0;
    for (int i = 0; i < 8; ++i) u = (u << 8) | in[i];
    double f;
    __builtin_memcpy(&f, &u, 8);
    *fp = f;
    return f > 0.0 && f <= DBL_MAX;
}

__host__ __device__ __forceinline__ int32_t np_i32le(const uint8_t* p) {
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// pic: every value one half-byte integer.  -> 0 or FAL_PEAK_ST_* bits; *n_out = values written (<= out_cap)
static __host__ __device__ int numpress_pic(const uint8_t* in, int64_t len, double* out, int64_t out_cap, int64_t* n_out) {
    const int64_t n_nib = 2 * len;
    int64_t pos = 0, n = 0;
    int st = 0;
    while (!np_at_end(in, n_nib, pos)) {                                // every turn consumes a nibble or leaves
        int32_t x;
        if (n >= out_cap) { st = FAL_PEAK_ST_OVERFLOW; break; }
        if (!np_half_byte_int(in, n_nib, &pos, &x)) { st = FAL_PEAK_ST_NUMPRESS; break; }
        out[n++] = (double)x;
    }
    *n_out = n;
    return st;
}

// linear: fixed point, y0, y1 (i32 little-endian), then half-byte second differences: y_i = 2 y_{i-1} - y_{i-2} + d_i (int64,
// wrapping); value = (double)y_i / fp
static __host__ __device__ int numpress_linear(const uint8_t* in, int64_t len, double* out, int64_t out_cap, int64_t* n_out) {
    *n_out = 0;
    double fp;
    if (len < 8 || (len > 8 && len < 12) || (len > 12 && len < 16) || !np_fixed_point(in, &fp)) return FAL_PEAK_ST_NUMPRESS;
    if (len == 8) return 0;
    if (out_cap < 1) return FAL_PEAK_ST_OVERFLOW;
    uint64_t y0 = (uint64_t)(int64_t)np_i32le(in + 8);
    out[0] = (double)(int64_t)y0 / fp;
    *n_out = 1;
    if (len == 12) return 0;
    if (out_cap < 2) return FAL_PEAK_ST_OVERFLOW;
    uint64_t y1 = (uint64_t)(int64_t)np_i32le(in + 12);
    out[1] = (double)(int64_t)y1 / fp;
    const uint8_t* body = in + 16;
    const int64_t n_nib = 2 * (len - 16);
    int64_t pos = 0, n = 2;
    int st = 0;
    while (!np_at_end(body, n_nib, pos)) {
        int32_t d;
        if (n >= out_cap) { st = FAL_PEAK_ST_OVERFLOW; break; }
        if (!np_half_byte_int(body, n_nib, &pos, &d)) { st = FAL_PEAK_ST_NUMPRESS; break; }
        const uint64_t y = y1 + (y1 - y0) + (uint64_t)(int64_t)d;
        out[n++] = (double)(int64_t)y / fp;
        y0 = y1;
        y1 = y;
    }
    *n_out = n;
    return st;
}

// slof: fixed point, then one u16 little-endian per value: exp(u / fp) - 1.  The values are independent: the header gives the
// count, numpress_slof_value any one of them (the kernel takes one per lane).
__host__ __device__ __forceinline__ int numpress_slof_header(const uint8_t* in, int64_t len, double* fp, int64_t* n_values) {
    *n_values = 0;
    if (len < 8 || ((len - 8) & 1) || !np_fixed_point(in, fp)) return FAL_PEAK_ST_NUMPRESS;
    *n_values = (len - 8) >> 1;
    return 0;
}

__host__ __device__ __forceinline__ double numpress_slof_value(const uint8_t* in, double fp, int64_t i) {
    const uint32_t u = (uint32_t)in[8 + 2 * i] | ((uint32_t)in[9 + 2 * i] << 8);
    return exp((double)u / fp) - 1.0;
}

static __host__ __device__ int numpress_slof(const uint8_t* in, int64_t len, double* out, int64_t out_cap, int64_t* n_out) {
    double fp;
    int64_t n;
    *n_out = 0;
    const int st = numpress_slof_header(in, len, &fp, &n);
    if (st) return st;
    const int64_t m = n < out_cap ? n : out_cap;
    for (int64_t i = 0; i < m; ++i) out[i] = numpress_slof_value(in, fp, i);
    *n_out = m;
    return n > out_cap ? FAL_PEAK_ST_OVERFLOW : 0;
}

// one stream of the codec `codec` (FAL_PEAK_NUMPRESS_*) that declares `count` values into out[0 .. count): 0, or status bits
// (fewer values than declared: FAL_PEAK_ST_SHORT)
static __host__ __device__ int numpress_decode(int64_t codec, const uint8_t* in, int64_t len, double* out, int64_t count,
                                               int64_t* n_out) {
    int st = codec == FAL_PEAK_NUMPRESS_LINEAR ? numpress_linear(in, len, out, count, n_out)
             : codec == FAL_PEAK_NUMPRESS_PIC  ? numpress_pic(in, len, out, count, n_out)
                                               : numpress_slof(in, len, out, count, n_out);
    if (!st && *n_out < count) st = FAL_PEAK_ST_SHORT;
    return st;
}

}  // namespace fal
