// zlib inflate (RFC 1950 / 1951) of one stream by one thread: stored, fixed- and dynamic-Huffman blocks, overlapping copies,
// header and Adler-32 checks.  Canonical-code tables in puff's count / symbol form (HuffLds: 896 B, the kernel keeps one per
// thread in LDS).  Every read is bounded by in_len, every write by out_cap.  Pure functions, shared by peakdecode.hip's
// inflate kernel and the host build of the CPU tests.
#pragma once
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

constexpr int kMaxBits = 15;
constexpr int kMaxLit = 288;
constexpr int kMaxDist = 30;

// per-thread canonical Huffman tables (LDS)
struct __attribute__((aligned(16))) HuffLds {
    uint16_t lencnt[16];
    uint16_t distcnt[16];
    uint16_t offs[16];
    uint16_t lensym[kMaxLit];
    uint16_t distsym[kMaxDist + 2];
    uint8_t lengths[160];            // code lengths of the dynamic header, two 4-bit values per byte (320 symbols)
};
static_assert(sizeof(HuffLds) == 896, "HuffLds layout");

struct Inflater {
    const uint8_t* in;
    int64_t in_len, in_pos;
    uint32_t bitbuf;
    int bitcnt;
    uint8_t* out;
    int64_t out_cap, out_pos;
    uint32_t s1, s2;                 // Adler-32
    int err;

    __host__ __device__ __forceinline__ uint32_t bits(int need) {        // need <= 16
        while (bitcnt < need) {
            if (in_pos >= in_len) {
                err |= FAL_PEAK_ST_CODE;                        // stream ends inside a block
                return 0;
            }
            bitbuf |= (uint32_t)in[in_pos++] << bitcnt;
            bitcnt += 8;
        }
        const uint32_t v = bitbuf & ((1u << need) - 1u);
        bitbuf >>= need;
        bitcnt -= need;
        return v;
    }

    __host__ __device__ __forceinline__ void emit(uint8_t b) {
        out[out_pos++] = b;
        s1 += b;
        if (s1 >= 65521u) s1 -= 65521u;
        s2 += s1;
        if (s2 >= 65521u) s2 -= 65521u;
    }

    // one symbol of a canonical code (count per length, symbols in code order); -1 on a code that is not in the table
    __host__ __device__ __forceinline__ int decode(const uint16_t* cnt, const uint16_t* sym) {
        int code = 0, first = 0, index = 0;
        for (int len = 1; len <= kMaxBits; ++len) {
            code |= (int)bits(1);
            const int count = cnt[len];
            if (code - count < first) return sym[index + (code - first)];
            index += count;
            first = (first + count) << 1;
            code <<= 1;
            if (err) return -1;
        }
        return -1;
    }
};

__host__ __device__ __forceinline__ int get_len(const uint8_t* l, int i) { return (l[i >> 1] >> ((i & 1) * 4)) & 15; }
__host__ __device__ __forceinline__ void set_len(uint8_t* l, int i, int v) {
    const int sh = (i & 1) * 4;
    l[i >> 1] = (uint8_t)((l[i >> 1] & ~(15 << sh)) | (v << sh));
}

// canonical code from code lengths[first .. first + n) (4-bit packed) -> cnt / sym; returns the unused code space (0 = complete,
// > 0 = incomplete, < 0 = over-subscribed), as puff's construct()
static __host__ __device__ int construct(uint16_t* cnt, uint16_t* sym, uint16_t* offs, const uint8_t* lengths, int first, int n) {
    for (int len = 0; len <= kMaxBits; ++len) cnt[len] = 0;
    for (int s = 0; s < n; ++s) cnt[get_len(lengths, first + s)]++;
    if (cnt[0] == n) return 0;
    int left = 1;
    for (int len = 1; len <= kMaxBits; ++len) {
        left <<= 1;
        left -= cnt[len];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int len = 1; len < kMaxBits; ++len) offs[len + 1] = offs[len] + cnt[len];
    for (int s = 0; s < n; ++s) {
        const int l = get_len(lengths, first + s);
        if (l) sym[offs[l]++] = (uint16_t)s;
    }
    return left;
}

// length / distance bases and extra bits (RFC 1951 3.2.5) without tables
__host__ __device__ __forceinline__ void length_base(int i, int* base, int* extra) {     // i = symbol - 257, 0..28
    if (i < 8) { *base = 3 + i; *extra = 0; }
    else if (i == 28) { *base = 258; *extra = 0; }
    else { const int e = (i - 4) >> 2; *base = ((4 + (i & 3)) << e) + 3; *extra = e; }
}
__host__ __device__ __forceinline__ void dist_base(int i, int* base, int* extra) {       // i = 0..29
    if (i < 4) { *base = 1 + i; *extra = 0; }
    else { const int e = (i - 2) >> 1; *base = ((2 + (i & 1)) << e) + 1; *extra = e; }
}

// order of the code-length code lengths, 5 bits per entry: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
constexpr uint64_t pack5(const int* v, int n) {
    uint64_t r = 0;
    for (int i = 0; i < n; ++i) r |= (uint64_t)v[i] << (5 * i);
    return r;
}
constexpr int kOrderLo[12] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4};
constexpr int kOrderHi[7] = {12, 3, 13, 2, 14, 1, 15};
constexpr uint64_t kOrderLoBits = pack5(kOrderLo, 12), kOrderHiBits = pack5(kOrderHi, 7);
__host__ __device__ __forceinline__ int cl_order(int i) {
    return (int)(((i < 12 ? kOrderLoBits >> (5 * i) : kOrderHiBits >> (5 * (i - 12)))) & 31);
}

// literal / length + distance symbols of one block until end-of-block
static __host__ __device__ void inflate_codes(Inflater& z, const HuffLds& h) {
    while (!z.err) {
        const int sym = z.decode(h.lencnt, h.lensym);
        if (sym < 0) { z.err |= FAL_PEAK_ST_CODE; return; }
        if (sym < 256) {
            if (z.out_pos >= z.out_cap) { z.err |= FAL_PEAK_ST_OVERFLOW; return; }
            z.emit((uint8_t)sym);
        } else if (sym == 256) {
            return;
        } else {
            if (sym > 285) { z.err |= FAL_PEAK_ST_CODE; return; }
            int base, extra;
            length_base(sym - 257, &base, &extra);
            const int len = base + (int)z.bits(extra);
            const int ds = z.decode(h.distcnt, h.distsym);
            if (ds < 0 || ds > 29) { z.err |= FAL_PEAK_ST_CODE; return; }
            dist_base(ds, &base, &extra);
            const int64_t dist = base + (int64_t)z.bits(extra);
            if (z.err) return;
            if (dist > z.out_pos) { z.err |= FAL_PEAK_ST_CODE; return; }
            if (len > z.out_cap - z.out_pos) { z.err |= FAL_PEAK_ST_OVERFLOW; return; }
            for (int k = 0; k < len; ++k) z.emit(z.out[z.out_pos - dist]);     // byte by byte: overlapping copies repeat
        }
    }
}

static __host__ __device__ void inflate_fixed(Inflater& z, HuffLds& h) {
    for (int s = 0; s < 320; s += 2) {
        const int l0 = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
        const int l1 = s + 1 < 144 ? 8 : s + 1 < 256 ? 9 : s + 1 < 280 ? 7 : s + 1 < 288 ? 8 : 5;
        h.lengths[s >> 1] = (uint8_t)(l0 | (l1 << 4));
    }
    construct(h.lencnt, h.lensym, h.offs, h.lengths, 0, 288);
    construct(h.distcnt, h.distsym, h.offs, h.lengths, 288, 30);
    inflate_codes(z, h);
}

static __host__ __device__ void inflate_dynamic(Inflater& z, HuffLds& h) {
    const int nlen = (int)z.bits(5) + 257, ndist = (int)z.bits(5) + 1, ncode = (int)z.bits(4) + 4;
    if (z.err) return;
    if (nlen > 286 || ndist > 30) { z.err |= FAL_PEAK_ST_CODE; return; }
    // code-length code: 19 lengths in their permuted order, kept in lengths[0 .. 19)
    for (int i = 0; i < 19; ++i) set_len(h.lengths, i, 0);
    for (int i = 0; i < ncode; ++i) set_len(h.lengths, cl_order(i), (int)z.bits(3));
    if (z.err) return;
    if (construct(h.lencnt, h.lensym, h.offs, h.lengths, 0, 19) != 0) { z.err |= FAL_PEAK_ST_CODE; return; }
    int idx = 0;
    while (idx < nlen + ndist) {
        int sym = z.decode(h.lencnt, h.lensym);
        if (sym < 0 || z.err) { z.err |= FAL_PEAK_ST_CODE; return; }
        if (sym < 16) {
            set_len(h.lengths, idx++, sym);
            continue;
        }
        int val = 0, rep;
        if (sym == 16) {
            if (idx == 0) { z.err |= FAL_PEAK_ST_CODE; return; }
            val = get_len(h.lengths, idx - 1);
            rep = 3 + (int)z.bits(2);
        } else if (sym == 17) {
            rep = 3 + (int)z.bits(3);
        } else {
            rep = 11 + (int)z.bits(7);
        }
        if (z.err || idx + rep > nlen + ndist) { z.err |= FAL_PEAK_ST_CODE; return; }
        while (rep--) set_len(h.lengths, idx++, val);
    }
    if (get_len(h.lengths, 256) == 0) { z.err |= FAL_PEAK_ST_CODE; return; }      // no end-of-block code
    // the lengths live in lengths[0 .. nlen + ndist); the code-length code's tables are overwritten now
    int left = construct(h.lencnt, h.lensym, h.offs, h.lengths, 0, nlen);
    if (left < 0 || (left > 0 && nlen != h.lencnt[0] + h.lencnt[1])) { z.err |= FAL_PEAK_ST_CODE; return; }
    left = construct(h.distcnt, h.distsym, h.offs, h.lengths, nlen, ndist);
    if (left < 0 || (left > 0 && ndist != h.distcnt[0] + h.distcnt[1])) { z.err |= FAL_PEAK_ST_CODE; return; }
    inflate_codes(z, h);
}

static __host__ __device__ void inflate_stored(Inflater& z) {
    z.bitbuf = 0;                                                       // to the byte boundary (fewer than 8 bits are held)
    z.bitcnt = 0;
    if (z.in_len - z.in_pos < 4) { z.err |= FAL_PEAK_ST_CODE; return; }
    const uint32_t len = z.in[z.in_pos] | ((uint32_t)z.in[z.in_pos + 1] << 8);
    const uint32_t nlen = z.in[z.in_pos + 2] | ((uint32_t)z.in[z.in_pos + 3] << 8);
    z.in_pos += 4;
    if (len != (~nlen & 0xFFFFu)) { z.err |= FAL_PEAK_ST_CODE; return; }
    if ((int64_t)len > z.in_len - z.in_pos) { z.err |= FAL_PEAK_ST_CODE; return; }
    if ((int64_t)len > z.out_cap - z.out_pos) { z.err |= FAL_PEAK_ST_OVERFLOW; return; }
    for (uint32_t k = 0; k < len; ++k) z.emit(z.in[z.in_pos + k]);
    z.in_pos += len;
}

// one zlib stream (in[0 .. in_len)) into out[0 .. out_cap): 0, or FAL_PEAK_ST_* bits; *out_len = the bytes written.  `exact`:
// an output shorter than out_cap is FAL_PEAK_ST_SHORT; otherwise out_cap is an upper bound only (a stream whose inflated size
// is not declared: MS-Numpress) and the caller takes the length.
static __host__ __device__ int inflate_stream_upto(const uint8_t* in, int64_t in_len, uint8_t* out, int64_t out_cap, bool exact,
                                                   int64_t* out_len, HuffLds& h) {
    Inflater z;
    z.in = in;
    z.in_len = in_len;
    z.in_pos = 0;
    z.bitbuf = 0;
    z.bitcnt = 0;
    z.out = out;
    z.out_cap = out_cap;
    z.out_pos = 0;
    z.s1 = 1;
    z.s2 = 0;
    z.err = 0;
    // RFC 1950 header: CM = 8, CINFO <= 7, FCHECK, no preset dictionary
    *out_len = 0;
    if (in_len < 2) return FAL_PEAK_ST_HEADER;
    const uint32_t cmf = in[0], flg = in[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return FAL_PEAK_ST_HEADER;
    z.in_pos = 2;
    int last = 0;
    while (!last && !z.err) {
        last = (int)z.bits(1);
        const int type = (int)z.bits(2);
        if (z.err) break;
        if (type == 0) inflate_stored(z);
        else if (type == 1) inflate_fixed(z, h);
        else if (type == 2) inflate_dynamic(z, h);
        else z.err |= FAL_PEAK_ST_CODE;
    }
    *out_len = z.out_pos;
    if (!z.err && exact && z.out_pos != z.out_cap) z.err |= FAL_PEAK_ST_SHORT;
    if (!z.err) {
        const int64_t p = z.in_pos;                                     // the bit buffer holds < 8 bits: the trailer is byte aligned
        if (in_len - p < 4) return FAL_PEAK_ST_ADLER;
        const uint32_t want = ((uint32_t)in[p] << 24) | ((uint32_t)in[p + 1] << 16) | ((uint32_t)in[p + 2] << 8) | in[p + 3];
        if (want != ((z.s2 << 16) | z.s1)) z.err |= FAL_PEAK_ST_ADLER;
    }
    return z.err;
}

// the declared-size form: the stream must fill out[0 .. out_cap) exactly.  Host-callable as well: tests/test_inflate_cpu.py
// builds this header with the host compiler and checks it against zlib (good, corrupted and truncated streams).
static __host__ __device__ int inflate_stream(const uint8_t* in, int64_t in_len, uint8_t* out, int64_t out_cap, HuffLds& h) {
    int64_t n;
    return inflate_stream_upto(in, in_len, out, out_cap, true, &n, h);
}

}  // namespace fal
