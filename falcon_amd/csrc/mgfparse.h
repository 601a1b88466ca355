// MGF text on the device: the pure per-line functions of the reader -- line classifier, header key, CHARGE fast form and the
// decimal -> double conversion.  Shared by mgfparse.hip's kernels and the host build of the CPU tests (tests/hostbuild_mgf.py);
// they mirror falcon_amd/ms_io/mgf_io.get_spectra, which stays the reader of record: whatever these functions do not decide
// ("not decided": they never guess a value and never report an error) is decided by that reader on the host.
//
// Numbers.  Token grammar [+-]?(D+ '.'? D* | '.' D+)([eE][+-]?D+)? -> integer w (leading zeros stripped, at most 19 digits:
// fits a uint64) and decimal exponent q.  The result is the correctly rounded double (round to nearest even), the bits of
// Python's float(), for every such token with -27 <= q <= 27 (5^27 < 2^63):
//   w <= 2^53 and |q| <= 22 : Clinger's fast path, one exact double product or quotient with 10^|q| = 5^|q| 2^|q|;
//   q >= 0                  : the exact 128-bit product w 5^q, rounded once;
//   q <  0                  : long division of w 2^(64 + lz) by 5^-q to a quotient of at least 65 bits plus a sticky bit (one
//                             64-bit division and 64 shift-subtract steps: no 128-bit divide, no table), rounded once.
// Everything else float() may accept or reject (nan, inf, 1_0, letters, more digits, other exponents): not decided.
//
// Lines.  A line longer than kMgfMaxLine bytes (stripped) that is a header or peak line carries MGF_LONG: its spectrum goes to
// the host reader.  Whitespace is space, tab, CR, LF: the device grammar admits no other byte str.strip() strips.
#pragma once
#include <stdint.h>
#include "numtext.h"          // the 128-bit multiply; the qualifiers for a plain host compiler (the CPU tests' shim)

namespace fal {

constexpr int kMgfMaxLine = 4096;
enum { MGF_SKIP = 0, MGF_BEGIN = 1, MGF_END = 2, MGF_HEADER = 3, MGF_PEAK = 4, MGF_KIND = 7, MGF_LONG = 8 };
enum { MGF_KEY_OTHER = 0, MGF_KEY_TITLE = 1, MGF_KEY_PEPMASS = 2, MGF_KEY_CHARGE = 3, MGF_KEY_RT = 4 };

__host__ __device__ __forceinline__ bool mgf_space(uint32_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
__host__ __device__ __forceinline__ bool mgf_digit(uint32_t c) { return c - '0' < 10u; }

// str.strip() of p[lo, hi)
__host__ __device__ __forceinline__ void mgf_strip(const uint8_t* p, int* lo, int* hi) {
    while (*lo < *hi && mgf_space(p[*lo])) ++*lo;
    while (*hi > *lo && mgf_space(p[*hi - 1])) --*hi;
}

__host__ __device__ __forceinline__ bool mgf_equals(const uint8_t* p, int len, const char* word, int n, bool fold) {
    if (len != n) return false;
    for (int i = 0; i < n; ++i) {
        uint32_t c = p[i];
        if (fold && c - 'A' < 26u) c += 32;
        if (c != (uint32_t)(uint8_t)word[i]) return false;
    }
    return true;
}

// one line (without its '\n') -> MGF_* kind, MGF_LONG added; *lo / *hi: the stripped range
__host__ __device__ __forceinline__ int mgf_classify(const uint8_t* p, int len, int* lo, int* hi) {
    *lo = 0;
    *hi = len;
    mgf_strip(p, lo, hi);
    const int n = *hi - *lo;
    if (n == 0) return MGF_SKIP;
    const uint32_t c = p[*lo];
    if (c == '#' || c == ';' || c == '!' || c == '/') return MGF_SKIP;
    if (mgf_equals(p + *lo, n, "BEGIN IONS", 10, false)) return MGF_BEGIN;
    if (mgf_equals(p + *lo, n, "END IONS", 8, false)) return MGF_END;
    bool eq = false;
    for (int i = *lo; i < *hi && !eq; ++i) eq = p[i] == '=';
    return ((eq && !(mgf_digit(c) || c == '.')) ? MGF_HEADER : MGF_PEAK) | (n > kMgfMaxLine ? MGF_LONG : 0);
}

// a line's stripped range -> [*klo, *khi): the stripped key before the first Sep; [*vlo, *vhi): the stripped value behind it
// ('=' in MGF, ':' in MSP: mspparse.h)
template <char Sep>
__host__ __device__ __forceinline__ void mgf_split_at(const uint8_t* p, int lo, int hi, int* klo, int* khi, int* vlo, int* vhi) {
    int eq = lo;
    while (eq < hi && p[eq] != Sep) ++eq;
    *klo = lo;
    *khi = eq;
    mgf_strip(p, klo, khi);
    *vlo = eq < hi ? eq + 1 : hi;
    *vhi = hi;
    mgf_strip(p, vlo, vhi);
}

// a header line's stripped range -> [*klo, *khi): the stripped key before the first '='; [*vlo, *vhi): the stripped value behind it
__host__ __device__ __forceinline__ void mgf_split(const uint8_t* p, int lo, int hi, int* klo, int* khi, int* vlo, int* vhi) {
    mgf_split_at<'='>(p, lo, hi, klo, khi, vlo, vhi);
}

// a header line's stripped range -> MGF_KEY_*; [*vlo, *vhi): the stripped value behind the first '='
__host__ __device__ __forceinline__ int mgf_header(const uint8_t* p, int lo, int hi, int* vlo, int* vhi) {
    int klo, khi;
    mgf_split(p, lo, hi, &klo, &khi, vlo, vhi);
    const uint8_t* k = p + klo;
    const int n = khi - klo;
    if (mgf_equals(k, n, "title", 5, true)) return MGF_KEY_TITLE;
    if (mgf_equals(k, n, "pepmass", 7, true)) return MGF_KEY_PEPMASS;
    if (mgf_equals(k, n, "charge", 6, true)) return MGF_KEY_CHARGE;
    if (mgf_equals(k, n, "rtinseconds", 11, true)) return MGF_KEY_RT;
    return MGF_KEY_OTHER;
}

// the next whitespace-separated token of p[*pos, hi) -> [*a, *b) (empty at the end); *pos moves behind it
__host__ __device__ __forceinline__ void mgf_token(const uint8_t* p, int* pos, int hi, int* a, int* b) {
    while (*pos < hi && mgf_space(p[*pos])) ++*pos;
    *a = *pos;
    while (*pos < hi && !mgf_space(p[*pos])) ++*pos;
    *b = *pos;
}

// CHARGE fast form: D+ (at most 9) and at most one '+' or '-' behind them -> sign * int; everything else _parse_charge
// handles ("2+ and 3+", "2,3", "+2"): not decided
__host__ __device__ __forceinline__ bool mgf_parse_charge(const uint8_t* p, int len, int32_t* out) {
    int i = 0;
    int32_t v = 0;
    while (i < len && mgf_digit(p[i])) {
        if (i == 9) return false;
        v = v * 10 + (int32_t)(p[i] - '0');
        ++i;
    }
    if (i == 0) return false;
    bool neg = false;
    if (i < len && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    if (i != len) return false;
    *out = neg ? -v : v;
    return true;
}

__host__ __device__ __forceinline__ uint64_t mgf_pow5(int k) {          // k <= 27
    uint64_t v = 1;
    for (int i = 0; i < k; ++i) v *= 5;
    return v;
}

__host__ __device__ __forceinline__ double mgf_from_bits(uint64_t u) { return __builtin_bit_cast(double, u); }

// (hi 2^64 + lo + a fraction in (0, 1) when sticky) 2^e, hi | lo != 0, inside the normal range -> nearest double, ties to even
__host__ __device__ __forceinline__ double mgf_round128(uint64_t hi, uint64_t lo, bool sticky, int e, bool neg) {
    const int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
    uint64_t mant;
    int shift = top - 52;
    if (shift <= 0) {
        mant = lo << -shift;
    } else {
        const int s = shift - 1;                      // v = the top 54 bits; the last one is the rounding bit
        uint64_t v;
        if (s >= 64) {
            sticky |= lo != 0 || (s > 64 && (hi & ((uint64_t(1) << (s - 64)) - 1)) != 0);
            v = hi >> (s - 64);
        } else if (s == 0) {
            v = lo;
        } else {
            sticky |= (lo & ((uint64_t(1) << s) - 1)) != 0;
            v = (lo >> s) | (hi << (64 - s));
        }
        mant = v >> 1;
        if ((v & 1) && (sticky || (mant & 1))) ++mant;
        if (mant >> 53) {
            mant >>= 1;
            ++shift;
        }
    }
    const uint64_t bits = ((uint64_t)(1023 + 52 + e + shift) << 52) | (mant & ((uint64_t(1) << 52) - 1));
    return mgf_from_bits(bits | (neg ? uint64_t(1) << 63 : 0));
}

// float(token), or false: not decided
__host__ __device__ __forceinline__ bool mgf_parse_double(const uint8_t* p, int len, double* out) {
    int i = 0;
    bool neg = false;
    if (i < len && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    uint64_t w = 0;
    int sig = 0, digits = 0, frac = 0;
    bool many = false;
    for (int part = 0; part < 2; ++part) {
        while (i < len && mgf_digit(p[i])) {
            const uint32_t d = p[i] - '0';
            ++digits;
            frac += part;
            if (w != 0 || d != 0) {
                if (sig == 19) many = true;
                else {
                    w = w * 10 + d;
                    ++sig;
                }
            }
            ++i;
        }
        if (part == 0) {
            if (i < len && p[i] == '.') ++i;
            else break;
        }
    }
    if (digits == 0 || many) return false;
    int ex = 0;
    if (i < len && (p[i] == 'e' || p[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < len && (p[i] == '+' || p[i] == '-')) eneg = p[i++] == '-';
        int ed = 0;
        while (i < len && mgf_digit(p[i])) {
            if (ex < 100000) ex = ex * 10 + (int)(p[i] - '0');
            ++ed;
            ++i;
        }
        if (ed == 0) return false;
        if (eneg) ex = -ex;
    }
    if (i != len) return false;
    if (w == 0) {
        *out = neg ? -0.0 : 0.0;
        return true;
    }
    if (frac > 100000) return false;
    const int q = ex - frac;
    if (q < -27 || q > 27) return false;
    const int k = q < 0 ? -q : q;
    const uint64_t p5 = mgf_pow5(k);
    if (w <= (uint64_t(1) << 53) && k <= 22) {                                     // Clinger: both operands exact
        const double x = (double)w, t = (double)p5 * mgf_from_bits((uint64_t)(1023 + k) << 52);
        const double r = q < 0 ? x / t : x * t;
        *out = neg ? -r : r;
        return true;
    }
    if (q >= 0) {
        uint64_t hi, lo;
        num_mul128(w, p5, &hi, &lo);
        *out = mgf_round128(hi, lo, false, q, neg);
        return true;
    }
    const int lz = __builtin_clzll(w);
    const uint64_t wn = w << lz;                                                   // w 2^lz, top bit set: the quotient has >= 65 bits
    const uint64_t qhi = wn / p5;
    uint64_t rem = wn % p5, qlo = 0;
    for (int b = 0; b < 64; ++b) {                                                 // rem < 5^27 < 2^63: the shift cannot overflow
        rem <<= 1;
        qlo <<= 1;
        if (rem >= p5) {
            rem -= p5;
            qlo |= 1;
        }
    }
    *out = mgf_round128(qhi, qlo, rem != 0, -64 - lz - k, neg);
    return true;
}

}  // namespace fal
