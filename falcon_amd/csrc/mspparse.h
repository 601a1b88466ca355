// MSP library text on the device: the pure per-line functions of the reader -- line kind, the split at the first ':', the
// peak segments of a line and the Num Peaks fast form.  Shared by mspparse.hip's kernels and the host build of the CPU tests
// (tests/hostbuild_msp.py); they mirror falcon_amd/ms_io/msp_io.py, which stays the reader of record: whatever these functions
// do not decide is decided by that reader on the host.  The grammar is DESIGN.md's "MSP on the device".  Numbers and charges
// are mgfparse.h's (mgf_parse_double, mgf_parse_charge); whitespace is its space, tab, CR, LF.
//
// Lines.  A line is `key: value`: the key is what stands before the first ':', stripped, compared without case.  A line longer
// than kMgfMaxLine bytes (stripped) that is not blank carries MSP_LONG: its entry goes to the host reader.
// Peak text.  What stands before a line's first '"' is split at ';'; every segment that is non-empty after stripping is one
// peak: its first two whitespace-separated tokens are m/z and intensity.
#pragma once
#include <stdint.h>
#include "mgfparse.h"

namespace fal {

enum { MSP_BLANK = 0, MSP_NAME = 1, MSP_NUMPEAKS = 2, MSP_HEADER = 3, MSP_OTHER = 4, MSP_KIND = 7, MSP_LONG = 8 };
static_assert((int)MSP_LONG == (int)MGF_LONG, "the header pass (textkeys.h) reads the long bit of either reader's line classes");

// a line's stripped range [lo, hi) -> [*klo, *khi): the stripped key before the first ':'; [*vlo, *vhi): the stripped value behind
// it; false: the line has no ':' (the key range is then the line, the value empty)
__host__ __device__ __forceinline__ bool msp_split(const uint8_t* p, int lo, int hi, int* klo, int* khi, int* vlo, int* vhi) {
    int c = lo;
    while (c < hi && p[c] != ':') ++c;
    mgf_split_at<':'>(p, lo, hi, klo, khi, vlo, vhi);
    return c < hi;
}

// one line (without its '\n') -> MSP_* kind, MSP_LONG added; *lo / *hi: the stripped range
__host__ __device__ __forceinline__ int msp_classify(const uint8_t* p, int len, int* lo, int* hi) {
    *lo = 0;
    *hi = len;
    mgf_strip(p, lo, hi);
    const int n = *hi - *lo;
    if (n == 0) return MSP_BLANK;
    int klo, khi, vlo, vhi, kind = MSP_OTHER;
    if (msp_split(p, *lo, *hi, &klo, &khi, &vlo, &vhi)) {
        kind = MSP_HEADER;
        if (mgf_equals(p + klo, khi - klo, "name", 4, true)) kind = MSP_NAME;
        else if (mgf_equals(p + klo, khi - klo, "num peaks", 9, true)) kind = MSP_NUMPEAKS;
    }
    return kind | (n > kMgfMaxLine ? MSP_LONG : 0);
}

// the end of a line's peak text: the position of the first '"' of p[lo, hi), hi when there is none
__host__ __device__ __forceinline__ int msp_peak_end(const uint8_t* p, int lo, int hi) {
    int q = lo;
    while (q < hi && p[q] != '"') ++q;
    return q;
}

// the next peak segment of p[*pos, end) -- end = msp_peak_end -- that is non-empty after stripping -> its stripped range
// [*a, *b), *pos behind its ';'; false: no further one
__host__ __device__ __forceinline__ bool msp_segment(const uint8_t* p, int* pos, int end, int* a, int* b) {
    while (*pos < end) {
        int s = *pos, e = s;
        while (e < end && p[e] != ';') ++e;
        *pos = e < end ? e + 1 : end;
        mgf_strip(p, &s, &e);
        if (e > s) {
            *a = s;
            *b = e;
            return true;
        }
    }
    return false;
}

// the peaks of one line (without its '\n'): its non-empty segments
__host__ __device__ __forceinline__ int msp_segments(const uint8_t* p, int len) {
    const int end = msp_peak_end(p, 0, len);
    int pos = 0, a, b, cnt = 0;
    while (msp_segment(p, &pos, end, &a, &b)) ++cnt;
    return cnt;
}

// a peak segment's stripped range [a, b) -> the token ranges of m/z [*t0, *t1) and intensity [*u0, *u1) (empty: absent)
__host__ __device__ __forceinline__ void msp_peak_tokens(const uint8_t* p, int a, int b, int* t0, int* t1, int* u0, int* u1) {
    int pos = a;
    mgf_token(p, &pos, b, t0, t1);
    mgf_token(p, &pos, b, u0, u1);
}

// Num Peaks fast form D{1,9} -> int(value); everything else int() may accept or reject ("+3", "3 4", "1_0", 10 digits): not decided
__host__ __device__ __forceinline__ bool msp_parse_count(const uint8_t* p, int len, int32_t* out) {
    if (len < 1 || len > 9) return false;
    int32_t v = 0;
    for (int i = 0; i < len; ++i) {
        if (!mgf_digit(p[i])) return false;
        v = v * 10 + (int32_t)(p[i] - '0');
    }
    *out = v;
    return true;
}

}  // namespace fal
