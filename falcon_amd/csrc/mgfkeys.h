// MGF header values by a caller's key table: the pure per-line functions of fal_mgf_headers -- the table key of a header line
// and the integer fast form.  Shared by mgfparse.hip's kernel and the host build of the CPU tests
// (tests/hostbuild_mgf_headers.py).  The key rule is mgf_header()'s (mgfparse.h) and DESIGN.md "MGF on the device": the key is
// what stands before the first '=', stripped, compared without case; the value is what stands behind it, stripped.
#pragma once
#include <stdint.h>
#include "mgfparse.h"

namespace fal {

constexpr int kMgfMaxKeys = 16;          // FAL_MGF_MAX_KEYS
constexpr int kMgfMaxKeyBytes = 32;      // FAL_MGF_MAX_KEY_BYTES
enum { MGF_VAL_SPAN = 0, MGF_VAL_INT = 1 };                          // FAL_MGF_KEY_SPAN / FAL_MGF_KEY_INT
enum { MGF_STATE_ABSENT = 0, MGF_STATE_PRESENT = 1, MGF_STATE_HOST = 2 };

// the table as the kernel takes it: key k is bytes[k][0 .. len[k]), lower-case ASCII
struct MgfKeyTable {
    uint8_t bytes[kMgfMaxKeys][kMgfMaxKeyBytes];
    int32_t len[kMgfMaxKeys];
    int32_t kind[kMgfMaxKeys];
    int32_t n;
};

// the stripped key p[0, n) of a header line -> its index in the table, -1: none of them
__host__ __device__ __forceinline__ int mgf_table_key(const uint8_t* p, int n, const uint8_t (*keys)[kMgfMaxKeyBytes],
                                                      const int32_t* len, int n_keys) {
    if (n < 1 || n > kMgfMaxKeyBytes) return -1;
    for (int k = 0; k < n_keys; ++k)
        if (len[k] == n && mgf_equals(p, n, reinterpret_cast<const char*>(keys[k]), n, true)) return k;
    return -1;
}

// integer fast form [+-]?D{1,18} -> int(value); everything else int() may accept or reject ("1_0", "1 2", 19 digits, "0x5",
// other digits than ASCII's): not decided
__host__ __device__ __forceinline__ bool mgf_parse_int(const uint8_t* p, int len, int64_t* out) {
    int i = 0;
    bool neg = false;
    if (i < len && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    const int digits = len - i;
    if (digits < 1 || digits > 18) return false;
    int64_t v = 0;
    for (; i < len; ++i) {
        if (!mgf_digit(p[i])) return false;
        v = v * 10 + (int64_t)(p[i] - '0');
    }
    *out = neg ? -v : v;
    return true;
}

}  // namespace fal
