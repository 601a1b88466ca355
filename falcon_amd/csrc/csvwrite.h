// Cluster CSV out of the device: the pure functions of the writer -- the row order's comparator, the number text, the quoting and
// the row layout.  Shared by csvwrite.hip's kernels and the host build of the CPU tests (tests/hostbuild_csvwrite.py); they mirror
// falcon_amd/falcon.py's `_natural_key` and `_write_cluster_info`, which stay the order and the writer of record: for the same
// rows the bytes are the same.
//
// Order.  csv_natural_cmp compares two ASCII byte strings as `_natural_key` does: `re.split(r"(\d+)")` cuts a string into text
// run, digit run, text run, ..., first and last a text run that may be empty.  Text runs compare as whole byte strings (a proper
// prefix is smaller: "a1" < "a!" because "a" < "a!"), a string that ends behind equal runs is smaller than one that goes on, and
// digit runs compare as integers of any length (leading zeros dropped, then the longer is larger, then bytewise).  Keys that
// differ only in leading zeros are equal: 0.
//
// Numbers.  A float32 x becomes the bytes of str(np.float32(x)): the shortest digits inside the float32's own rounding interval
// (numtext.h's num_shortest_f32), in numpy's layout.
//   layout : positional when 1e-4 <= |x| < 1e16 as doubles ("0.0001", "12.5", "9999999000000000.0"), otherwise d[.ddd]e[+-]XX;
//            the float32 nearest 1e-4 lies below it ("1e-04"), the one nearest 1e16 above it ("1e+16").  "nan", "inf", "-inf",
//            "0.0", "-0.0".
//   length : at most 9 digits; the longest text is sign + 16 digits + ".0" = 19 bytes = kCsvNumMax.
//
// Fields are csv.QUOTE_MINIMAL's: a field with ',', '"' or '\n' -- and '\r' where the running interpreter's csv module quotes it
// (CPython 3.13 on; before, a bare '\r' stays as it is with the line terminator "\n"): `quote_cr` -- goes in quotes with its quotes
// doubled.  A row is <filename>,<spectrum_id>,<charge>,<precursor_mz>,<retention_time>,<cluster>\n; charge 0 prints None.
#pragma once
#include <stdint.h>
#include "numtext.h"

namespace fal {

constexpr int kCsvNumMax = 19;                       // bytes of one number, at most
constexpr int kCsvChargeMax = 11;                    // "-2147483648"
constexpr int kCsvClusterMax = 20;                   // "-9223372036854775808"
constexpr int kCsvFixedMax = kCsvChargeMax + 2 * kCsvNumMax + kCsvClusterMax + 6;   // a row without its two text fields

__host__ __device__ __forceinline__ bool csv_is_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }

// -1 / 0 / 1: the order of falcon._natural_key over ASCII bytes
__host__ __device__ inline int csv_natural_cmp(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb) {
    int64_t i = 0, j = 0;
    for (;;) {
        for (;;) {                                               // text runs: byte strings, the proper prefix first
            const bool ea = i >= la || csv_is_digit(a[i]), eb = j >= lb || csv_is_digit(b[j]);
            if (ea || eb) {
                if (ea != eb) return ea ? -1 : 1;
                break;
            }
            if (a[i] != b[j]) return a[i] < b[j] ? -1 : 1;
            ++i;
            ++j;
        }
        const bool enda = i >= la, endb = j >= lb;               // equal text runs: the string that ends is smaller
        if (enda || endb) return enda == endb ? 0 : enda ? -1 : 1;
        while (i < la && a[i] == '0') ++i;                       // digit runs: integers of any length
        while (j < lb && b[j] == '0') ++j;
        int64_t i1 = i, j1 = j;
        while (i1 < la && csv_is_digit(a[i1])) ++i1;
        while (j1 < lb && csv_is_digit(b[j1])) ++j1;
        if (i1 - i != j1 - j) return i1 - i < j1 - j ? -1 : 1;
        for (; i < i1; ++i, ++j)
            if (a[i] != b[j]) return a[i] < b[j] ? -1 : 1;
    }
}

// the longest run of digits (what int() of the host key has to take)
__host__ __device__ inline int64_t csv_max_digit_run(const uint8_t* a, int64_t la) {
    int64_t best = 0, run = 0;
    for (int64_t i = 0; i < la; ++i) {
        run = csv_is_digit(a[i]) ? run + 1 : 0;
        best = run > best ? run : best;
    }
    return best;
}

// a number made ready once: its length and its text come from the same digits
struct CsvNum {
    NumDecimal d;
    int kind;                    // 0: digits, 1: zero, 2: inf, 3: nan
    bool neg, positional;
};

__host__ __device__ __forceinline__ CsvNum csv_num(float x) {
    const uint32_t bits = num_float_bits(x);
    CsvNum v;
    v.d.digits = 0;
    v.d.n = v.d.decpt = 0;
    v.neg = bits >> 31;
    v.positional = true;
    if ((bits & 0x7F800000u) == 0x7F800000u) {
        v.kind = (bits & 0x7FFFFFu) ? 3 : 2;
        if (v.kind == 3) v.neg = false;
    } else if ((bits & 0x7FFFFFFFu) == 0) {
        v.kind = 1;
    } else {
        v.kind = 0;
        v.d = num_shortest_f32(bits);
        const double a = (double)__builtin_bit_cast(float, bits & 0x7FFFFFFFu);
        v.positional = a >= 1e-4 && a < 1e16;
    }
    return v;
}

__host__ __device__ __forceinline__ int csv_num_len(const CsvNum& v) {
    return (int)v.neg + (v.kind ? 3 : num_decimal_len(v.d, v.positional));
}

// (room for kCsvNumMax bytes) -> the length
__host__ __device__ __forceinline__ int csv_write_num(uint8_t* dst, const CsvNum& v) {
    int at = 0;
    if (v.neg) dst[at++] = '-';
    if (v.kind == 0) return at + num_write_decimal(dst + at, v.d, v.positional);
    const char* w = v.kind == 1 ? "0.0" : v.kind == 2 ? "inf" : "nan";
    return at + num_put(dst + at, w, 3);
}

__host__ __device__ __forceinline__ int csv_num_len(float x) { return csv_num_len(csv_num(x)); }
__host__ __device__ __forceinline__ int csv_write_num(uint8_t* dst, float x) { return csv_write_num(dst, csv_num(x)); }

// bytes of a field under csv.QUOTE_MINIMAL: n when it is copied as it is, n + 2 + its quotes otherwise
__host__ __device__ inline int64_t csv_field_len(const uint8_t* p, int64_t n, bool quote_cr) {
    int64_t quotes = 0;
    bool special = false;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t c = p[i];
        quotes += c == '"';
        special |= c == ',' || c == '"' || c == '\n' || (quote_cr && c == '\r');
    }
    return special ? n + 2 + quotes : n;
}

// the field at dst, `len` its csv_field_len -> len
__host__ __device__ inline int64_t csv_write_field(uint8_t* dst, const uint8_t* p, int64_t n, int64_t len) {
    if (len == n) {
        for (int64_t i = 0; i < n; ++i) dst[i] = p[i];
        return n;
    }
    int64_t at = 0;
    dst[at++] = '"';
    for (int64_t i = 0; i < n; ++i) {
        if (p[i] == '"') dst[at++] = '"';
        dst[at++] = p[i];
    }
    dst[at++] = '"';
    return at;
}

// one row with its numbers made ready and its text fields measured (fn_len / id_len: csv_field_len of the two)
struct CsvRow {
    const uint8_t* fn;
    const uint8_t* id;
    int64_t fn_n, id_n, fn_len, id_len;
    int32_t charge;
    int64_t cluster;
    CsvNum pm, rt;
};

__host__ __device__ inline CsvRow csv_row(const uint8_t* fn, int64_t fn_n, const uint8_t* id, int64_t id_n, int32_t charge, float pm, float rt,
                                          int64_t cluster, bool quote_cr) {
    CsvRow r;
    r.fn = fn;
    r.id = id;
    r.fn_n = fn_n;
    r.id_n = id_n;
    r.fn_len = csv_field_len(fn, fn_n, quote_cr);
    r.id_len = csv_field_len(id, id_n, quote_cr);
    r.charge = charge;
    r.cluster = cluster;
    r.pm = csv_num(pm);
    r.rt = csv_num(rt);
    return r;
}

__host__ __device__ inline int64_t csv_row_len(const CsvRow& r) {
    return r.fn_len + r.id_len + (r.charge == 0 ? 4 : num_int_len(r.charge)) + csv_num_len(r.pm) + csv_num_len(r.rt) +
           num_int_len(r.cluster) + 6;
}

// the row at dst (room for csv_row_len bytes) -> its length
__host__ __device__ inline int64_t csv_write_row(uint8_t* dst, const CsvRow& r) {
    int64_t at = csv_write_field(dst, r.fn, r.fn_n, r.fn_len);
    dst[at++] = ',';
    at += csv_write_field(dst + at, r.id, r.id_n, r.id_len);
    dst[at++] = ',';
    at += r.charge == 0 ? num_put(dst + at, "None", 4) : num_write_int(dst + at, r.charge);
    dst[at++] = ',';
    at += csv_write_num(dst + at, r.pm);
    dst[at++] = ',';
    at += csv_write_num(dst + at, r.rt);
    dst[at++] = ',';
    at += num_write_int(dst + at, r.cluster);
    dst[at++] = '\n';
    return at;
}

}  // namespace fal
