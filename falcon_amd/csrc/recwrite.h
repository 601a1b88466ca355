// Records of fields out of the device: the pure functions of the record writer -- a field's value made ready, its length, its
// text, XML character data, and a whole unit.  Shared by recwrite.hip's kernels and the host build of the CPU tests
// (tests/hostbuild_records.py).  falcon_amd/ms_io/graphml_io.py's `node_units` / `edge_units` are the writer of record of the one
// file written with them so far: for the same columns the bytes are the same.
//
// A unit's text is the table's head literal, every present field in turn -- prefix literal, value, suffix literal -- and the tail
// literal.  Unit u reads row index[u] of a field's column, row u without an index.  A field is absent, and contributes nothing,
// when its index is negative, when its float32 is not finite or when its text is empty.  Integers are decimal; a float32 is
// str(np.float32(x)) (csvwrite.h's csv_num); text is XML character data: '&' '<' '>' become "&amp;" "&lt;" "&gt;", '\r' becomes
// "&#13;", '\t', '\n' and every byte from 0x20 up are copied.  A byte below 0x20 other than those three is outside the grammar
// (XML 1.0 forbids it): *bad.  So are an index at or beyond its column's length and a text row whose byte range does not ascend
// inside the blob; such a field counts as absent and nothing outside an array is read.
#pragma once
#include <stdint.h>
#include "csvwrite.h"

namespace fal {

enum { REC_I32 = 0, REC_I64 = 1, REC_F32 = 2, REC_TEXT = 3 };      // include/falcon_hip.h FAL_REC_*
constexpr int kRecMaxFields = 32;                    // include/falcon_hip.h FAL_REC_MAX_FIELDS
constexpr int kRecLitMax = 4096;                     // bytes of the literal blob, at most (FAL_REC_MAX_LITERALS)
constexpr int kRecNumMax = 20;                       // bytes of one number, at most: "-9223372036854775808" (a float32: kCsvNumMax)
constexpr int kRecEntityMax = 5;                     // bytes one text byte becomes, at most: "&amp;", "&#13;"
static_assert(kRecNumMax >= kCsvNumMax && kRecNumMax >= kCsvClusterMax, "a number's room");

// the layout of include/falcon_hip.h's fal_rec_field (recwrite.hip asserts it)
struct RecField {
    const void* column;          // i32 / i64 / f32 [rows], or the text blob u8[blob_bytes]
    const int64_t* ptr;          // text: i64[rows + 1], row r's bytes [ptr[r], ptr[r + 1])
    const int32_t* index;        // i32[n]: unit u reads row index[u], negative: absent; NULL: row u
    int64_t rows, blob_bytes;
    int32_t kind;
    int32_t prefix[2], suffix[2];    // [begin, end) of the literal blob
};

struct RecTable {
    RecField f[kRecMaxFields];
    int32_t n_fields;
    int32_t head[2], tail[2];
};

// ---- XML character data ---------------------------------------------------------------------------------------------------------------
// bytes of the text of one byte; 0: outside the grammar
__host__ __device__ __forceinline__ int rec_xml_byte_len(uint8_t c) {
    if (c >= 0x20) return c == '&' ? 5 : (c == '<' || c == '>') ? 4 : 1;
    return c == '\r' ? 5 : (c == '\t' || c == '\n') ? 1 : 0;
}

// the text of one byte at dst (room for kRecEntityMax bytes) -> its length (a byte outside the grammar: nothing)
__host__ __device__ __forceinline__ int rec_xml_write_byte(uint8_t* dst, uint8_t c) {
    switch (c) {
        case '&': return num_put(dst, "&amp;", 5);
        case '<': return num_put(dst, "&lt;", 4);
        case '>': return num_put(dst, "&gt;", 4);
        case '\r': return num_put(dst, "&#13;", 5);
        default: break;
    }
    if (c < 0x20 && c != '\t' && c != '\n') return 0;
    dst[0] = c;
    return 1;
}

__host__ __device__ inline int64_t rec_xml_len(const uint8_t* p, int64_t n, bool* bad) {
    int64_t len = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int b = rec_xml_byte_len(p[i]);
        if (b == 0) *bad = true;
        len += b;
    }
    return len;
}

__host__ __device__ inline int64_t rec_xml_write(uint8_t* dst, const uint8_t* p, int64_t n) {
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) at += rec_xml_write_byte(dst + at, p[i]);
    return at;
}

// ---- a field's value --------------------------------------------------------------------------------------------------------------------
// made ready once: the length and the text come from the same digits and the same byte range
struct RecValue {
    int kind;                    // REC_*; REC_I32 is held as REC_I64
    bool present;
    int64_t i;
    CsvNum num;
    const uint8_t* p;            // text: the row's bytes and the length of their character data
    int64_t n, text_len;
};

// unit u's value of field f; *bad as the head comment states (then absent)
__host__ __device__ inline RecValue rec_load(const RecField& f, int64_t u, bool* bad) {
    RecValue v;
    v.kind = f.kind == REC_I32 ? (int)REC_I64 : (int)f.kind;
    v.present = false;
    v.i = 0;
    v.num = CsvNum();
    v.p = nullptr;
    v.n = v.text_len = 0;
    int64_t r = u;
    if (f.index) {
        r = f.index[u];
        if (r < 0) return v;
    }
    if (r >= f.rows) {
        *bad = true;
        return v;
    }
    switch (f.kind) {
        case REC_I32:
            v.i = static_cast<const int32_t*>(f.column)[r];
            v.present = true;
            break;
        case REC_I64:
            v.i = static_cast<const int64_t*>(f.column)[r];
            v.present = true;
            break;
        case REC_F32: {
            const float x = static_cast<const float*>(f.column)[r];
            v.present = (num_float_bits(x) & 0x7F800000u) != 0x7F800000u;
            if (v.present) v.num = csv_num(x);
            break;
        }
        case REC_TEXT: {
            const int64_t a = f.ptr[r], b = f.ptr[r + 1];
            if (a < 0 || b < a || b > f.blob_bytes) {
                *bad = true;
                return v;
            }
            bool outside = false;
            v.p = static_cast<const uint8_t*>(f.column) + a;
            v.n = b - a;
            v.text_len = rec_xml_len(v.p, v.n, &outside);
            if (outside) *bad = true;
            v.present = v.n > 0 && !outside;
            break;
        }
        default:
            *bad = true;
            break;
    }
    return v;
}

// bytes of a present value's text: the one length function of the sizing call and the write call
__host__ __device__ __forceinline__ int64_t rec_value_len(const RecValue& v) {
    return v.kind == REC_I64 ? num_int_len(v.i) : v.kind == REC_F32 ? csv_num_len(v.num) : v.text_len;
}

// a number's text at dst (room for kRecNumMax bytes) -> its length
__host__ __device__ __forceinline__ int rec_write_number(uint8_t* dst, const RecValue& v) {
    return v.kind == REC_I64 ? num_write_int(dst, v.i) : csv_write_num(dst, v.num);
}

// bytes a field adds to its unit: nothing when absent
__host__ __device__ __forceinline__ int64_t rec_field_len(const RecField& f, const RecValue& v) {
    return v.present ? (f.prefix[1] - f.prefix[0]) + rec_value_len(v) + (f.suffix[1] - f.suffix[0]) : 0;
}

// ---- a unit -----------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int64_t rec_unit_len(const RecTable& t, int64_t u, bool* bad) {
    int64_t len = (t.head[1] - t.head[0]) + (t.tail[1] - t.tail[0]);
    for (int j = 0; j < t.n_fields; ++j) len += rec_field_len(t.f[j], rec_load(t.f[j], u, bad));
    return len;
}

__host__ __device__ __forceinline__ int64_t rec_put_literal(uint8_t* dst, const uint8_t* lit, const int32_t* range) {
    for (int i = range[0]; i < range[1]; ++i) dst[i - range[0]] = lit[i];
    return range[1] - range[0];
}

// unit u at dst (room for rec_unit_len bytes); lit: the literal blob -> its length
__host__ __device__ inline int64_t rec_write_unit(uint8_t* dst, const RecTable& t, const uint8_t* lit, int64_t u) {
    int64_t at = rec_put_literal(dst, lit, t.head);
    for (int j = 0; j < t.n_fields; ++j) {
        bool bad = false;
        const RecValue v = rec_load(t.f[j], u, &bad);
        if (!v.present) continue;
        at += rec_put_literal(dst + at, lit, t.f[j].prefix);
        at += v.kind == REC_TEXT ? rec_xml_write(dst + at, v.p, v.n) : (int64_t)rec_write_number(dst + at, v);
        at += rec_put_literal(dst + at, lit, t.f[j].suffix);
    }
    return at + rec_put_literal(dst + at, lit, t.tail);
}

}  // namespace fal
