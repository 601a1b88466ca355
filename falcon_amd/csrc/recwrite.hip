// Columns on the device -> the text of n units, each a record of fields: a head literal, every present field as prefix literal,
// value, suffix literal, and a tail literal.  The caller describes the unit by a table of at most 32 fields (include/falcon_hip.h
// fal_rec_field); the kinds, the absence rule, the number text and the XML character data are recwrite.h's (shared with the CPU
// tests); DESIGN.md "Records of fields out of the device" has the field model and the one file written with it (GraphML).
//
// fal_records_write_sizes (one synchronisation, at its end): a lane per unit adds up its text (textwrite.h's sizes_by_lane), then
// the library's scan turns the sizes into offsets.
//
// fal_records_write (one synchronisation, at its end): a lane per unit, a wave per tile of 64 consecutive units -- textwrite.h's
// write_units_by_lane, which has the rounds, the tile and every bound on a store.  What this unit gives it is RecUnits.  The
// workgroup stages the literal blob in LDS once; the field table is a kernel argument.  A unit that no tile takes is written by
// the whole wave with textwrite.h's pieces: a literal copied lane-strided; a number from lane 0; kRecTextChunk text bytes per lane
// at a wave prefix sum of their character data.
#include <stddef.h>
#include <algorithm>
#include "common.h"
#include "recwrite.h"
#include "textwrite.h"

namespace fal {
namespace {

constexpr int kRecTile = 8192;                   // bytes of a wave's tile; a multiple of 16
constexpr int kRecTextChunk = 16;                // text bytes a lane takes per round of the long-unit path
static_assert(kRecTile % 16 == 0 && kTileCarry + 64 * kRecTextChunk * kRecEntityMax <= kRecTile && kTileCarry + kRecLitMax <= kRecTile &&
                  kTileCarry + kRecNumMax <= kRecTile,
              "the tile takes one piece of a long unit behind what the last flush left");
static_assert(sizeof(RecField) == sizeof(fal_rec_field) && offsetof(RecField, index) == offsetof(fal_rec_field, index) &&
                  offsetof(RecField, blob_bytes) == offsetof(fal_rec_field, blob_bytes) && offsetof(RecField, kind) == offsetof(fal_rec_field, kind) &&
                  offsetof(RecField, suffix) == offsetof(fal_rec_field, suffix),
              "recwrite.h's RecField is the header's fal_rec_field");
static_assert(kRecMaxFields == FAL_REC_MAX_FIELDS && kRecLitMax == FAL_REC_MAX_LITERALS && REC_I32 == FAL_REC_I32 && REC_I64 == FAL_REC_I64 &&
                  REC_F32 == FAL_REC_F32 && REC_TEXT == FAL_REC_TEXT,
              "the header states the limits and the kinds");

// kRecTextChunk text bytes per lane as character data, 64 lanes a piece (p, n: the same in every lane)
__device__ __forceinline__ void tile_append_xml(Tile& t, const uint8_t* p, int64_t n, int lane) {
    for (int64_t c = 0; c < n; c += 64 * kRecTextChunk) {
        const int64_t a = std::min<int64_t>(c + (int64_t)lane * kRecTextChunk, n), b = std::min<int64_t>(a + kRecTextChunk, n);
        int len = 0;
        for (int64_t i = a; i < b; ++i) len += rec_xml_byte_len(p[i]);
        tile_append_by_lanes(t, len, lane, [&](uint8_t* dst) {
            for (int64_t i = a; i < b; ++i) dst += rec_xml_write_byte(dst, p[i]);
        });
    }
}

// ---- the units as textwrite.h's lane-per-unit writers take them ----------------------------------------------------------------------------
struct RecUnits {
    typedef int64_t Unit;                                                        // the unit's length: a lane formats from the columns again
    static constexpr bool kLongByWave = true;
    const RecTable& t;
    const uint8_t* lit;                                                          // the literal blob (in LDS; the sizes need none)
    __device__ int64_t load(int64_t k, bool* bad) const { return rec_unit_len(t, k, bad); }
    __device__ int64_t len(int64_t unit) const { return unit; }
    __device__ int64_t write(uint8_t* dst, int64_t, int64_t k) const { return rec_write_unit(dst, t, lit, k); }
    __device__ void literal(Tile& text, const int32_t* range, int lane) const {
        tile_append_bytes<kRecLitMax>(text, lit + range[0], range[1] - range[0], lane);
    }
    // a unit that no tile takes: the whole wave writes it, piece after piece through the tile
    __device__ void long_unit(uint8_t* tile, uint8_t* dst, int64_t len, int64_t k, unsigned long long* meta) const {
        const int lane = threadIdx.x & 63;
        Tile text = tile_open(tile, dst, dst + len);
        literal(text, t.head, lane);
        for (int j = 0; j < t.n_fields; ++j) {
            bool unused = false;
            const RecValue v = rec_load(t.f[j], k, &unused);                    // (unit k in every lane)
            if (!v.present) continue;
            literal(text, t.f[j].prefix, lane);
            if (v.kind == REC_TEXT) tile_append_xml(text, v.p, v.n, lane);
            else tile_append_by_lane0(text, (int)rec_value_len(v), lane, [&](uint8_t* d) { rec_write_number(d, v); });
            literal(text, t.f[j].suffix, lane);
        }
        literal(text, t.tail, lane);
        tile_close(text, lane, meta);
    }
};

__global__ __launch_bounds__(256) void rec_write_sizes_kernel(RecTable t, int64_t n, int64_t* __restrict__ sizes,
                                                              unsigned long long* __restrict__ meta) {
    sizes_by_lane(RecUnits{t, nullptr}, n, sizes, meta);
}

__global__ __launch_bounds__(256) void rec_write_kernel(RecTable t, const uint8_t* __restrict__ literals, int lit_bytes,
                                                        const int64_t* __restrict__ offsets, int64_t first, int64_t last,
                                                        uint8_t* __restrict__ out, int64_t out_bytes, unsigned long long* __restrict__ meta) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4][kRecTile];
    __shared__ __attribute__((aligned(16))) uint8_t lit[kRecLitMax];
    for (int i = threadIdx.x; i < lit_bytes; i += blockDim.x) lit[i] = literals[i];              // (lit_bytes <= kRecLitMax: the host checked)
    __syncthreads();
    write_units_by_lane<kRecTile>(RecUnits{t, lit}, tiles[threadIdx.x >> 6], offsets, first, last, out, out_bytes, meta);
}

FAL_WARM_KERNEL(rec_write_kernel);

bool range_ok(const int32_t* r, int64_t literal_bytes) { return r[0] >= 0 && r[0] <= r[1] && r[1] <= literal_bytes; }

// the caller's table, checked -> the kernels' argument
int make_table(const char* who, fal_ctx* ctx, int64_t n, const fal_rec_field* fields, int n_fields, const uint8_t* literals,
               int64_t literal_bytes, int head_begin, int head_end, int tail_begin, int tail_end, RecTable* t) {
    FAL_REQUIRE(ctx && n >= 0, FAL_EINVAL, "%s: bad argument", who);
    FAL_REQUIRE(n_fields >= 0 && n_fields <= kRecMaxFields && (fields || n_fields == 0), FAL_EINVAL, "%s: %d fields (at most %d)", who,
                n_fields, kRecMaxFields);
    FAL_REQUIRE(literal_bytes >= 0 && literal_bytes <= kRecLitMax && (literals || literal_bytes == 0), FAL_EINVAL,
                "%s: %lld bytes of literals (at most %d)", who, (long long)literal_bytes, kRecLitMax);
    *t = RecTable();
    t->n_fields = n_fields;
    t->head[0] = head_begin, t->head[1] = head_end, t->tail[0] = tail_begin, t->tail[1] = tail_end;
    FAL_REQUIRE(range_ok(t->head, literal_bytes) && range_ok(t->tail, literal_bytes), FAL_EINVAL,
                "%s: the head or the tail lies outside the literal blob", who);
    for (int j = 0; j < n_fields; ++j) {
        const fal_rec_field& f = fields[j];
        RecField& g = t->f[j];
        g.column = f.column, g.ptr = f.ptr, g.index = f.index, g.rows = f.rows, g.blob_bytes = f.blob_bytes, g.kind = f.kind;
        for (int i = 0; i < 2; ++i) g.prefix[i] = f.prefix[i], g.suffix[i] = f.suffix[i];
        FAL_REQUIRE(f.kind >= REC_I32 && f.kind <= REC_TEXT && f.rows >= 0 && f.blob_bytes >= 0, FAL_EINVAL, "%s: field %d: bad kind or size",
                    who, j);
        FAL_REQUIRE(range_ok(g.prefix, literal_bytes) && range_ok(g.suffix, literal_bytes), FAL_EINVAL,
                    "%s: field %d: a literal range outside the literal blob", who, j);
        FAL_REQUIRE(f.index || f.rows >= n, FAL_EINVAL, "%s: field %d: %lld rows for %lld units and no index", who, j, (long long)f.rows,
                    (long long)n);
        if (f.kind == REC_TEXT) FAL_REQUIRE(f.ptr && (f.column || f.blob_bytes == 0), FAL_EINVAL, "%s: field %d: NULL text column", who, j);
        else FAL_REQUIRE(f.column || f.rows == 0, FAL_EINVAL, "%s: field %d: NULL column", who, j);
    }
    return FAL_OK;
}

}  // namespace
}  // namespace fal

using namespace fal;

extern "C" int fal_records_write_sizes(fal_ctx* ctx, int64_t n, const fal_rec_field* fields, int n_fields, const uint8_t* literals,
                                       int64_t literal_bytes, int head_begin, int head_end, int tail_begin, int tail_end, int64_t* sizes_out,
                                       int64_t* offsets_out, int64_t* total_out) {
    fal::CallScope _call(ctx);
    RecTable t;
    FAL_TRY(make_table("fal_records_write_sizes", ctx, n, fields, n_fields, literals, literal_bytes, head_begin, head_end, tail_begin,
                       tail_end, &t));
    FAL_REQUIRE(offsets_out && total_out && (n == 0 || sizes_out), FAL_EINVAL, "fal_records_write_sizes: NULL output");
    *total_out = 0;
    if (n == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(offsets_out, 0, sizeof(int64_t), ctx->stream));
        return FAL_OK;
    }
    unsigned long long* meta = nullptr;
    FAL_TRY(writer_meta(ctx, SLOT_RECW, &meta));
    hipLaunchKernelGGL(rec_write_sizes_kernel, dim3(capped_grid(ctx, n, 256)), dim3(256), 0, ctx->stream, t, n, sizes_out, meta);
    return finish_sizes(ctx, meta, sizes_out, n, offsets_out, total_out,
                        "fal_records_write_sizes: an index at or beyond its column's length, a text row whose bytes do not ascend inside "
                        "the blob, or a text byte below 0x20 that is no tab, line feed or carriage return");
}

extern "C" int fal_records_write(fal_ctx* ctx, int64_t n, const fal_rec_field* fields, int n_fields, const uint8_t* literals,
                                 int64_t literal_bytes, int head_begin, int head_end, int tail_begin, int tail_end, const int64_t* offsets,
                                 int64_t first, int64_t last, uint8_t* out, int64_t out_bytes, uint8_t* host_out) {
    fal::CallScope _call(ctx);
    RecTable t;
    FAL_TRY(make_table("fal_records_write", ctx, n, fields, n_fields, literals, literal_bytes, head_begin, head_end, tail_begin, tail_end, &t));
    FAL_REQUIRE(offsets && first >= 0 && first <= last && last <= n && out_bytes >= 0 && (out || out_bytes == 0), FAL_EINVAL,
                "fal_records_write: bad argument");
    unsigned long long* meta = nullptr;
    FAL_TRY(writer_meta(ctx, SLOT_RECW, &meta));
    hipLaunchKernelGGL(rec_write_kernel, dim3(capped_grid(ctx, ceil_div(std::max<int64_t>(last - first, 1), (int64_t)64), 4)), dim3(256), 0,
                       ctx->stream, t, literals, (int)literal_bytes, offsets, first, last, out, out_bytes, meta);
    return finish_write(ctx, meta, "fal_records_write", "units", "a unit", first, last, out, out_bytes, host_out);
}
