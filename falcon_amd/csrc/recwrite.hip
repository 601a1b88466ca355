// Columns on the device -> the text of n units, each a record of fields: a head literal, every present field as prefix literal,
// value, suffix literal, and a tail literal.  The caller describes the unit by a table of at most 32 fields (include/falcon_hip.h
// fal_rec_field); the kinds, the absence rule, the number text and the XML character data are recwrite.h's (shared with the CPU
// tests); DESIGN.md "Records of fields out of the device" has the field model and the one file written with it (GraphML).
//
// fal_records_write_sizes (one synchronisation, at its end): a lane per unit adds up its text, then the library's scan turns the
// sizes into offsets.
//
// fal_records_write (one synchronisation, at its end): csvwrite.hip's shape -- a lane per unit, a wave per tile of 64 consecutive
// units.  The workgroup stages the literal blob in LDS once; the field table is a kernel argument.  A round measures the units
// again, places them in the wave's LDS tile (textwrite.h's Tile around the round's first byte) at a wave prefix sum of their
// lengths -- as many leading units as the tile takes -- the lanes format there and the tile is flushed whole.  A unit that no tile
// takes is written by the whole wave: piece after piece is appended to the tile (a literal; a number; kRecTextChunk text bytes per
// lane at a wave prefix sum of their character data) and the tile's complete 16-byte units are flushed behind every piece.  Every
// unit's length is checked against offsets[k + 1] - offsets[k] and every round's range against [0, offsets[last] -
// offsets[first]] <= out_bytes before anything of it is stored.
#include <stddef.h>
#include <algorithm>
#include "common.h"
#include "recwrite.h"
#include "textwrite.h"

namespace fal {
namespace {

constexpr int kRecTile = 8192;                   // bytes of a wave's tile; a multiple of 16
constexpr int kRecTextChunk = 16;                // text bytes a lane takes per round of the long-unit path
constexpr int kRecCarry = 31;                    // bytes a flush that is not the last may leave in the tile
static_assert(kRecTile % 16 == 0 && kRecCarry + 64 * kRecTextChunk * kRecEntityMax <= kRecTile && kRecCarry + kRecLitMax <= kRecTile &&
                  kRecCarry + kRecNumMax <= kRecTile,
              "the tile takes one piece of a long unit behind what the last flush left");
static_assert(sizeof(RecField) == sizeof(fal_rec_field) && offsetof(RecField, index) == offsetof(fal_rec_field, index) &&
                  offsetof(RecField, blob_bytes) == offsetof(fal_rec_field, blob_bytes) && offsetof(RecField, kind) == offsetof(fal_rec_field, kind) &&
                  offsetof(RecField, suffix) == offsetof(fal_rec_field, suffix),
              "recwrite.h's RecField is the header's fal_rec_field");
static_assert(kRecMaxFields == FAL_REC_MAX_FIELDS && kRecLitMax == FAL_REC_MAX_LITERALS && REC_I32 == FAL_REC_I32 && REC_I64 == FAL_REC_I64 &&
                  REC_F32 == FAL_REC_F32 && REC_TEXT == FAL_REC_TEXT,
              "the header states the limits and the kinds");

// ---- sizes: a lane per unit -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rec_write_sizes_kernel(RecTable t, int64_t n, int64_t* __restrict__ sizes,
                                                              unsigned long long* __restrict__ meta) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    bool any_bad = false;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += step) {
        bool bad = false;
        const int64_t len = rec_unit_len(t, k, &bad);
        sizes[k] = bad ? 0 : len;
        any_bad |= bad;
    }
    if (any_bad) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
}

// ---- the long-unit path: the wave appends pieces to its tile ---------------------------------------------------------------------------
__device__ __forceinline__ void tile_append_literal(Tile& t, const uint8_t* lit, const int32_t* range, int lane) {
    const int m = range[1] - range[0];
    for (int i = lane; i < m; i += 64) t.tile[t.hi + i] = lit[range[0] + i];
    t.hi += m;
    tile_flush(t, false, lane);
}

__device__ __forceinline__ void tile_append_number(Tile& t, const RecValue& v, int lane) {
    if (lane == 0) rec_write_number(t.tile + t.hi, v);
    t.hi += (int)rec_value_len(v);
    tile_flush(t, false, lane);
}

__device__ __forceinline__ void tile_append_xml(Tile& t, const uint8_t* p, int64_t n, int lane) {
    for (int64_t c = 0; c < n; c += 64 * kRecTextChunk) {                        // (n: the same in every lane)
        const int64_t a = std::min<int64_t>(c + (int64_t)lane * kRecTextChunk, n), b = std::min<int64_t>(a + kRecTextChunk, n);
        int len = 0;
        for (int64_t i = a; i < b; ++i) len += rec_xml_byte_len(p[i]);
        const int incl = wave_prefix_sum(len);
        uint8_t* dst = t.tile + t.hi + incl - len;
        for (int64_t i = a; i < b; ++i) dst += rec_xml_write_byte(dst, p[i]);
        t.hi += __shfl(incl, 63, 64);
        tile_flush(t, false, lane);
    }
}

// ---- write: a lane per unit, a wave per tile of 64 units ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rec_write_kernel(RecTable t, const uint8_t* __restrict__ literals, int lit_bytes,
                                                        const int64_t* __restrict__ offsets, int64_t first, int64_t last,
                                                        uint8_t* __restrict__ out, int64_t out_bytes, unsigned long long* __restrict__ meta) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4][kRecTile];
    __shared__ __attribute__((aligned(16))) uint8_t lit[kRecLitMax];
    for (int i = threadIdx.x; i < lit_bytes; i += blockDim.x) lit[i] = literals[i];              // (lit_bytes <= kRecLitMax: the host checked)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint8_t* tile = tiles[threadIdx.x >> 6];
    const int64_t base = offsets[first], need = offsets[last] - base;
    if (need < 0 || need > out_bytes) {                                          // uniform over the grid: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_TOO_SMALL);
        return;
    }
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6), n_tiles = (last - first + 63) / 64;
    for (int64_t w = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); w < n_tiles; w += waves) {
        const int64_t k1 = std::min<int64_t>(first + 64 * (w + 1), last);
        int64_t r = first + 64 * w;
        while (r < k1) {                                                         // (r, k1: the same in every lane)
            const int64_t k = r + lane;
            const bool on = k < k1;
            bool bad = false;
            int64_t len = 0;
            if (on) {
                len = rec_unit_len(t, k, &bad);
                bad |= len != offsets[k + 1] - offsets[k];
            }
            const int64_t g0 = offsets[r] - base;
            if (__ballot(bad) != 0ull || g0 < 0 || g0 > need) {                 // columns or offsets that are not the sizing pass's
                if (lane == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
                break;
            }
            const int mis = (int)(reinterpret_cast<uintptr_t>(out + g0) & 15);
            const int cap = kRecTile - mis;
            const int clen = (int)std::min<int64_t>(len, kRecTile + 1);         // (64 of them stay far below 2^31)
            const int incl = wave_prefix_sum(clen);
            const int cnt = __popcll(__ballot(on && incl <= cap));              // the leading units the tile takes (incl ascends)
            if (cnt == 0) {                                                      // unit r alone is longer than a tile: the whole wave writes it
                const int64_t len0 = __shfl((long long)len, 0, 64);
                if (g0 + len0 > need) {
                    if (lane == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
                    break;
                }
                Tile text{tile, out + g0 - mis, out + g0 + len0, mis, mis, false};
                tile_append_literal(text, lit, t.head, lane);
                for (int j = 0; j < t.n_fields; ++j) {
                    bool unused = false;
                    const RecValue v = rec_load(t.f[j], r, &unused);            // (unit r in every lane)
                    if (!v.present) continue;
                    tile_append_literal(text, lit, t.f[j].prefix, lane);
                    if (v.kind == REC_TEXT) tile_append_xml(text, v.p, v.n, lane);
                    else tile_append_number(text, v, lane);
                    tile_append_literal(text, lit, t.f[j].suffix, lane);
                }
                tile_append_literal(text, lit, t.tail, lane);
                tile_flush(text, true, lane);
                const bool shortfall = text.gbase + text.hi != text.end;         // (less text than the sizes said)
                if (lane == 0 && (text.overflow || shortfall)) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_OVERFLOW);
                wave_lds_sync();
                r += 1;
                continue;
            }
            const int total = __shfl(incl, cnt - 1, 64);
            if (g0 + total > need) {
                if (lane == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
                break;
            }
            if (lane < cnt && rec_write_unit(tile + mis + incl - clen, t, lit, k) != len) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_OVERFLOW);
            Tile text{tile, out + g0 - mis, out + g0 + total, mis, mis + total, false};       // [mis, mis + total): this round's text
            tile_flush(text, true, lane);
            wave_lds_sync();                                                     // (the next round writes the tile again)
            r += cnt;
        }
    }
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
