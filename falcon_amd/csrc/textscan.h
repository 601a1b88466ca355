// What the text readers on the device (mgfparse.hip, mzmlscan.hip) share.  Device side: 16-byte loads that stop at the end of
// the text, a block-wide prefix sum, the copy of a byte range into an LDS tile, and the two passes that build a text's mark
// table (the positions of one byte value: the line starts of MGF, the '<' of mzML).  Host side (at the bottom): the index
// handle fal_ctx::TextIndex that carries the tables from fal_*_index to fal_*_parse.  The meta words and their read-back are
// util.h's, shared with the text writers (textwrite.h).
#pragma once
#include <algorithm>
#include "common.h"
#include "util.h"

namespace fal {

// 16 text bytes at pos (a multiple of 16) as four words; bytes at or behind n read as 0
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ text, int64_t n, int64_t pos) {
    if (pos + 16 <= n) return *reinterpret_cast<const uint4*>(text + pos);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (pos + j < n) w[j >> 2] |= (uint32_t)text[pos + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t byte_of(const uint4& v, int j) {
    const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 0xFF;
}

// exclusive prefix of v over the 256 threads of a block, *total: the block's sum
__device__ __forceinline__ int block_prefix(int v, int* total) {
    __shared__ int ws[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_prefix_sum(v);
    __syncthreads();                             // (the previous use of ws is over)
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
    for (int w = 0; w < 4; ++w) {
        before += w < wave ? ws[w] : 0;
        sum += ws[w];
    }
    *total = sum;
    return before + incl - v;
}

// bytes [b0, b1) of the text into an LDS tile whose byte 0 is text byte (b0 & ~15); `step` lanes x 16 bytes per round
__device__ __forceinline__ void stage_bytes(const uint8_t* __restrict__ text, int64_t n, int64_t b0, int64_t b1, uint8_t* tile, int lane,
                                            int step) {
    const int64_t a0 = b0 & ~(int64_t)15;
    for (int64_t off = lane * 16; a0 + off < b1; off += step * 16) *reinterpret_cast<uint4*>(tile + off) = load16(text, n, a0 + off);
}

// ---- the mark table ----------------------------------------------------------------------------------------------------------------
// Two walks over the text, 16 bytes per lane and kTileBytes per block of 256, with a device scan of the tile counts between
// them (tile_base[0 .. n_tiles], the last entry the total).  Of the meta words (util.h) both passes need two: meta[META_COUNT] =
// the table's entries, whatever its capacity, and meta[META_FLAGS], where Flag is set when they exceed it.
constexpr int kTileBytes = 4096;

// how many of the lane's 16 bytes v = load16(text, n, pos) are Mark
template <char Mark>
__device__ __forceinline__ int count_marks(const uint4 v, int64_t n, int64_t pos) {
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) cnt += pos + j < n && byte_of(v, j) == Mark;
    return cnt;
}

// first walk: tile_cnt[tile] = its marks
template <char Mark>
__device__ __forceinline__ void mark_count_pass(const uint8_t* __restrict__ text, int64_t n, int32_t* __restrict__ tile_cnt) {
    const int64_t pos = blockIdx.x * (int64_t)kTileBytes + threadIdx.x * 16;
    const uint4 v = load16(text, n, pos);
    int total;
    block_prefix(count_marks<Mark>(v, n, pos), &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// the first walk of the line readers (MGF, MSP): the '\n' of every tile, and the byte check of their device grammar -- Flag is
// set for a byte outside \t, \n, 0x20-0x7E and a \r that is directly followed by \n
template <unsigned Flag>
__device__ __forceinline__ void newline_count_pass(const uint8_t* __restrict__ text, int64_t n, int32_t* __restrict__ tile_cnt,
                                                   unsigned long long* __restrict__ meta) {
    const int64_t pos = blockIdx.x * (int64_t)kTileBytes + threadIdx.x * 16;
    const uint4 v = load16(text, n, pos);
    // the byte behind this lane's 16: the next lane's first (the last lane of a wave reads it)
    uint32_t next = __shfl_down(v.x & 0xFF, 1, 64);
    if ((threadIdx.x & 63) == 63) next = pos + 16 < n ? text[pos + 16] : 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t c = byte_of(v, j), c1 = j < 15 ? byte_of(v, j + 1) : next;
        bad |= pos + j < n && !(c == '\t' || c == '\n' || (c >= 0x20 && c <= 0x7E) || (c == '\r' && pos + j + 1 < n && c1 == '\n'));
    }
    int total;
    block_prefix(count_marks<'\n'>(v, n, pos), &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)Flag);
}

// second walk: the table (i32, cap + 1 entries), closed by a sentinel behind its last entry.
//   Shift 0: entry k = the position of mark k; `marks` entries; sentinel n          (a tag begins at its '<')
//   Shift 1: entry 0 = 0, entry k + 1 = the byte behind mark k; `marks + 1` entries; sentinel n + 1   (a line begins behind a '\n')
// More entries than cap: the table's first cap are written, the sentinel is not, and Flag is set.
template <char Mark, int Shift, unsigned Flag>
__device__ __forceinline__ void mark_table_pass(const uint8_t* __restrict__ text, int64_t n, const int64_t* __restrict__ tile_base,
                                                int64_t n_tiles, int32_t* __restrict__ table, int64_t cap,
                                                unsigned long long* __restrict__ meta) {
    const int64_t pos = blockIdx.x * (int64_t)kTileBytes + threadIdx.x * 16;
    const uint4 v = load16(text, n, pos);
    int total;
    int64_t k = tile_base[blockIdx.x] + block_prefix(count_marks<Mark>(v, n, pos), &total) + Shift;      // the lane's first entry
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (pos + j < n && byte_of(v, j) == Mark) {
            if (k < cap + Shift) table[k] = (int32_t)(pos + j + Shift);
            ++k;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t entries = tile_base[n_tiles] + Shift;
        if (Shift) table[0] = 0;
        meta[META_COUNT] = (unsigned long long)entries;
        if (entries <= cap) table[entries] = (int32_t)(n + Shift);
        else atomicOr(&meta[META_FLAGS], (unsigned long long)Flag);
    }
}

// ---- host side: the index handle -----------------------------------------------------------------------------------------------------
// `who` is the entry point's name in the messages.

// the opening of fal_*_index: argument checks, the handle and the counts reset; a zero-byte text is indexed by that alone
inline int text_index_begin(const char* who, fal_ctx* ctx, fal_ctx::TextIndex fal_ctx::*which, const uint8_t* text, int64_t n_bytes,
                            int64_t* counts_out) {
    FAL_REQUIRE(ctx && counts_out && n_bytes >= 0 && n_bytes < 0x7FFFFFFF, FAL_EINVAL, "%s: bad argument", who);
    FAL_REQUIRE(n_bytes == 0 || (text && ((uintptr_t)text & 15) == 0), FAL_EINVAL, "%s: text NULL or not 16-byte aligned", who);
    fal_ctx::TextIndex& ix = ctx->*which;
    ix = fal_ctx::TextIndex{};
    for (int i = 0; i < 4; ++i) counts_out[i] = 0;
    if (n_bytes == 0) {
        ix.text = text;
        ix.bytes = 0;
    }
    return FAL_OK;
}

inline void store_index(fal_ctx::TextIndex& ix, const void* text, int64_t n_bytes, int64_t spectra, int64_t extra, int64_t cap_table,
                        int64_t cap_spectra, const void* b0, const void* b1, const void* b2, const void* b3) {
    ix = fal_ctx::TextIndex{text, n_bytes, spectra, extra, cap_table, cap_spectra, {b0, b1, b2, b3}};
}

// is `ix` the index of this text, length and spectrum count, its tables still in the slots first_slot .. first_slot + 3?
inline bool matches(const fal_ctx* ctx, const fal_ctx::TextIndex& ix, int first_slot, const void* text, int64_t n_bytes, int64_t n_spectra) {
    bool mine = ix.bytes == n_bytes && ix.text == text && ix.spectra == n_spectra;
    if (mine && n_bytes > 0) {
        mine = ix.blocks[0] != nullptr;
        for (int i = 0; i < 4; ++i) mine = mine && ix.blocks[i] == ctx->scratch[first_slot + i].ptr;
    }
    return mine;
}

}  // namespace fal
