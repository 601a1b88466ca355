// mzML structure on the device -> the per-spectrum columns and the tables fal_decode_peaks takes (payload, arrays).  The per-tag
// and per-spectrum functions are mzmlscan.h's (shared with the CPU tests); the grammar is DESIGN.md's "mzML on the device";
// falcon_amd/ms_io/mzml_io.read_chunks is the reader all of this mirrors.
//
// fal_mzml_index (one synchronisation, at its end):
//   count    : textscan.h's count walk over '<'; a device scan of the tile counts;
//   tags     : textscan.h's table walk (Shift 0): pos[k] = the '<' of tag k (i32), pos[tags] = n;
//   classify : a block takes 256 consecutive tags, stages their bytes -- one contiguous range -- into LDS with 16-byte loads per
//              lane and classifies a tag per thread from there: name, form, the quote-aware walk to '>', the attributes (a
//              range that does not fit the tile, because binary text lies in it, is read from global memory).  Every tag
//              becomes one MzTag record.  Per block: the <spectrum ...> opens and </spectrum> closes in it;
//   spectra  : a scan of the block counts numbers the opens and the closes; open s and close s are spectrum s, and every
//              marker checks that they alternate (an open has as many closes as opens in front of it, a close one open more).
// The tag table is sized before the tag count is known: n / 4 + 2 tags (a text with more is the host reader's,
// FAL_MZML_FLAG_TAGS); "<spectrum></spectrum>" takes 21 bytes, so n / 21 + 2 spectrum rows always suffice.
//
// fal_mzml_parse: the tables stay in the context's SLOT_MZML* slots between the two calls (checked against the text pointer, its
// length and the slot blocks).  One thread per spectrum walks its tag records (mzml_walk) and writes the columns, the array
// rows and the two text ranges; a scan of the 8-byte rounded lengths gives every spectrum's place in the payload; one wave per
// spectrum copies the two ranges there, a word per lane, and turns the spectrum to HOST when a byte of them is no base64
// candidate.  Every write is bounded by what the index counted.
#include <algorithm>
#include "common.h"
#include "ivf.h"
#include "mzmlscan.h"
#include "textscan.h"
#include "util.h"

static_assert(fal::MZ_PEAK_F64 == FAL_PEAK_F64 && fal::MZ_PEAK_ZLIB == FAL_PEAK_ZLIB && fal::MZ_PEAK_NP_LINEAR == FAL_PEAK_NUMPRESS_LINEAR &&
                  fal::MZ_PEAK_NP_PIC == FAL_PEAK_NUMPRESS_PIC && fal::MZ_PEAK_NP_SLOF == FAL_PEAK_NUMPRESS_SLOF,
              "mzmlscan.h: array flags differ from falcon_hip.h");
static_assert(fal::MZ_ST_OK == FAL_MZML_ST_OK && fal::MZ_ST_SKIP == FAL_MZML_ST_SKIP && fal::MZ_ST_HOST == FAL_MZML_ST_HOST,
              "mzmlscan.h: spectrum status differs from falcon_hip.h");

namespace fal {
namespace {

constexpr int kBlockTags = 256;                  // classify / spectra passes: a tag per thread
constexpr int kStageBytes = 32768;               // classify: LDS tile of a block's 256 tags
enum { META_TAGS = META_COUNT, META_SPECTRA = 2, META_INSIDE = 3 };

// ---- '<' per 4 KB block ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mzml_count_kernel(const uint8_t* __restrict__ text, int64_t n, int32_t* __restrict__ tile_cnt) {
    mark_count_pass<'<'>(text, n, tile_cnt);
}

// ---- the tag table -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mzml_tags_kernel(const uint8_t* __restrict__ text, int64_t n, const int64_t* __restrict__ tile_base,
                                                        int64_t n_tiles, int32_t* __restrict__ tag_pos, int64_t cap_tags,
                                                        unsigned long long* __restrict__ meta) {
    mark_table_pass<'<', 0, FAL_MZML_FLAG_TAGS>(text, n, tile_base, n_tiles, tag_pos, cap_tags, meta);
}

__device__ __forceinline__ int64_t indexed_tags(const unsigned long long* meta) {      // 0 when the table overflowed
    return (meta[META_FLAGS] & FAL_MZML_FLAG_TAGS) ? 0 : (int64_t)meta[META_TAGS];
}

__device__ __forceinline__ bool is_marker(int info, int form) {
    return (info & MZ_KIND) == MZ_SPECTRUM && ((info >> MZ_FORM_SHIFT) & MZ_FORM) == form;
}

// ---- tag records + spectrum markers per block -----------------------------------------------------------------------------------
// block_cnt[blk] = opens | closes << 32 (zeroed before: the grid strides over the blocks the tag count gives)
__global__ __launch_bounds__(256) void mzml_classify_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ tag_pos,
                                                            unsigned long long* __restrict__ meta, MzTag* __restrict__ recs,
                                                            int64_t* __restrict__ block_cnt) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kStageBytes + 16];
    const int64_t tags = indexed_tags(meta);
    const int64_t n_blocks = (tags + kBlockTags - 1) / kBlockTags;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t t0 = blk * kBlockTags, t1 = std::min<int64_t>(t0 + kBlockTags, tags);
        const int64_t b0 = tag_pos[t0], b1 = std::min<int64_t>(tag_pos[t1], n), a0 = b0 & ~(int64_t)15;
        const bool staged = b1 - a0 <= kStageBytes;                            // block-uniform
        __syncthreads();                                                        // the previous round's readers are done
        if (staged) stage_bytes(text, n, b0, b1, tile, threadIdx.x, 256);
        __syncthreads();
        const int64_t k = t0 + threadIdx.x;
        int info = 0;
        if (k < t1) {
            const int64_t s = tag_pos[k];
            const int limit = (int)(std::min<int64_t>(tag_pos[k + 1], n) - s);
            MzTag t;
            mzml_classify_tag(staged ? tile + (s - a0) : text + s, limit, (int32_t)s, &t);
            recs[k] = t;
            info = t.info;
        }
        if (__ballot(info & MZ_MARKUP) != 0 && (threadIdx.x & 63) == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)FAL_MZML_FLAG_MARKUP);
        int opens, closes;
        block_prefix(k < t1 && is_marker(info, MZ_OPEN), &opens);
        block_prefix(k < t1 && is_marker(info, MZ_CLOSE), &closes);
        if (threadIdx.x == 0) block_cnt[blk] = (int64_t)opens | ((int64_t)closes << 32);
    }
}

// ---- the spectrum table ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mzml_spectra_kernel(const MzTag* __restrict__ recs, unsigned long long* __restrict__ meta,
                                                           const int64_t* __restrict__ block_base, int64_t cap_blocks, int64_t cap_spectra,
                                                           int32_t* __restrict__ spec_open, int32_t* __restrict__ spec_close) {
    const int64_t tags = indexed_tags(meta);
    const int64_t n_blocks = (tags + kBlockTags - 1) / kBlockTags;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t k = blk * kBlockTags + threadIdx.x;
        const int info = k < tags ? recs[k].info : 0;
        const bool open = k < tags && is_marker(info, MZ_OPEN), close = k < tags && is_marker(info, MZ_CLOSE);
        int total;
        const int64_t base = block_base[blk];
        const int64_t ob = (base & 0xFFFFFFFF) + block_prefix(open, &total);
        const int64_t cb = (base >> 32) + block_prefix(close, &total);
        bool bad = false;
        long long inside = 0;
        if (open) {
            bad = ob != cb;
            if (ob < cap_spectra) spec_open[ob] = (int32_t)k;
            inside = -(long long)k - 1;
        }
        if (close) {
            bad = ob != cb + 1;
            if (cb < cap_spectra) spec_close[cb] = (int32_t)k;
            inside = (long long)k;
        }
        // (common.h's wave_xor_reduce, left written out: the call reorders the kernel's prologue -- profiles/NOTES.md)
        for (int d = 32; d > 0; d >>= 1) inside += __shfl_xor(inside, d, 64);
        const bool any_bad = __ballot(bad) != 0;
        if ((threadIdx.x & 63) == 0) {
            if (inside != 0) atomicAdd(&meta[META_INSIDE], (unsigned long long)inside);
            if (any_bad) atomicOr(&meta[META_FLAGS], (unsigned long long)FAL_MZML_FLAG_STRUCT);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t total = block_base[cap_blocks];
        const int64_t opens = total & 0xFFFFFFFF, closes = total >> 32;
        meta[META_SPECTRA] = (unsigned long long)opens;
        if (opens != closes) atomicOr(&meta[META_FLAGS], (unsigned long long)FAL_MZML_FLAG_STRUCT);
    }
}

// ---- parse: one walker per spectrum ---------------------------------------------------------------------------------------------
struct MzmlOut {
    int32_t* status;
    int64_t* id;
    int64_t* span;
    double* pmz;
    int32_t* charge;
    double* rt;
    int64_t* arrays;
};

// src[4 s ..]: the two text ranges {m/z from, m/z to, intensity from, intensity to}; rlen[s]: their 8-byte rounded lengths together, in units of 8 bytes
__global__ __launch_bounds__(256) void mzml_walk_kernel(const uint8_t* __restrict__ text, const MzTag* __restrict__ recs,
                                                        const int32_t* __restrict__ tag_pos, const int32_t* __restrict__ spec_open,
                                                        const int32_t* __restrict__ spec_close, int64_t n_spec, int32_t* __restrict__ src,
                                                        int32_t* __restrict__ rlen, MzmlOut out) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= n_spec) return;
    const int64_t k0 = spec_open[s], k1 = spec_close[s];
    MzSpectrum r;
    mzml_walk(text, recs, tag_pos, k0, k1, &r);
    out.status[s] = r.status;
    out.id[2 * s] = r.id_lo;
    out.id[2 * s + 1] = r.id_hi;
    out.span[2 * s] = tag_pos[k0];
    out.span[2 * s + 1] = (int64_t)recs[k1].end + 1;
    out.pmz[s] = r.pmz;
    out.charge[s] = r.charge;
    out.rt[s] = r.rt;
    int32_t rounded = 0;
    for (int a = 0; a < 2; ++a) {
        const int32_t len = r.text_hi[a] - r.text_lo[a];
        int64_t* row = out.arrays + 4 * (2 * s + a);
        row[0] = 0;                                                             // (the gather pass sets the offset)
        row[1] = len;
        row[2] = r.count[a];
        row[3] = r.flags[a];
        src[4 * s + 2 * a] = r.text_lo[a];
        src[4 * s + 2 * a + 1] = r.text_hi[a];
        rounded += (len + 7) >> 3;
    }
    rlen[s] = rounded;
}

// the text word (4 bytes, little endian) at byte position a, which need not be aligned; bytes at or behind n read as 0
__device__ __forceinline__ uint32_t load_word(const uint8_t* __restrict__ text, int64_t n, int64_t a) {
    const int64_t w = a & ~(int64_t)3;
    const int sh = (int)(a & 3) * 8;
    uint32_t lo, hi = 0;
    if (w + 8 <= n) {
        lo = *reinterpret_cast<const uint32_t*>(text + w);
        hi = *reinterpret_cast<const uint32_t*>(text + w + 4);
    } else {
        lo = 0;
        for (int j = 0; j < 8; ++j)
            if (w + j < n) (j < 4 ? lo : hi) |= (uint32_t)text[w + j] << (8 * (j & 3));
    }
    return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
}

// ---- gather: one wave per spectrum copies its two text ranges into the payload --------------------------------------------------
__global__ __launch_bounds__(256) void mzml_gather_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ src,
                                                          const int64_t* __restrict__ offs, int64_t n_spec, uint8_t* __restrict__ payload,
                                                          int64_t payload_cap, MzmlOut out) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_spec; s += waves) {
        if (out.status[s] != MZ_ST_OK) continue;                               // wave-uniform
        int64_t at = offs[s] * 8;
        if (offs[s + 1] * 8 > payload_cap) {                                        // (the entry point refuses such a capacity)
            if (lane == 0) out.status[s] = MZ_ST_HOST;
            continue;
        }
        bool bad = false;
        for (int a = 0; a < 2; ++a) {
            const int64_t lo = src[4 * s + 2 * a], len = src[4 * s + 2 * a + 1] - lo;
            const int64_t words = ((len + 7) & ~(int64_t)7) >> 2;
            uint32_t* dst = reinterpret_cast<uint32_t*>(payload + at);
            for (int64_t j = lane; j < words; j += 64) {
                uint32_t w = 4 * j < len ? load_word(text, n, lo + 4 * j) : 0;
                const int64_t left = len - 4 * j;                               // bytes of this word inside the range
                if (left < 4) w &= left <= 0 ? 0u : (1u << (8 * left)) - 1;
#pragma unroll
                for (int b = 0; b < 4; ++b) bad |= b < left && !mzml_binary_byte((w >> (8 * b)) & 0xFF);
                dst[j] = w;
            }
            if (lane == 0) out.arrays[4 * (2 * s + a)] = at;
            at += words * 4;
        }
        if (__ballot(bad) != 0) {                                                 // HOST after all: its columns and rows are zeros
            if (lane == 0) {
                out.status[s] = MZ_ST_HOST;
                out.charge[s] = 0;
                out.pmz[s] = out.rt[s] = 0.0;
                out.id[2 * s] = out.id[2 * s + 1] = 0;
            }
            if (lane < 8) out.arrays[8 * s + lane] = 0;
        }
    }
}

FAL_WARM_KERNEL(mzml_classify_kernel);

}  // namespace
}  // namespace fal

using namespace fal;

extern "C" int fal_mzml_index(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t* counts_out) {
    fal::CallScope _call(ctx);
    FAL_TRY(text_index_begin("fal_mzml_index", ctx, &fal_ctx::mzml, text, n_bytes, counts_out));
    if (n_bytes == 0) return FAL_OK;
    const int64_t n_tiles = ceil_div(n_bytes, kTileBytes);
    const int64_t cap_tags = n_bytes / 4 + 2, cap_spectra = n_bytes / 21 + 2, cap_blocks = ceil_div(cap_tags, kBlockTags);
    int32_t* tag_pos = nullptr;
    MzTag* recs = nullptr;
    FAL_TRY(ctx->reserve(SLOT_MZML, sizeof(int32_t) * (size_t)(cap_tags + 1), (void**)&tag_pos));
    FAL_TRY(ctx->reserve(SLOT_MZML2, sizeof(MzTag) * (size_t)cap_tags, (void**)&recs));
    ScratchLayout L3, L4;
    const auto meta = L3.array<unsigned long long>(8);                              // 64 B of meta words
    const auto block_cnt = L3.array<int64_t>(cap_blocks), block_base = L3.array<int64_t>(cap_blocks + 1);   // marker counts per tag block, their scan
    const auto tile_base = L3.array<int64_t>(n_tiles + 1);                          // the scan of the '<' counts per tile
    const auto tile_cnt = L3.array<int32_t>(n_tiles + 2);
    L3.pad(72);
    FAL_TRY(L3.reserve(ctx, SLOT_MZML3));
    const auto spec_open = L4.array<int32_t>(cap_spectra), spec_close = L4.array<int32_t>(cap_spectra);
    FAL_TRY(L4.reserve(ctx, SLOT_MZML4));
    FAL_CHECK_HIP(hipMemsetAsync(meta, 0, 64 + sizeof(int64_t) * (size_t)cap_blocks, ctx->stream));       // meta and block_cnt behind it
    hipLaunchKernelGGL(mzml_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, text, n_bytes, tile_cnt);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, tile_cnt, n_tiles, tile_base, SLOT_SORT));
    hipLaunchKernelGGL(mzml_tags_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, text, n_bytes, tile_base, n_tiles, tag_pos,
                       cap_tags, meta);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned grid = capped_grid(ctx, cap_tags, kBlockTags);
    hipLaunchKernelGGL(mzml_classify_kernel, dim3(grid), dim3(256), 0, ctx->stream, text, n_bytes, tag_pos, meta, recs, block_cnt);
    FAL_CHECK_HIP(hipGetLastError());
    ctx->release(SLOT_SORT);                                                    // (the first scan's block is no longer held here)
    FAL_TRY(device_scan_i64(ctx, block_cnt, cap_blocks, block_base, SLOT_SORT));
    hipLaunchKernelGGL(mzml_spectra_kernel, dim3(grid), dim3(256), 0, ctx->stream, recs, meta, block_base, cap_blocks, cap_spectra,
                       spec_open, spec_close);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned long long* h = nullptr;
    FAL_TRY(read_meta(ctx, meta, &h));
    const int64_t flags = (int64_t)h[META_FLAGS];
    FAL_REQUIRE(flags != 0 || (int64_t)h[META_SPECTRA] <= cap_spectra, FAL_EINTERNAL, "fal_mzml_index: more spectra than 21-byte slots");
    counts_out[0] = flags ? 0 : (int64_t)h[META_SPECTRA];
    counts_out[1] = flags ? 0 : (int64_t)h[META_INSIDE];
    counts_out[2] = flags;
    counts_out[3] = (int64_t)h[META_TAGS];
    store_index(ctx->mzml, text, n_bytes, counts_out[0], 0, cap_tags, cap_spectra, tag_pos, recs, meta, spec_open);
    return FAL_OK;
}

extern "C" int fal_mzml_parse(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, uint8_t* payload, int64_t payload_cap,
                              int32_t* status_out, int64_t* id, int64_t* span, double* precursor_mz, int32_t* charge,
                              double* retention_time, int64_t* arrays) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_spectra >= 0 && payload_cap >= 0, FAL_EINVAL, "fal_mzml_parse: bad argument");
    const fal_ctx::TextIndex& ix = ctx->mzml;
    FAL_REQUIRE(matches(ctx, ix, SLOT_MZML, text, n_bytes, n_spectra), FAL_EINVAL,
                "fal_mzml_parse: not the text, length and spectrum count of the last fal_mzml_index of this context");
    if (n_spectra == 0) return FAL_OK;
    FAL_REQUIRE(payload && payload_cap >= n_bytes + 16 * n_spectra && ((uintptr_t)payload & 7) == 0, FAL_EINVAL,
                "fal_mzml_parse: payload NULL, not 8-byte aligned or smaller than n_bytes + 16 n_spectra");
    FAL_REQUIRE(status_out && id && span && precursor_mz && charge && retention_time && arrays, FAL_EINVAL, "fal_mzml_parse: NULL column");
    const int32_t* tag_pos = static_cast<const int32_t*>(ix.blocks[0]);
    const MzTag* recs = static_cast<const MzTag*>(ix.blocks[1]);
    const int32_t* spec = static_cast<const int32_t*>(ix.blocks[3]);
    const int32_t *spec_open = spec, *spec_close = spec + ix.cap_spectra;
    ScratchLayout L;
    const auto src = L.array<int32_t>(4 * n_spectra);      // text ranges, four words a spectrum
    const auto rlen = L.array<int32_t>(n_spectra);         // rounded lengths
    const auto offs = L.array<int64_t>(n_spectra + 1);     // and their scan
    L.pad(64);
    FAL_TRY(L.reserve(ctx, SLOT_MZML5));
    const MzmlOut out{status_out, id, span, precursor_mz, charge, retention_time, arrays};
    hipLaunchKernelGGL(mzml_walk_kernel, dim3((unsigned)ceil_div(n_spectra, 64)), dim3(64), 0, ctx->stream, text, recs, tag_pos, spec_open,
                       spec_close, n_spectra, src, rlen, out);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, rlen, n_spectra, offs, SLOT_SORT));
    const unsigned grid = capped_grid(ctx, n_spectra, 4);
    hipLaunchKernelGGL(mzml_gather_kernel, dim3(grid), dim3(256), 0, ctx->stream, text, n_bytes, src, offs, n_spectra, payload, payload_cap,
                       out);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
