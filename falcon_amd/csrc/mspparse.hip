// MSP library text on the device -> the raw peak CSR fal_process_spectra takes (indptr i64, m/z f64, intensity f32, peaks sorted
// by m/z inside every entry) plus the per-entry columns.  The per-line functions are mspparse.h's (shared with the CPU tests); the
// grammar is DESIGN.md's "MSP on the device"; falcon_amd/ms_io/msp_io.py holds the reader all of this mirrors.
//
// fal_msp_index (one synchronisation, at its end):
//   newlines : textscan.h's newline walk with the byte check of the device grammar; a device scan of the tile counts;
//   lines    : textscan.h's table walk (Shift 1): start[k] = first byte of line k (i32), start[lines] = n + 1;
//   classify : mgf_classify_kernel's shape -- a block takes 256 consecutive lines, stages their bytes into LDS and handles a line
//              per thread (a range that does not fit the tile is read from global memory): the line's kind, its peak segments,
//              and per block the number of its Name: lines;
//   blocks   : one wave scans the blocks' Name: counts -- there is one marker kind, so the carry is a plain scan;
//   entries  : Name: line k begins entry k; entry_begin[entries] = lines closes the table;
//   counts   : one wave per entry: its first Num Peaks line (-1: none) and the sum of the segment counts of the lines behind it;
//              the total is the capacity the caller allocates.
// The line table is sized as MGF's (n / 4 + 2 lines, FAL_MGF_FLAG_LINES beyond); an entry takes at least its "name:" and a
// newline, so n / 6 + 2 entry rows always suffice.
//
// fal_msp_parse: the tables stay in the context's SLOT_MSP* slots between the two calls, checked as fal_mgf_parse checks its
// own.  A scan of the counts gives indptr; then one wave per entry, 64 lines at a time staged into the wave's LDS tile, a line
// per lane: first the header lines up to the Num Peaks line (precursor aliases, charge, the Num Peaks value; the last line of a
// key wins), then the peak text: a lane walks its line's segments and writes them at the entry's slot plus the exclusive prefix
// of the segment counts (a scratch copy); peaksort.h's sort moves them to the output.  Every write is bounded by the slot the
// index counted.
// fal_msp_headers: textkeys.h's pass (shared with fal_mgf_headers) over this index: separator ':', the lines from the Name: line
// to the first Num Peaks line.
#include <algorithm>
#include "common.h"
#include "ivf.h"
#include "mspparse.h"
#include "peaksort.h"
#include "textkeys.h"
#include "textscan.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kBlockLines = 256;                 // classify / entries passes: a line per thread
constexpr int kStageBytes = 16384;               // classify: LDS tile of a block's 256 lines
constexpr int kWaveStage = 4096;                 // parse: LDS tile of a wave's 64 lines
enum { META_LINES = META_COUNT, META_ENTRIES = 2, META_PEAKS = 3 };
enum { KEY_NONE = 0, KEY_PMZ0 = 1, KEY_PMZ1 = 2, KEY_PMZ2 = 3, KEY_CHARGE = 4, KEY_COUNT = 5 };

__global__ __launch_bounds__(256) void msp_newlines_kernel(const uint8_t* __restrict__ text, int64_t n, int32_t* __restrict__ block_nl,
                                                           unsigned long long* __restrict__ meta) {
    newline_count_pass<FAL_MGF_FLAG_BYTES>(text, n, block_nl, meta);
}

__global__ __launch_bounds__(256) void msp_lines_kernel(const uint8_t* __restrict__ text, int64_t n, const int64_t* __restrict__ block_base,
                                                        int64_t n_blocks, int32_t* __restrict__ start, int64_t cap_lines,
                                                        unsigned long long* __restrict__ meta) {
    mark_table_pass<'\n', 1, FAL_MGF_FLAG_LINES>(text, n, block_base, n_blocks, start, cap_lines, meta);
}

__device__ __forceinline__ int64_t indexed_lines(const unsigned long long* meta) {      // 0 when the table overflowed
    return (meta[META_FLAGS] & FAL_MGF_FLAG_LINES) ? 0 : (int64_t)meta[META_LINES];
}

__device__ __forceinline__ int64_t line_blocks(int64_t lines) { return (lines + kBlockLines - 1) / kBlockLines; }

// ---- line kinds, segment counts, Name: lines per block ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void msp_classify_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ start,
                                                           const unsigned long long* __restrict__ meta, uint8_t* __restrict__ cls,
                                                           int32_t* __restrict__ seg, int32_t* __restrict__ block_names) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kStageBytes + 16];
    const int64_t lines = indexed_lines(meta);
    const int64_t n_blocks = line_blocks(lines);
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t l0 = blk * kBlockLines, l1 = std::min<int64_t>(l0 + kBlockLines, lines);
        const int64_t b0 = start[l0], b1 = std::min<int64_t>(start[l1], n);
        const bool staged = b1 - (b0 & ~(int64_t)15) <= kStageBytes;          // block-uniform
        __syncthreads();                                                        // the previous round's readers are done
        if (staged) stage_bytes(text, n, b0, b1, tile, threadIdx.x, 256);
        __syncthreads();
        const int64_t line = l0 + threadIdx.x;
        int kind = MSP_BLANK;
        if (line < l1) {
            const int64_t s = start[line];
            const int len = (int)(start[line + 1] - 1 - s);
            const uint8_t* p = staged ? tile + (s - (b0 & ~(int64_t)15)) : text + s;
            int lo, hi;
            kind = msp_classify(p, len, &lo, &hi);
            cls[line] = (uint8_t)kind;
            seg[line] = msp_segments(p, len);
        }
        int total;
        block_prefix((kind & MSP_KIND) == MSP_NAME ? 1 : 0, &total);
        if (threadIdx.x == 0) block_names[blk] = total;
    }
}

// ---- scan over the blocks: one wave ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void msp_blocks_kernel(const int32_t* __restrict__ block_names, int32_t* __restrict__ block_first,
                                                        unsigned long long* __restrict__ meta) {
    const int lane = threadIdx.x;
    const int64_t n_blocks = line_blocks(indexed_lines(meta));
    int base = 0;                                                               // wave-uniform
    for (int64_t g = 0; g < n_blocks; g += 64) {
        const bool valid = g + lane < n_blocks;
        const int cnt = valid ? block_names[g + lane] : 0;
        const int incl = wave_prefix_sum(cnt);
        if (valid) block_first[g + lane] = base + incl - cnt;
        base += __shfl(incl, 63, 64);
    }
    if (lane == 0) meta[META_ENTRIES] = (unsigned long long)base;
}

// ---- the entry table: entry_begin[k] = the line of Name: line k, entry_begin[entries] = lines ------------------------------------
__global__ __launch_bounds__(256) void msp_entries_kernel(const uint8_t* __restrict__ cls, const unsigned long long* __restrict__ meta,
                                                          const int32_t* __restrict__ block_first, int64_t cap_entries,
                                                          int32_t* __restrict__ entry_begin) {
    const int64_t lines = indexed_lines(meta);
    const int64_t n_blocks = line_blocks(lines);
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t line = blk * kBlockLines + threadIdx.x;
        const bool name = line < lines && (cls[line] & MSP_KIND) == MSP_NAME;
        int total;
        const int64_t at = (int64_t)block_first[blk] + block_prefix(name ? 1 : 0, &total);
        if (name && at < cap_entries) entry_begin[at] = (int32_t)line;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t entries = (int64_t)meta[META_ENTRIES];
        if (entries <= cap_entries) entry_begin[entries] = (int32_t)lines;       // (the table has cap_entries + 1 rows)
    }
}

// ---- per entry: the first Num Peaks line and the peaks behind it ------------------------------------------------------------------
__global__ __launch_bounds__(256) void msp_counts_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ seg,
                                                         unsigned long long* __restrict__ meta, int64_t cap_entries,
                                                         const int32_t* __restrict__ entry_begin, int32_t* __restrict__ entry_np,
                                                         int32_t* __restrict__ entry_count) {
    const int lane = threadIdx.x & 63;
    const int64_t n_ent = (int64_t)meta[META_ENTRIES] <= cap_entries ? (int64_t)meta[META_ENTRIES] : 0;      // (beyond: no closed table)
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_ent; s += waves) {
        const int64_t b = entry_begin[s], e = entry_begin[s + 1];
        int64_t np = -1;
        for (int64_t g = b + 1; g < e && np < 0; g += 64) {
            const uint64_t m = __ballot(g + lane < e && (cls[g + lane] & MSP_KIND) == MSP_NUMPEAKS);
            if (m) np = g + __builtin_ctzll(m);
        }
        int cnt = 0;
        if (np >= 0)
            for (int64_t l = np + 1 + lane; l < e; l += 64) cnt += seg[l];
        cnt = __shfl(wave_prefix_sum(cnt), 63, 64);
        if (lane == 0) {
            entry_np[s] = (int32_t)np;
            entry_count[s] = cnt;
            atomicAdd(&meta[META_PEAKS], (unsigned long long)cnt);
        }
    }
}

// ---- parse: one wave per entry -------------------------------------------------------------------------------------------------
struct MspOut {
    double* pmz;
    int32_t* charge;
    int32_t* has_charge;
    int64_t* span;
    int32_t* status;
};

// a header line's stripped key -> KEY_*
__device__ __forceinline__ int msp_own_key(const uint8_t* k, int n) {
    if (mgf_equals(k, n, "precursormz", 11, true)) return KEY_PMZ0;
    if (mgf_equals(k, n, "precursor_mz", 12, true)) return KEY_PMZ1;
    if (mgf_equals(k, n, "pepmass", 7, true)) return KEY_PMZ2;
    if (mgf_equals(k, n, "charge", 6, true)) return KEY_CHARGE;
    if (mgf_equals(k, n, "num peaks", 9, true)) return KEY_COUNT;
    return KEY_NONE;
}

__global__ __launch_bounds__(256) void msp_parse_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ start,
                                                        const uint8_t* __restrict__ cls, const int32_t* __restrict__ seg,
                                                        const int32_t* __restrict__ entry_begin, const int32_t* __restrict__ entry_np,
                                                        int64_t n_ent, const int64_t* __restrict__ indptr, int64_t nnz_cap,
                                                        double* __restrict__ tmp_mz, float* __restrict__ tmp_it, MspOut out) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4][kWaveStage + 16];
    const int lane = threadIdx.x & 63;
    uint8_t* tile = tiles[threadIdx.x >> 6];
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_ent; s += waves) {
        const int64_t b = entry_begin[s], e = entry_begin[s + 1], np = entry_np[s];
        const int64_t slot = indptr[s], slot_end = std::min<int64_t>(indptr[s + 1], nnz_cap);
        // wave-uniform state: per key the last line's value
        bool host = np < 0;
        bool has_pm[3] = {false, false, false}, pm_ok[3] = {false, false, false}, has_ch = false, ch_ok = false, has_cnt = false, cnt_ok = false;
        double pm[3] = {0.0, 0.0, 0.0};
        int ch = 0, cnt = 0;
        // the header lines: from the Name: line to the Num Peaks line (without one the entry is the host's: nothing to read)
        for (int64_t g = b; g <= np; g += 64) {
            const int64_t g1 = std::min<int64_t>(g + 64, np + 1);
            const int64_t b0 = start[g], b1 = std::min<int64_t>(start[g1], n), a0 = b0 & ~(int64_t)15;
            const bool staged = b1 - a0 <= kWaveStage;                         // wave-uniform
            if (staged) stage_bytes(text, n, b0, b1, tile, lane, 64);
            wave_lds_sync();
            const int64_t line = g + lane;
            int key = KEY_NONE, ival = 0;
            bool ok = false;
            double val = 0.0;
            if (line < g1) {
                const int c = cls[line];
                const int kind = c & MSP_KIND;
                if (c & MSP_LONG) {
                    host = true;                                                // a line longer than kMgfMaxLine: the host reader's
                } else if (kind == MSP_HEADER || kind == MSP_NUMPEAKS) {
                    const int64_t ls = start[line];
                    const int len = (int)(start[line + 1] - 1 - ls);
                    const uint8_t* p = staged ? tile + (ls - a0) : text + ls;
                    int lo = 0, hi = len, klo, khi, a, z;
                    mgf_strip(p, &lo, &hi);
                    msp_split(p, lo, hi, &klo, &khi, &a, &z);
                    key = msp_own_key(p + klo, khi - klo);
                    if (key == KEY_CHARGE) {
                        ok = mgf_parse_charge(p + a, z - a, &ival);
                    } else if (key == KEY_COUNT) {
                        ok = msp_parse_count(p + a, z - a, &ival);
                    } else if (key != KEY_NONE) {                              // the first whitespace token; none: the host decides
                        int pos = a, t0, t1;
                        mgf_token(p, &pos, z, &t0, &t1);
                        ok = t1 > t0 && mgf_parse_double(p + t0, t1 - t0, &val);
                    }
                }
            }
            wave_lds_sync();                                                    // the tile's readers are done before it is staged again
            if (__ballot(key != KEY_NONE) == 0) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const uint64_t m = __ballot(key == KEY_PMZ0 + a);
                if (m) {
                    const int src = 63 - __builtin_clzll(m);
                    has_pm[a] = true;
                    pm_ok[a] = __shfl((int)ok, src, 64) != 0;
                    pm[a] = __shfl(val, src, 64);
                }
            }
            const uint64_t m_c = __ballot(key == KEY_CHARGE), m_n = __ballot(key == KEY_COUNT);
            if (m_c) {
                const int src = 63 - __builtin_clzll(m_c);
                has_ch = true;
                ch_ok = __shfl((int)ok, src, 64) != 0;
                ch = __shfl(ival, src, 64);
            }
            if (m_n) {                                                          // (np is the entry's first such line, and the range's last)
                const int src = 63 - __builtin_clzll(m_n);
                has_cnt = true;
                cnt_ok = __shfl((int)ok, src, 64) != 0;
                cnt = __shfl(ival, src, 64);
            }
        }
        // the peak text: every line behind the Num Peaks line
        int64_t n_peaks = 0;
        for (int64_t g = np < 0 ? e : np + 1; g < e; g += 64) {
            const int64_t g1 = std::min<int64_t>(g + 64, e);
            const int64_t b0 = start[g], b1 = std::min<int64_t>(start[g1], n), a0 = b0 & ~(int64_t)15;
            const bool staged = b1 - a0 <= kWaveStage;                         // wave-uniform
            if (staged) stage_bytes(text, n, b0, b1, tile, lane, 64);
            wave_lds_sync();
            const int64_t line = g + lane;
            const int mine = line < g1 ? seg[line] : 0;                         // the segments the index counted for this line
            const int incl = wave_prefix_sum(mine);
            if (line < g1 && (cls[line] & MSP_LONG)) {
                host = true;                                                    // the slot keeps its size; the host reader fills it
            } else if (mine > 0) {
                const int64_t ls = start[line];
                const int len = (int)(start[line + 1] - 1 - ls);
                {
                    const uint8_t* p = staged ? tile + (ls - a0) : text + ls;
                    const int end = msp_peak_end(p, 0, len);
                    int64_t at = slot + n_peaks + (incl - mine);
                    int pos = 0, a, z;
                    for (int j = 0; j < mine && msp_segment(p, &pos, end, &a, &z); ++j, ++at) {
                        int t0, t1, u0, u1;
                        double mz = 0.0, it = 0.0;
                        msp_peak_tokens(p, a, z, &t0, &t1, &u0, &u1);
                        bool ok = mgf_parse_double(p + t0, t1 - t0, &mz);
                        if (u1 > u0) ok = mgf_parse_double(p + u0, u1 - u0, &it) && ok;
                        if (!ok) {
                            host = true;
                            mz = it = 0.0;
                        }
                        if (at < slot_end) {
                            tmp_mz[at] = mz;
                            tmp_it[at] = (float)it;
                        }
                    }
                }
            }
            n_peaks += __shfl(incl, 63, 64);
            wave_lds_sync();                                                    // the tile's readers are done before it is staged again
        }
        // the host rule's order: precursormz, else precursor_mz, else pepmass
        const bool pm_good = has_pm[0] ? pm_ok[0] : has_pm[1] ? pm_ok[1] : has_pm[2] && pm_ok[2];
        const double pm_val = has_pm[0] ? pm[0] : has_pm[1] ? pm[1] : pm[2];
        host = __ballot(host) != 0 || !pm_good || (has_ch && !ch_ok) || !has_cnt || !cnt_ok || (int64_t)cnt != n_peaks ||
               n_peaks != indptr[s + 1] - slot;
        if (lane == 0) {
            out.pmz[s] = pm_good ? pm_val : 0.0;
            out.charge[s] = has_ch && ch_ok ? ch : 0;
            out.has_charge[s] = has_ch ? 1 : 0;
            out.span[2 * s] = start[b];
            out.span[2 * s + 1] = std::min<int64_t>(start[e], n);
            out.status[s] = host ? FAL_MSP_ST_HOST : 0;
        }
    }
}

// ---- sort: the scratch copy -> the output ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void msp_sort_kernel(const int64_t* __restrict__ indptr, int64_t n_ent, int64_t nnz_cap,
                                                       const double* __restrict__ tmp_mz, const float* __restrict__ tmp_it,
                                                       double* __restrict__ out_mz, float* __restrict__ out_it) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_ent; s += waves) {
        const int64_t b = indptr[s], e = indptr[s + 1];
        if (e > nnz_cap) continue;                                             // (the entry point refuses such a capacity)
        wave_sort_peaks(e - b, lane, [&](int64_t j) { return tmp_mz[b + j]; }, [&](int64_t j) { return tmp_it[b + j]; }, out_mz + b,
                        out_it + b);
    }
}

// ---- header values by a key table -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void msp_headers_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ start,
                                                          const uint8_t* __restrict__ cls, const int32_t* __restrict__ entry_begin,
                                                          const int32_t* __restrict__ entry_np, int64_t n_ent, MgfKeyTable table,
                                                          int64_t* __restrict__ span_out, int64_t* __restrict__ value_out,
                                                          int32_t* __restrict__ state_out) {
    headers_pass<':'>(
        text, n, start, cls, n_ent, table, span_out, value_out, state_out,
        [&](int64_t s, int64_t* first, int64_t* last) {
            const int64_t np = entry_np[s];
            *first = entry_begin[s];
            *last = np < 0 ? (int64_t)entry_begin[s + 1] : np + 1;
        },
        [](int c) {
            const int kind = c & MSP_KIND;
            return kind == MSP_NAME || kind == MSP_NUMPEAKS || kind == MSP_HEADER;
        });
}

FAL_WARM_KERNEL(msp_parse_kernel);

}  // namespace
}  // namespace fal

using namespace fal;

extern "C" int fal_msp_index(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t* counts_out) {
    fal::CallScope _call(ctx);
    FAL_TRY(text_index_begin("fal_msp_index", ctx, &fal_ctx::msp, text, n_bytes, counts_out));
    if (n_bytes == 0) {
        counts_out[3] = 1;                                                      // (lines = '\n' + 1, as for every other text)
        return FAL_OK;
    }
    const int64_t n_tiles = ceil_div(n_bytes, kTileBytes);
    const int64_t cap_lines = n_bytes / 4 + 2, cap_entries = n_bytes / 6 + 2, cap_blocks = ceil_div(cap_lines, kBlockLines);
    int32_t* start = nullptr;
    FAL_TRY(ctx->reserve(SLOT_MSP, sizeof(int32_t) * (size_t)(cap_lines + 1), (void**)&start));
    ScratchLayout L2, L3, L4;
    const auto seg = L2.array<int32_t>(cap_lines);
    const auto cls = L2.array<uint8_t>(cap_lines);
    FAL_TRY(L2.reserve(ctx, SLOT_MSP2));
    const auto meta = L3.array<unsigned long long>(8);                              // 64 B of meta words
    const auto block_base = L3.array<int64_t>(n_tiles + 1);                         // the scan of the newline counts
    const auto block_nl = L3.array<int32_t>(n_tiles + 2);
    const auto block_names = L3.array<int32_t>(cap_blocks), block_first = L3.array<int32_t>(cap_blocks);
    L3.pad(72);
    FAL_TRY(L3.reserve(ctx, SLOT_MSP3));
    const auto entry_begin = L4.array<int32_t>(cap_entries + 1), entry_np = L4.array<int32_t>(cap_entries),
               entry_count = L4.array<int32_t>(cap_entries);
    FAL_TRY(L4.reserve(ctx, SLOT_MSP4));
    FAL_CHECK_HIP(hipMemsetAsync(meta, 0, 64, ctx->stream));
    hipLaunchKernelGGL(msp_newlines_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, text, n_bytes, block_nl, meta);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, block_nl, n_tiles, block_base, SLOT_SORT));
    hipLaunchKernelGGL(msp_lines_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, text, n_bytes, block_base, n_tiles, start,
                       cap_lines, meta);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned line_grid = capped_grid(ctx, cap_lines, kBlockLines);
    hipLaunchKernelGGL(msp_classify_kernel, dim3(line_grid), dim3(256), 0, ctx->stream, text, n_bytes, start, meta, cls, seg, block_names);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(msp_blocks_kernel, dim3(1), dim3(64), 0, ctx->stream, block_names, block_first, meta);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(msp_entries_kernel, dim3(line_grid), dim3(256), 0, ctx->stream, cls, meta, block_first, cap_entries, entry_begin);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(msp_counts_kernel, dim3(capped_grid(ctx, cap_entries, 4)), dim3(256), 0, ctx->stream, cls, seg, meta, cap_entries,
                       entry_begin, entry_np, entry_count);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned long long* h = nullptr;
    FAL_TRY(read_meta(ctx, meta, &h));
    const int64_t flags = (int64_t)h[META_FLAGS];
    const bool overflow = (flags & FAL_MGF_FLAG_LINES) != 0;
    FAL_REQUIRE(overflow || (int64_t)h[META_ENTRIES] <= cap_entries, FAL_EINTERNAL, "fal_msp_index: more entries than 6-byte slots");
    counts_out[0] = overflow ? 0 : (int64_t)h[META_ENTRIES];
    counts_out[1] = overflow ? 0 : (int64_t)h[META_PEAKS];
    counts_out[2] = flags;
    counts_out[3] = (int64_t)h[META_LINES];
    store_index(ctx->msp, text, n_bytes, counts_out[0], counts_out[1], cap_lines, cap_entries, start, seg, meta, entry_begin);
    return FAL_OK;
}

extern "C" int fal_msp_parse(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_entries, int64_t nnz_cap, int64_t* out_indptr,
                             double* out_mz, float* out_intensity, double* precursor_mz, int32_t* charge, int32_t* has_charge,
                             int64_t* span, int32_t* status_out) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && out_indptr && n_entries >= 0 && nnz_cap >= 0, FAL_EINVAL, "fal_msp_parse: bad argument");
    const fal_ctx::TextIndex& ix = ctx->msp;
    FAL_REQUIRE(matches(ctx, ix, SLOT_MSP, text, n_bytes, n_entries), FAL_EINVAL,
                "fal_msp_parse: not the text, length and entry count of the last fal_msp_index of this context");
    if (n_entries == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int64_t), ctx->stream));
        return FAL_OK;
    }
    FAL_REQUIRE(nnz_cap >= ix.extra, FAL_EINVAL, "fal_msp_parse: nnz_cap %lld below the indexed peak count %lld", (long long)nnz_cap,
                (long long)ix.extra);
    FAL_REQUIRE(precursor_mz && charge && has_charge && span && status_out, FAL_EINVAL, "fal_msp_parse: NULL column");
    FAL_REQUIRE(ix.extra == 0 || (out_mz && out_intensity), FAL_EINVAL, "fal_msp_parse: NULL peaks");
    const int32_t* start = static_cast<const int32_t*>(ix.blocks[0]);
    const int32_t* seg = static_cast<const int32_t*>(ix.blocks[1]);
    const uint8_t* cls = reinterpret_cast<const uint8_t*>(seg + ix.cap_table);
    const int32_t* entry_begin = static_cast<const int32_t*>(ix.blocks[3]);
    const int32_t *entry_np = entry_begin + ix.cap_spectra + 1, *entry_count = entry_np + ix.cap_spectra;
    ScratchLayout L;
    const auto tmp_mz = L.array<double>(ix.extra);
    const auto tmp_it = L.array<float>(ix.extra);
    L.pad(64);
    FAL_TRY(L.reserve(ctx, SLOT_MSP5));
    FAL_TRY(device_scan_i32(ctx, entry_count, n_entries, out_indptr, SLOT_SORT));
    const unsigned grid = capped_grid(ctx, n_entries, 4);
    const MspOut out{precursor_mz, charge, has_charge, span, status_out};
    hipLaunchKernelGGL(msp_parse_kernel, dim3(grid), dim3(256), 0, ctx->stream, text, n_bytes, start, cls, seg, entry_begin, entry_np,
                       n_entries, out_indptr, nnz_cap, tmp_mz, tmp_it, out);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(msp_sort_kernel, dim3(grid), dim3(256), 0, ctx->stream, out_indptr, n_entries, nnz_cap, tmp_mz, tmp_it, out_mz,
                       out_intensity);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}

extern "C" int fal_msp_headers(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_entries, const uint8_t* keys,
                               const int64_t* key_ptr, const int32_t* key_kind, int n_keys, int64_t* span_out, int64_t* value_out,
                               int32_t* state_out) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_entries >= 0 && keys && key_ptr && key_kind, FAL_EINVAL, "fal_msp_headers: bad argument");
    MgfKeyTable table;
    FAL_TRY(key_table_from("fal_msp_headers", ':', false, keys, key_ptr, key_kind, n_keys, &table));
    const fal_ctx::TextIndex& ix = ctx->msp;
    FAL_REQUIRE(matches(ctx, ix, SLOT_MSP, text, n_bytes, n_entries), FAL_EINVAL,
                "fal_msp_headers: not the text, length and entry count of the last fal_msp_index of this context");
    if (n_entries == 0) return FAL_OK;
    FAL_REQUIRE(span_out && value_out && state_out, FAL_EINVAL, "fal_msp_headers: NULL output");
    const int32_t* start = static_cast<const int32_t*>(ix.blocks[0]);
    const int32_t* seg = static_cast<const int32_t*>(ix.blocks[1]);
    const uint8_t* cls = reinterpret_cast<const uint8_t*>(seg + ix.cap_table);
    const int32_t* entry_begin = static_cast<const int32_t*>(ix.blocks[3]);
    hipLaunchKernelGGL(msp_headers_kernel, dim3(capped_grid(ctx, n_entries, 4)), dim3(256), 0, ctx->stream, text, n_bytes, start, cls,
                       entry_begin, entry_begin + ix.cap_spectra + 1, n_entries, table, span_out, value_out, state_out);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
