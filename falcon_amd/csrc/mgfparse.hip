// MGF text on the device -> the raw peak CSR fal_process_spectra takes (indptr i64, m/z f64, intensity f32, peaks sorted by m/z
// inside every spectrum) plus the per-spectrum columns.  The per-line functions are mgfparse.h's (shared with the CPU tests); the
// grammar is DESIGN.md's "MGF on the device"; falcon_amd/ms_io/mgf_io.get_spectra is the reader all of this mirrors.
//
// fal_mgf_index (one synchronisation, at its end):
//   newlines : textscan.h's count walk over '\n', with the byte check of the device grammar; a device scan of the tile counts;
//   lines    : textscan.h's table walk (Shift 1): start[k] = first byte of line k (i32), start[lines] = n + 1;
//   classify : a block takes 256 consecutive lines, stages their bytes -- one contiguous range, so lines never straddle a tile --
//              into LDS with 16-byte loads per lane and classifies a line per thread from there (a range that does not fit the
//              tile is read from global memory); per block: first / last BEGIN-END marker and the spectra closed inside it;
//   blocks   : one wave carries "the last marker so far" and the spectrum count across the block summaries;
//   spectra  : an END IONS line whose previous marker is a BEGIN IONS line emits a spectrum (begin line, end line);
//   counts   : one wave per spectrum counts its peak lines; the total is the capacity the caller allocates.
// The line table is sized before the line count is known: n / 4 + 2 lines (a text with more is the host reader's,
// FAL_MGF_FLAG_LINES); a spectrum takes at least 20 bytes, so n / 20 + 2 spectrum rows always suffice.
//
// fal_mgf_parse: the tables stay in the context's SLOT_MGF* slots between the two calls (kept, not recomputed; checked against
// the text pointer, its length and the slot blocks).  A scan of the counts gives indptr; then one wave per spectrum: 64 lines at
// a time staged into the wave's LDS tile, a line per lane: header lines give title / pepmass / charge / rtinseconds (the last
// line of a key wins), peak lines convert two tokens and land at the spectrum's slot in line order (a scratch copy); the sort
// of peakdecode.hip (peaksort.h) moves them to the output.  Every write is bounded by the slot the index counted.
// fal_mgf_parse_ex is that call with a set of optional keys (FAL_MGF_OPT_TITLE: no TITLE is no reason for the host).
//
// fal_mgf_headers: a third consumer of the same index, the parse kernel's form: per spectrum and key of the caller's table
// (mgfkeys.h) the value range of the last header line of that key, a state, and for an integer key the value of its fast form.
// fal_text_rows: byte ranges of a text -> zero-padded rows of one width (the readers' string columns); needs no index.
#include <algorithm>
#include "common.h"
#include "ivf.h"
#include "mgfkeys.h"
#include "mgfparse.h"
#include "peaksort.h"
#include "textkeys.h"
#include "textscan.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kBlockLines = 256;                 // classify / spectra passes: a line per thread
constexpr int kStageBytes = 16384;               // classify: LDS tile of a block's 256 lines (64 bytes a line on average)
constexpr int kWaveStage = 4096;                 // parse: LDS tile of a wave's 64 lines
enum { META_LINES = META_COUNT, META_SPECTRA = 2, META_PEAKS = 3 };

// ---- newlines per 4 KB block + the byte grammar ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mgf_newlines_kernel(const uint8_t* __restrict__ text, int64_t n, int32_t* __restrict__ block_nl,
                                                           unsigned long long* __restrict__ meta) {
    newline_count_pass<FAL_MGF_FLAG_BYTES>(text, n, block_nl, meta);
}

// ---- the line table ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mgf_lines_kernel(const uint8_t* __restrict__ text, int64_t n, const int64_t* __restrict__ block_base,
                                                        int64_t n_blocks, int32_t* __restrict__ start, int64_t cap_lines,
                                                        unsigned long long* __restrict__ meta) {
    mark_table_pass<'\n', 1, FAL_MGF_FLAG_LINES>(text, n, block_base, n_blocks, start, cap_lines, meta);
}

__device__ __forceinline__ int64_t indexed_lines(const unsigned long long* meta) {      // 0 when the table overflowed
    return (meta[META_FLAGS] & FAL_MGF_FLAG_LINES) ? 0 : (int64_t)meta[META_LINES];
}

__device__ __forceinline__ int64_t line_blocks(int64_t lines) { return (lines + kBlockLines - 1) / kBlockLines; }

// the markers (BEGIN / END lines) of a block's 256 lines in line order, from the four waves' ballots
template <class F>
__device__ __forceinline__ void for_each_marker(const uint64_t* begins, const uint64_t* ends, const F& f) {
    for (int w = 0; w < 4; ++w) {
        uint64_t m = begins[w] | ends[w];
        while (m) {
            const int j = __builtin_ctzll(m);
            f(w * 64 + j, ((begins[w] >> j) & 1) ? MGF_BEGIN : MGF_END);
            m &= m - 1;
        }
    }
}

// ---- line classes + block summaries ------------------------------------------------------------------------------------------
// summary[blk] = {first marker kind or 0, last marker kind or 0, last marker line, spectra closed by BEGIN-END pairs inside it}
__global__ __launch_bounds__(256) void mgf_classify_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ start,
                                                           const unsigned long long* __restrict__ meta, uint8_t* __restrict__ cls,
                                                           int4* __restrict__ summary) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kStageBytes + 16];
    __shared__ uint64_t begins[4], ends[4];
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
        int kind = MGF_SKIP;
        if (line < l1) {
            const int64_t s = start[line];
            const int len = (int)(start[line + 1] - 1 - s);
            const uint8_t* p = staged ? tile + (s - (b0 & ~(int64_t)15)) : text + s;
            int lo, hi;
            kind = mgf_classify(p, len, &lo, &hi);
            cls[line] = (uint8_t)kind;
        }
        const uint64_t mb = __ballot(kind == MGF_BEGIN), me = __ballot(kind == MGF_END);
        if ((threadIdx.x & 63) == 0) {
            begins[threadIdx.x >> 6] = mb;
            ends[threadIdx.x >> 6] = me;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int first = 0, prev = 0, last_line = -1, closed = 0;
            for_each_marker(begins, ends, [&](int j, int kind_j) {
                if (!first) first = kind_j;
                closed += kind_j == MGF_END && prev == MGF_BEGIN;
                prev = kind_j;
                last_line = (int)l0 + j;
            });
            summary[blk] = make_int4(first, prev, last_line, closed);
        }
    }
}

// ---- carry over the blocks: one wave -------------------------------------------------------------------------------------------
// carry[blk] = {kind of the last marker before the block or 0, its line, index of the block's first spectrum, 0}
__global__ __launch_bounds__(64) void mgf_blocks_kernel(const int4* __restrict__ summary, int4* __restrict__ carry,
                                                        unsigned long long* __restrict__ meta) {
    const int lane = threadIdx.x;
    const int64_t n_blocks = line_blocks(indexed_lines(meta));
    int in_kind = 0, in_line = -1, base = 0;                                   // wave-uniform
    for (int64_t g = 0; g < n_blocks; g += 64) {
        const bool valid = g + lane < n_blocks;
        const int4 s = valid ? summary[g + lane] : make_int4(0, 0, -1, 0);
        const uint64_t has = __ballot(s.y != 0);
        const uint64_t below = has & ((uint64_t(1) << lane) - 1);
        const int src = below ? 63 - __builtin_clzll(below) : 0;
        const int k_src = __shfl(s.y, src, 64), l_src = __shfl(s.z, src, 64);
        const int my_kind = below ? k_src : in_kind, my_line = below ? l_src : in_line;
        const int closed = s.w + (s.x == MGF_END && my_kind == MGF_BEGIN);
        const int incl = wave_prefix_sum(closed);
        if (valid) carry[g + lane] = make_int4(my_kind, my_line, base + incl - closed, 0);
        base += __shfl(incl, 63, 64);
        if (has) {
            const int top = 63 - __builtin_clzll(has);
            in_kind = __shfl(s.y, top, 64);
            in_line = __shfl(s.z, top, 64);
        }
    }
    if (lane == 0) meta[META_SPECTRA] = (unsigned long long)base;
}

// ---- the spectrum table --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mgf_spectra_kernel(const uint8_t* __restrict__ cls, const unsigned long long* __restrict__ meta,
                                                          const int4* __restrict__ carry, int64_t cap_spectra, int32_t* __restrict__ spec_begin,
                                                          int32_t* __restrict__ spec_end) {
    __shared__ uint64_t begins[4], ends[4];
    const int64_t lines = indexed_lines(meta);
    const int64_t n_blocks = line_blocks(lines);
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t line = blk * kBlockLines + threadIdx.x;
        const int kind = line < lines ? cls[line] : MGF_SKIP;
        const uint64_t mb = __ballot(kind == MGF_BEGIN), me = __ballot(kind == MGF_END);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
            begins[threadIdx.x >> 6] = mb;
            ends[threadIdx.x >> 6] = me;
        }
        __syncthreads();
        if (threadIdx.x == 0 && (begins[0] | begins[1] | begins[2] | begins[3] | ends[0] | ends[1] | ends[2] | ends[3])) {
            const int4 c = carry[blk];
            int prev = c.x, prev_line = c.y;
            int64_t s = c.z;
            for_each_marker(begins, ends, [&](int j, int kind_j) {
                const int here = (int)(blk * kBlockLines) + j;
                if (kind_j == MGF_END && prev == MGF_BEGIN) {
                    if (s < cap_spectra) {
                        spec_begin[s] = prev_line;
                        spec_end[s] = here;
                    }
                    ++s;
                }
                prev = kind_j;
                prev_line = here;
            });
        }
    }
}

// ---- peak lines per spectrum ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mgf_counts_kernel(const uint8_t* __restrict__ cls, unsigned long long* __restrict__ meta,
                                                         int64_t cap_spectra, const int32_t* __restrict__ spec_begin,
                                                         const int32_t* __restrict__ spec_end, int32_t* __restrict__ spec_count) {
    const int lane = threadIdx.x & 63;
    const int64_t n_spec = std::min<int64_t>((int64_t)meta[META_SPECTRA], cap_spectra);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_spec; s += waves) {
        const int64_t b = spec_begin[s], e = spec_end[s];
        int cnt = 0;
        for (int64_t l = b + 1 + lane; l < e; l += 64) cnt += (cls[l] & MGF_KIND) == MGF_PEAK;
        cnt = __shfl(wave_prefix_sum(cnt), 63, 64);
        if (lane == 0) {
            spec_count[s] = cnt;
            atomicAdd(&meta[META_PEAKS], (unsigned long long)cnt);
        }
    }
}

// ---- parse: one wave per spectrum ----------------------------------------------------------------------------------------------
struct MgfOut {
    double* pmz;
    int32_t* charge;
    int32_t* has_charge;
    double* rt;
    int64_t* title;
    int64_t* span;
    int32_t* status;
};

__global__ __launch_bounds__(256) void mgf_parse_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ start,
                                                        const uint8_t* __restrict__ cls, const int32_t* __restrict__ spec_begin,
                                                        const int32_t* __restrict__ spec_end, int64_t n_spec,
                                                        const int64_t* __restrict__ indptr, int64_t nnz_cap, double* __restrict__ tmp_mz,
                                                        float* __restrict__ tmp_it, MgfOut out, int optional_keys) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4][kWaveStage + 16];
    const int lane = threadIdx.x & 63;
    uint8_t* tile = tiles[threadIdx.x >> 6];
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_spec; s += waves) {
        const int64_t b = spec_begin[s], e = spec_end[s];
        const int64_t slot = indptr[s], slot_end = std::min<int64_t>(indptr[s + 1], nnz_cap);
        // wave-uniform state: per key the last line's value
        bool host = false, has_title = false, has_pm = false, pm_ok = false, has_ch = false, ch_ok = false, has_rt = false, rt_ok = false;
        int64_t t_lo = 0, t_hi = 0, n_peaks = 0;
        double pm = 0.0, rt = -1.0;
        int ch = 0;
        for (int64_t g = b + 1; g < e; g += 64) {
            const int64_t g1 = std::min<int64_t>(g + 64, e);
            const int64_t b0 = start[g], b1 = std::min<int64_t>(start[g1], n), a0 = b0 & ~(int64_t)15;
            const bool staged = b1 - a0 <= kWaveStage;                         // wave-uniform
            if (staged) stage_bytes(text, n, b0, b1, tile, lane, 64);
            wave_lds_sync();
            const int64_t line = g + lane;
            int kind = MGF_SKIP, key = MGF_KEY_OTHER;
            bool ok = false, is_peak = false;
            double val = 0.0, val2 = 0.0;
            int64_t v_lo = 0, v_hi = 0;
            int ival = 0;
            if (line < g1) {
                const int c = cls[line];
                kind = c & MGF_KIND;
                const int64_t ls = start[line];
                const int len = (int)(start[line + 1] - 1 - ls);
                const uint8_t* p = staged ? tile + (ls - a0) : text + ls;
                if ((kind == MGF_HEADER || kind == MGF_PEAK) && (c & MGF_LONG)) {
                    host = true;                                               // the slot keeps its size; the host reader fills it
                    is_peak = kind == MGF_PEAK;
                    kind = MGF_SKIP;
                } else if (kind == MGF_PEAK) {
                    is_peak = true;
                    int lo = 0, hi = len, pos, t0, t1, u0, u1;
                    mgf_strip(p, &lo, &hi);
                    pos = lo;
                    mgf_token(p, &pos, hi, &t0, &t1);
                    mgf_token(p, &pos, hi, &u0, &u1);
                    ok = mgf_parse_double(p + t0, t1 - t0, &val);
                    if (u1 > u0) ok = mgf_parse_double(p + u0, u1 - u0, &val2) && ok;
                    if (!ok) {
                        host = true;
                        val = val2 = 0.0;
                    }
                } else if (kind == MGF_HEADER) {
                    int lo = 0, hi = len, a, z;
                    mgf_strip(p, &lo, &hi);
                    key = mgf_header(p, lo, hi, &a, &z);
                    v_lo = ls + a;
                    v_hi = ls + z;
                    if (key == MGF_KEY_PEPMASS) {                              // the first whitespace token; none: the host rejects it
                        int pos = a, t0, t1;
                        mgf_token(p, &pos, z, &t0, &t1);
                        ok = t1 > t0 && mgf_parse_double(p + t0, t1 - t0, &val);
                    } else if (key == MGF_KEY_RT) {
                        ok = mgf_parse_double(p + a, z - a, &val);
                    } else if (key == MGF_KEY_CHARGE) {
                        ok = mgf_parse_charge(p + a, z - a, &ival);
                    }
                }
            }
            const uint64_t peaks = __ballot(is_peak);
            if (is_peak) {
                const int64_t at = slot + n_peaks + __popcll(peaks & ((uint64_t(1) << lane) - 1));
                if (at < slot_end) {
                    tmp_mz[at] = val;
                    tmp_it[at] = (float)val2;
                }
            }
            n_peaks += __popcll(peaks);
            const uint64_t m_t = __ballot(key == MGF_KEY_TITLE), m_p = __ballot(key == MGF_KEY_PEPMASS);
            const uint64_t m_c = __ballot(key == MGF_KEY_CHARGE), m_r = __ballot(key == MGF_KEY_RT);
            if (m_t) {
                const int src = 63 - __builtin_clzll(m_t);
                has_title = true;
                t_lo = __shfl(v_lo, src, 64);
                t_hi = __shfl(v_hi, src, 64);
            }
            if (m_p) {
                const int src = 63 - __builtin_clzll(m_p);
                has_pm = true;
                pm_ok = __shfl((int)ok, src, 64) != 0;
                pm = __shfl(val, src, 64);
            }
            if (m_c) {
                const int src = 63 - __builtin_clzll(m_c);
                has_ch = true;
                ch_ok = __shfl((int)ok, src, 64) != 0;
                ch = __shfl(ival, src, 64);
            }
            if (m_r) {
                const int src = 63 - __builtin_clzll(m_r);
                has_rt = true;
                rt_ok = __shfl((int)ok, src, 64) != 0;
                rt = __shfl(val, src, 64);
            }
        }
        host = __ballot(host) != 0 || (!has_title && !(optional_keys & FAL_MGF_OPT_TITLE)) || !has_pm || !pm_ok || (has_ch && !ch_ok) || (has_rt && !rt_ok);
        if (lane == 0) {
            out.pmz[s] = has_pm && pm_ok ? pm : 0.0;
            out.charge[s] = has_ch && ch_ok ? ch : 0;
            out.has_charge[s] = has_ch ? 1 : 0;
            out.rt[s] = has_rt ? (rt_ok ? rt : 0.0) : -1.0;
            out.title[2 * s] = has_title ? t_lo : 0;
            out.title[2 * s + 1] = has_title ? t_hi : 0;
            out.span[2 * s] = start[b];
            out.span[2 * s + 1] = std::min<int64_t>(start[e + 1], n);
            out.status[s] = host ? FAL_MGF_ST_HOST : 0;
        }
    }
}

// ---- sort: the scratch copy -> the output ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mgf_sort_kernel(const int64_t* __restrict__ indptr, int64_t n_spec, int64_t nnz_cap,
                                                       const double* __restrict__ tmp_mz, const float* __restrict__ tmp_it,
                                                       double* __restrict__ out_mz, float* __restrict__ out_it) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_spec; s += waves) {
        const int64_t b = indptr[s], e = indptr[s + 1];
        if (e > nnz_cap) continue;                                             // (the entry point refuses such a capacity)
        wave_sort_peaks(e - b, lane, [&](int64_t j) { return tmp_mz[b + j]; }, [&](int64_t j) { return tmp_it[b + j]; }, out_mz + b,
                        out_it + b);
    }
}

// ---- header values by a key table: one wave per spectrum -----------------------------------------------------------------------
// mgf_parse_kernel's form over the same index; the body is textkeys.h's, shared with fal_msp_headers: here the separator is '='
// and the lines scanned are the spectrum's header lines between BEGIN IONS and END IONS.
__global__ __launch_bounds__(256) void mgf_headers_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ start,
                                                          const uint8_t* __restrict__ cls, const int32_t* __restrict__ spec_begin,
                                                          const int32_t* __restrict__ spec_end, int64_t n_spec, MgfKeyTable table,
                                                          int64_t* __restrict__ span_out, int64_t* __restrict__ value_out,
                                                          int32_t* __restrict__ state_out) {
    headers_pass<'='>(
        text, n, start, cls, n_spec, table, span_out, value_out, state_out,
        [&](int64_t s, int64_t* first, int64_t* last) {
            *first = (int64_t)spec_begin[s] + 1;
            *last = spec_end[s];
        },
        [](int c) { return (c & MGF_KIND) == MGF_HEADER; });
}

// ---- byte ranges -> fixed-width rows ---------------------------------------------------------------------------------------------
// a thread per four bytes of a row; a range outside the text gives a zero row and sets the call's range flag
constexpr unsigned long long kTextFlagRange = 1;
__global__ __launch_bounds__(256) void text_rows_kernel(const uint8_t* __restrict__ text, int64_t n_bytes, const int64_t* __restrict__ span,
                                                        int64_t stride, int64_t column, int64_t n, int width, uint8_t* __restrict__ rows_out,
                                                        int32_t* __restrict__ long_out, unsigned long long* __restrict__ meta) {
    const int groups = (width + 3) / 4;
    const int64_t total = n * groups, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t r = i / groups;
        const int q = (int)(i - r * groups);
        const int64_t from = span[(r * stride + column) * 2], to = span[(r * stride + column) * 2 + 1];
        const bool ok = from >= 0 && to >= from && to <= n_bytes;
        const int64_t len = ok ? to - from : 0;
        if (q == 0) {
            long_out[r] = len > width ? 1 : 0;
            if (!ok) atomicOr(&meta[META_FLAGS], kTextFlagRange);
        }
        for (int c = 4 * q; c < std::min(4 * q + 4, width); ++c) rows_out[r * width + c] = c < len ? text[from + c] : (uint8_t)0;
    }
}

FAL_WARM_KERNEL(mgf_parse_kernel);

}  // namespace
}  // namespace fal

using namespace fal;

extern "C" int fal_mgf_index(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t* counts_out) {
    fal::CallScope _call(ctx);
    FAL_TRY(text_index_begin("fal_mgf_index", ctx, &fal_ctx::mgf, text, n_bytes, counts_out));
    if (n_bytes == 0) {
        counts_out[3] = 1;                                                      // (lines = '\n' + 1, as for every other text)
        return FAL_OK;
    }
    const int64_t n_tiles = ceil_div(n_bytes, kTileBytes);
    const int64_t cap_lines = n_bytes / 4 + 2, cap_spectra = n_bytes / 20 + 2, cap_blocks = ceil_div(cap_lines, kBlockLines);
    int32_t* start = nullptr;
    uint8_t* cls = nullptr;
    FAL_TRY(ctx->reserve(SLOT_MGF, sizeof(int32_t) * (size_t)(cap_lines + 1), (void**)&start));
    FAL_TRY(ctx->reserve(SLOT_MGF2, (size_t)cap_lines, (void**)&cls));
    ScratchLayout L3, L4;
    const auto meta = L3.array<unsigned long long>(8);                              // 64 B of meta words
    const auto summary = L3.array<int4>(cap_blocks), carry = L3.array<int4>(cap_blocks);
    const auto block_base = L3.array<int64_t>(n_tiles + 1);                         // the scan of the newline counts
    const auto block_nl = L3.array<int32_t>(n_tiles + 2);
    L3.pad(72);
    FAL_TRY(L3.reserve(ctx, SLOT_MGF3));
    const auto spec_begin = L4.array<int32_t>(cap_spectra), spec_end = L4.array<int32_t>(cap_spectra), spec_count = L4.array<int32_t>(cap_spectra);
    FAL_TRY(L4.reserve(ctx, SLOT_MGF4));
    FAL_CHECK_HIP(hipMemsetAsync(meta, 0, 64, ctx->stream));
    hipLaunchKernelGGL(mgf_newlines_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, text, n_bytes, block_nl, meta);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, block_nl, n_tiles, block_base, SLOT_SORT));
    hipLaunchKernelGGL(mgf_lines_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, text, n_bytes, block_base, n_tiles, start,
                       cap_lines, meta);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned line_grid = capped_grid(ctx, cap_lines, kBlockLines);
    hipLaunchKernelGGL(mgf_classify_kernel, dim3(line_grid), dim3(256), 0, ctx->stream, text, n_bytes, start, meta, cls, summary);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(mgf_blocks_kernel, dim3(1), dim3(64), 0, ctx->stream, summary, carry, meta);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(mgf_spectra_kernel, dim3(line_grid), dim3(256), 0, ctx->stream, cls, meta, carry, cap_spectra, spec_begin,
                       spec_end);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(mgf_counts_kernel, dim3(capped_grid(ctx, cap_spectra, 4)), dim3(256), 0, ctx->stream, cls, meta, cap_spectra,
                       spec_begin, spec_end, spec_count);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned long long* h = nullptr;
    FAL_TRY(read_meta(ctx, meta, &h));
    const int64_t flags = (int64_t)h[META_FLAGS];
    const bool overflow = (flags & FAL_MGF_FLAG_LINES) != 0;
    FAL_REQUIRE(overflow || (int64_t)h[META_SPECTRA] <= cap_spectra, FAL_EINTERNAL, "fal_mgf_index: more spectra than 20-byte slots");
    counts_out[0] = overflow ? 0 : (int64_t)h[META_SPECTRA];
    counts_out[1] = overflow ? 0 : (int64_t)h[META_PEAKS];
    counts_out[2] = flags;
    counts_out[3] = (int64_t)h[META_LINES];
    store_index(ctx->mgf, text, n_bytes, counts_out[0], counts_out[1], cap_lines, cap_spectra, start, cls, meta, spec_begin);
    return FAL_OK;
}

extern "C" int fal_mgf_parse_ex(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, int64_t nnz_cap,
                                int64_t* out_indptr, double* out_mz, float* out_intensity, double* precursor_mz, int32_t* charge,
                                int32_t* has_charge, double* retention_time, int64_t* title, int64_t* span, int32_t* status_out,
                                int optional_keys) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && out_indptr && n_spectra >= 0 && nnz_cap >= 0, FAL_EINVAL, "fal_mgf_parse: bad argument");
    FAL_REQUIRE((optional_keys & ~FAL_MGF_OPT_TITLE) == 0, FAL_EINVAL, "fal_mgf_parse: unknown optional_keys bits %d", optional_keys);
    const fal_ctx::TextIndex& ix = ctx->mgf;
    FAL_REQUIRE(matches(ctx, ix, SLOT_MGF, text, n_bytes, n_spectra), FAL_EINVAL,
                "fal_mgf_parse: not the text, length and spectrum count of the last fal_mgf_index of this context");
    if (n_spectra == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int64_t), ctx->stream));
        return FAL_OK;
    }
    FAL_REQUIRE(nnz_cap >= ix.extra, FAL_EINVAL, "fal_mgf_parse: nnz_cap %lld below the indexed peak count %lld", (long long)nnz_cap,
                (long long)ix.extra);
    FAL_REQUIRE(precursor_mz && charge && has_charge && retention_time && title && span && status_out, FAL_EINVAL,
                "fal_mgf_parse: NULL column");
    FAL_REQUIRE(ix.extra == 0 || (out_mz && out_intensity), FAL_EINVAL, "fal_mgf_parse: NULL peaks");
    const int32_t* start = static_cast<const int32_t*>(ix.blocks[0]);
    const uint8_t* cls = static_cast<const uint8_t*>(ix.blocks[1]);
    const int32_t* spec = static_cast<const int32_t*>(ix.blocks[3]);
    const int32_t *spec_begin = spec, *spec_end = spec + ix.cap_spectra, *spec_count = spec + 2 * ix.cap_spectra;
    ScratchLayout L;
    const auto tmp_mz = L.array<double>(ix.extra);
    const auto tmp_it = L.array<float>(ix.extra);
    L.pad(64);
    FAL_TRY(L.reserve(ctx, SLOT_MGF5));
    FAL_TRY(device_scan_i32(ctx, spec_count, n_spectra, out_indptr, SLOT_SORT));
    const unsigned grid = capped_grid(ctx, n_spectra, 4);
    const MgfOut out{precursor_mz, charge, has_charge, retention_time, title, span, status_out};
    hipLaunchKernelGGL(mgf_parse_kernel, dim3(grid), dim3(256), 0, ctx->stream, text, n_bytes, start, cls, spec_begin, spec_end, n_spectra,
                       out_indptr, nnz_cap, tmp_mz, tmp_it, out, optional_keys);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(mgf_sort_kernel, dim3(grid), dim3(256), 0, ctx->stream, out_indptr, n_spectra, nnz_cap, tmp_mz, tmp_it, out_mz,
                       out_intensity);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}

extern "C" int fal_mgf_parse(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, int64_t nnz_cap,
                             int64_t* out_indptr, double* out_mz, float* out_intensity, double* precursor_mz, int32_t* charge,
                             int32_t* has_charge, double* retention_time, int64_t* title, int64_t* span, int32_t* status_out) {
    return fal_mgf_parse_ex(ctx, text, n_bytes, n_spectra, nnz_cap, out_indptr, out_mz, out_intensity, precursor_mz, charge, has_charge,
                            retention_time, title, span, status_out, 0);
}

extern "C" int fal_mgf_headers(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, const uint8_t* keys,
                               const int64_t* key_ptr, const int32_t* key_kind, int n_keys, int64_t* span_out, int64_t* value_out,
                               int32_t* state_out) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_spectra >= 0 && keys && key_ptr && key_kind, FAL_EINVAL, "fal_mgf_headers: bad argument");
    MgfKeyTable table;
    FAL_TRY(key_table_from("fal_mgf_headers", '=', true, keys, key_ptr, key_kind, n_keys, &table));
    const fal_ctx::TextIndex& ix = ctx->mgf;
    FAL_REQUIRE(matches(ctx, ix, SLOT_MGF, text, n_bytes, n_spectra), FAL_EINVAL,
                "fal_mgf_headers: not the text, length and spectrum count of the last fal_mgf_index of this context");
    if (n_spectra == 0) return FAL_OK;
    FAL_REQUIRE(span_out && value_out && state_out, FAL_EINVAL, "fal_mgf_headers: NULL output");
    const int32_t* start = static_cast<const int32_t*>(ix.blocks[0]);
    const uint8_t* cls = static_cast<const uint8_t*>(ix.blocks[1]);
    const int32_t* spec = static_cast<const int32_t*>(ix.blocks[3]);
    hipLaunchKernelGGL(mgf_headers_kernel, dim3(capped_grid(ctx, n_spectra, 4)), dim3(256), 0, ctx->stream, text, n_bytes, start, cls, spec,
                       spec + ix.cap_spectra, n_spectra, table, span_out, value_out, state_out);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}

extern "C" int fal_text_rows(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, const int64_t* span, int64_t stride, int64_t column,
                             int64_t n, int width, uint8_t* rows_out, int32_t* long_out) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && n_bytes >= 0 && stride >= 1 && column >= 0 && column < stride, FAL_EINVAL, "fal_text_rows: bad argument");
    FAL_REQUIRE(width >= 1 && width <= FAL_TEXT_MAX_WIDTH, FAL_EINVAL, "fal_text_rows: width %d, 1 to %d are taken", width,
                FAL_TEXT_MAX_WIDTH);
    if (n == 0) return FAL_OK;
    FAL_REQUIRE((text || n_bytes == 0) && span && rows_out && long_out, FAL_EINVAL, "fal_text_rows: NULL argument");
    unsigned long long* meta = nullptr;
    FAL_TRY(ctx->reserve(SLOT_MGF5, sizeof(unsigned long long) * META_WORDS, (void**)&meta));
    FAL_CHECK_HIP(hipMemsetAsync(meta, 0, sizeof(unsigned long long) * META_WORDS, ctx->stream));
    hipLaunchKernelGGL(text_rows_kernel, dim3(capped_grid(ctx, n * ((width + 3) / 4), 256)), dim3(256), 0, ctx->stream, text, n_bytes, span,
                       stride, column, n, width, rows_out, long_out, meta);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned long long* h = nullptr;
    FAL_TRY(read_meta(ctx, meta, &h));
    FAL_REQUIRE((h[META_FLAGS] & kTextFlagRange) == 0, FAL_EINVAL, "fal_text_rows: a range lies outside the text (its row is zero)");
    return FAL_OK;
}
