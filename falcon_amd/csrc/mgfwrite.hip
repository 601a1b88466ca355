// Peak CSR + per-entry columns on the device -> the text of a representative MGF, byte for byte what
// falcon_amd/ms_io/mgf_io.write_spectra writes for the same entries.  The per-number and per-field functions are mgfwrite.h's
// (shared with the CPU tests); DESIGN.md "MGF out of the device" has the layout and the number algorithm.
//
// fal_mgf_write_sizes (one synchronisation, at its end): one wave per entry adds up its text -- the lanes take the peak lines 64
// at a time, lanes 0-3 the four fields behind the title -- then the library's scan (device_scan_i64) turns the sizes into offsets.
//
// fal_mgf_write (one synchronisation, at its end): one wave per entry.  The wave owns a kWriteTile-byte LDS tile and appends the
// entry to it with textwrite.h's pieces: the head from lane 0; the title copied lane-strided; the four fields and then the peak
// lines, 64 at a time, a lane each at a wave prefix sum of their lengths (the digits are computed again rather than kept from
// the sizing pass); the tail.  Every store is bounded by the entry's own range [offset[k], offset[k + 1]) - offset[first],
// checked against out_bytes before anything is written.
#include <algorithm>
#include "common.h"
#include "mgfwrite.h"
#include "textwrite.h"

namespace fal {
namespace {

constexpr int kWriteTile = 3136;                 // >= the bytes carried over + 64 peak lines of kMgfPeakMax bytes; a multiple of 16
constexpr int kTitleChunk = 2048;                // title bytes appended per piece
static_assert(kTileCarry + 64 * kMgfPeakMax <= kWriteTile && kTileCarry + kTitleChunk <= kWriteTile && kTileCarry + kMgfHeadLen <= kWriteTile &&
                  kWriteTile % 16 == 0, "the tile takes one round's text behind what the last flush left");

struct MgfEntries {
    const float* mz;
    const float* intensity;
    const int64_t* indptr;
    int64_t n_rows, nnz;
    const int32_t* rows;
    const float* pm;
    const float* rt;
    const int32_t* charge;
    const int64_t* cluster;
    const uint8_t* title;
    const int64_t* title_ptr;
    int64_t title_bytes;
};

// the peak range and the title range of entry k, both inside their arrays (an entry whose ranges are not: empty ranges, *bad set)
__device__ __forceinline__ void entry_ranges(const MgfEntries& e, int64_t k, int64_t* p0, int64_t* p1, int64_t* t0, int64_t* t1, bool* bad) {
    const int64_t r = e.rows[k];
    *p0 = *p1 = *t0 = *t1 = 0;
    *bad = false;
    if (r < 0 || r >= e.n_rows) {
        *bad = true;
    } else {
        const int64_t a = e.indptr[r], b = e.indptr[r + 1];
        if (a < 0 || b < a || b > e.nnz) *bad = true;
        else {
            *p0 = a;
            *p1 = b;
        }
    }
    const int64_t a = e.title_ptr[k], b = e.title_ptr[k + 1];
    if (a < 0 || b < a || b > e.title_bytes) *bad = true;
    else {
        *t0 = a;
        *t1 = b;
    }
}

// ---- sizes: one wave per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mgf_write_sizes_kernel(MgfEntries e, int64_t n, int64_t* __restrict__ sizes,
                                                              unsigned long long* __restrict__ meta) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t k = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); k < n; k += waves) {
        int64_t p0, p1, t0, t1;
        bool bad;
        entry_ranges(e, k, &p0, &p1, &t0, &t1, &bad);
        int64_t len = 0;
        if (lane < kMgfFields) len = mgf_field_len(lane, e.pm[k], e.charge[k], e.rt[k], e.cluster[k]);
        for (int64_t j = p0 + lane; j < p1; j += 64) len += mgf_peak_len(e.mz[j], e.intensity[j]);
        len = wave_xor_reduce(len, [](int64_t a, int64_t b) { return a + b; });
        if (lane == 0) {
            sizes[k] = kMgfHeadLen + (t1 - t0) + len + kMgfTailLen;
            if (bad) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
        }
    }
}

// ---- write: one wave per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mgf_write_kernel(MgfEntries e, const int64_t* __restrict__ offsets, int64_t first, int64_t last,
                                                        uint8_t* __restrict__ out, int64_t out_bytes, unsigned long long* __restrict__ meta) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4][kWriteTile];
    const int lane = threadIdx.x & 63;
    const int64_t base = offsets[first], need = offsets[last] - base;
    if (need < 0 || need > out_bytes) {                                          // uniform over the grid: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_TOO_SMALL);
        return;
    }
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t k = first + blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); k < last; k += waves) {
        const int64_t g0 = offsets[k] - base, g1 = offsets[k + 1] - base;
        if (g0 < 0 || g1 < g0 || g1 > need) {                                    // offsets that are no scan of sizes
            if (lane == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
            continue;
        }
        int64_t p0, p1, t0, t1;
        bool bad;
        entry_ranges(e, k, &p0, &p1, &t0, &t1, &bad);
        Tile t = tile_open(tiles[threadIdx.x >> 6], out + g0, out + g1);
        tile_append_by_lane0(t, kMgfHeadLen, lane, [](uint8_t* dst) { mgf_write_head(dst); });      // BEGIN IONS / TITLE=
        tile_append_bytes<kTitleChunk>(t, e.title + t0, t1 - t0, lane);
        const float pm = e.pm[k], rt = e.rt[k];                                  // the four fields, a lane each
        const int32_t ch = e.charge[k];
        const int64_t cl = e.cluster[k];
        tile_append_by_lanes(t, lane < kMgfFields ? mgf_field_len(lane, pm, ch, rt, cl) : 0, lane,
                             [&](uint8_t* dst) { mgf_write_field(dst, lane, pm, ch, rt, cl); });
        for (int64_t g = p0; g < p1; g += 64) {                                  // the peak lines, 64 at a time
            const int64_t j = g + lane;
            const bool on = j < p1;
            const float m = on ? e.mz[j] : 0.f, v = on ? e.intensity[j] : 0.f;
            tile_append_by_lanes(t, on ? mgf_peak_len(m, v) : 0, lane, [&](uint8_t* dst) { mgf_write_peak(dst, m, v); });
        }
        tile_append_by_lane0(t, kMgfTailLen, lane, [](uint8_t* dst) { mgf_write_tail(dst); });      // END IONS
        tile_close(t, lane, meta);
    }
}

FAL_WARM_KERNEL(mgf_write_kernel);

int check_entries(const char* who, fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_rows, int64_t nnz,
                  const int32_t* rows, int64_t n, const float* pm, const float* rt, const int32_t* charge, const int64_t* cluster,
                  const int64_t* title_ptr, int64_t title_bytes) {
    FAL_REQUIRE(ctx && n >= 0 && n_rows >= 0 && nnz >= 0 && title_bytes >= 0, FAL_EINVAL, "%s: bad argument", who);
    FAL_REQUIRE(n == 0 || (indptr && rows && pm && rt && charge && cluster && title_ptr), FAL_EINVAL, "%s: NULL column", who);
    FAL_REQUIRE(nnz == 0 || (mz && intensity), FAL_EINVAL, "%s: NULL peaks", who);
    return FAL_OK;
}

}  // namespace
}  // namespace fal

using namespace fal;

extern "C" int fal_mgf_write_sizes(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_rows, int64_t nnz,
                                   const int32_t* rows, int64_t n, const float* precursor_mz, const float* retention_time,
                                   const int32_t* charge, const int64_t* cluster, const int64_t* title_ptr, int64_t title_bytes,
                                   int64_t* sizes_out, int64_t* offsets_out, int64_t* total_out) {
    fal::CallScope _call(ctx);
    FAL_TRY(check_entries("fal_mgf_write_sizes", ctx, mz, intensity, indptr, n_rows, nnz, rows, n, precursor_mz, retention_time, charge,
                          cluster, title_ptr, title_bytes));
    FAL_REQUIRE(offsets_out && total_out && (n == 0 || sizes_out), FAL_EINVAL, "fal_mgf_write_sizes: NULL output");
    *total_out = 0;
    if (n == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(offsets_out, 0, sizeof(int64_t), ctx->stream));
        return FAL_OK;
    }
    unsigned long long* meta = nullptr;
    FAL_TRY(writer_meta(ctx, SLOT_MGFW, &meta));
    const MgfEntries e{mz, intensity, indptr, n_rows, nnz, rows, precursor_mz, retention_time, charge, cluster, nullptr, title_ptr, title_bytes};
    hipLaunchKernelGGL(mgf_write_sizes_kernel, dim3(capped_grid(ctx, n, 4)), dim3(256), 0, ctx->stream, e, n, sizes_out, meta);
    return finish_sizes(ctx, meta, sizes_out, n, offsets_out, total_out,
                        "fal_mgf_write_sizes: a row outside the CSR, or indptr / title_ptr not ascending inside their arrays");
}

extern "C" int fal_mgf_write(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_rows, int64_t nnz,
                             const int32_t* rows, int64_t n, const float* precursor_mz, const float* retention_time, const int32_t* charge,
                             const int64_t* cluster, const uint8_t* title, const int64_t* title_ptr, int64_t title_bytes,
                             const int64_t* offsets, int64_t first, int64_t last, uint8_t* out, int64_t out_bytes, uint8_t* host_out) {
    fal::CallScope _call(ctx);
    FAL_TRY(check_entries("fal_mgf_write", ctx, mz, intensity, indptr, n_rows, nnz, rows, n, precursor_mz, retention_time, charge, cluster,
                          title_ptr, title_bytes));
    FAL_REQUIRE(offsets && first >= 0 && first <= last && last <= n && out_bytes >= 0 && (out || out_bytes == 0) &&
                    (title || title_bytes == 0),
                FAL_EINVAL, "fal_mgf_write: bad argument");
    unsigned long long* meta = nullptr;
    FAL_TRY(writer_meta(ctx, SLOT_MGFW, &meta));
    const MgfEntries e{mz, intensity, indptr, n_rows, nnz, rows, precursor_mz, retention_time, charge, cluster, title, title_ptr, title_bytes};
    hipLaunchKernelGGL(mgf_write_kernel, dim3(capped_grid(ctx, std::max<int64_t>(last - first, 1), 4)), dim3(256), 0, ctx->stream, e, offsets,
                       first, last, out, out_bytes, meta);
    return finish_write(ctx, meta, "fal_mgf_write", "entries", "an entry", first, last, out, out_bytes, host_out);
}
