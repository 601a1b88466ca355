// The cluster CSV's columns on the device -> the order of its rows and their text, byte for byte what falcon.py's
// `_write_outputs` sort and `_write_cluster_info` give for the same rows.  The comparator, the number text, the quoting and the row
// layout are csvwrite.h's (shared with the CPU tests); DESIGN.md "Cluster CSV out of the device" has the key order and the mapping.
//
// fal_csv_order: a check pass (a lane per row: id_ptr ascending inside the blob, the longest digit run; one synchronisation), then
// rocprim's stable merge sort of the row indices under (file_rank, csv_natural_cmp of the ids, index).  The comparator reads the
// id blob through id_ptr, which the check pass has bounded; an index outside [0, n) compares by itself alone and reads nothing.
//
// fal_csv_write_sizes (one synchronisation, at its end): a lane per row adds up its text (textwrite.h's sizes_by_lane), then the
// library's scan turns the sizes into offsets.
//
// fal_csv_write (one synchronisation, at its end): a lane per row, a wave per tile of 64 consecutive rows -- textwrite.h's
// write_units_by_lane, which has the rounds, the tile and every bound on a store.  What this unit gives it is CsvUnits: a lane
// keeps its row measured (the digits are made once per round and kept for the text), and a row that no tile takes (longer than
// kCsvTile - 15 bytes) is written by its lane alone, straight into its own range.
#include <algorithm>
#include <rocprim/device/device_merge_sort.hpp>
#include "common.h"
#include "csvwrite.h"
#include "textwrite.h"

namespace fal {
namespace {

constexpr int kCsvTile = 8192;                   // bytes of a wave's tile; a multiple of 16
constexpr int kCsvSortBlock = 1024;              // rows per block of the merge sort's first pass (include/falcon_hip.h FAL_CSV_SORT_BLOCK)
static_assert(kCsvTile % 16 == 0 && kCsvTile >= 64 * (kCsvFixedMax + 16), "a tile takes 64 rows with short text fields");
static_assert(kCsvSortBlock == FAL_CSV_SORT_BLOCK, "the header states the sort's block size");
// block sort of 256 threads x 4 rows; merge path from 16,384 rows on (below: the odd-even merge)
using CsvSortConfig = rocprim::merge_sort_config<256, 256, kCsvSortBlock / 256, 128, 128, 4, (1 << 14)>;
enum { META_DIGITS = 2 };                                            // meta word: the longest digit run

struct CsvColumns {
    const int32_t* order;        // row k of the text is input row order[k]; NULL: k
    const int32_t* file_id;
    const uint8_t* fn;
    const int64_t* fn_ptr;
    int64_t n_files, fn_bytes;
    const uint8_t* id;
    const int64_t* id_ptr;
    int64_t id_bytes;
    const int32_t* charge;
    const float* pm;
    const float* rt;
    const int64_t* cluster;
    int64_t n;
    bool quote_cr;
};

// row k of the text, measured; *bad when the row, its file or a byte range lies outside its array (then an empty row)
__device__ __forceinline__ CsvRow load_row(const CsvColumns& c, int64_t k, bool* bad) {
    const int64_t r = c.order ? (int64_t)c.order[k] : k;
    *bad = r < 0 || r >= c.n;
    int64_t f0 = 0, f1 = 0, i0 = 0, i1 = 0;
    int32_t charge = 0;
    float pm = 0.f, rt = 0.f;
    int64_t cluster = 0;
    if (!*bad) {
        const int64_t f = c.file_id[r];
        if (f < 0 || f >= c.n_files) {
            *bad = true;
        } else {
            f0 = c.fn_ptr[f];
            f1 = c.fn_ptr[f + 1];
            if (f0 < 0 || f1 < f0 || f1 > c.fn_bytes) *bad = true;
        }
        i0 = c.id_ptr[r];
        i1 = c.id_ptr[r + 1];
        if (i0 < 0 || i1 < i0 || i1 > c.id_bytes) *bad = true;
        charge = c.charge[r];
        pm = c.pm[r];
        rt = c.rt[r];
        cluster = c.cluster[r];
    }
    if (*bad) f0 = f1 = i0 = i1 = 0;
    return csv_row(c.fn + f0, f1 - f0, c.id + i0, i1 - i0, charge, pm, rt, cluster, c.quote_cr);
}

// ---- order ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void csv_check_ids_kernel(const uint8_t* __restrict__ id, const int64_t* __restrict__ id_ptr, int64_t id_bytes,
                                                            int64_t n, int32_t* __restrict__ iota, unsigned long long* __restrict__ meta) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    unsigned long long longest = 0;
    bool bad = false;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += step) {
        iota[r] = (int32_t)r;
        const int64_t a = id_ptr[r], b = id_ptr[r + 1];
        if (a < 0 || b < a || b > id_bytes) bad = true;
        else longest = std::max<unsigned long long>(longest, (unsigned long long)csv_max_digit_run(id + a, b - a));
    }
    if (bad) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
    if (longest) atomicMax(&meta[META_DIGITS], longest);
}

struct CsvRowLess {
    const int32_t* file_rank;
    const uint8_t* id;
    const int64_t* id_ptr;
    int64_t n;
    __device__ bool operator()(const int32_t& a, const int32_t& b) const {
        if (a == b) return false;
        if ((uint32_t)a >= (uint64_t)n || (uint32_t)b >= (uint64_t)n) return a < b;          // (never a row: reads nothing)
        const int32_t ra = file_rank[a], rb = file_rank[b];
        if (ra != rb) return ra < rb;
        const int64_t a0 = id_ptr[a], b0 = id_ptr[b];
        const int c = csv_natural_cmp(id + a0, id_ptr[a + 1] - a0, id + b0, id_ptr[b + 1] - b0);
        return c != 0 ? c < 0 : a < b;
    }
};

// ---- the rows as textwrite.h's lane-per-unit writers take them ----------------------------------------------------------------------------
struct CsvUnits {
    typedef CsvRow Unit;                                                         // the row measured: its digits are made once and kept for the text
    static constexpr bool kLongByWave = false;                                   // a row that no tile takes: lane 0 alone, straight into its range
    const CsvColumns& c;
    __device__ CsvRow load(int64_t k, bool* bad) const { return load_row(c, k, bad); }
    __device__ int64_t len(const CsvRow& row) const { return csv_row_len(row); }
    __device__ int64_t write(uint8_t* dst, const CsvRow& row, int64_t) const { return csv_write_row(dst, row); }
};

__global__ __launch_bounds__(256) void csv_write_sizes_kernel(CsvColumns c, int64_t rows, int64_t* __restrict__ sizes,
                                                              unsigned long long* __restrict__ meta) {
    sizes_by_lane(CsvUnits{c}, rows, sizes, meta);
}

__global__ __launch_bounds__(256) void csv_write_kernel(CsvColumns c, const int64_t* __restrict__ offsets, int64_t first, int64_t last,
                                                        uint8_t* __restrict__ out, int64_t out_bytes, unsigned long long* __restrict__ meta) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4][kCsvTile];
    write_units_by_lane<kCsvTile>(CsvUnits{c}, tiles[threadIdx.x >> 6], offsets, first, last, out, out_bytes, meta);
}

FAL_WARM_KERNEL(csv_write_kernel);

int check_columns(const char* who, fal_ctx* ctx, const int32_t* file_id, const int64_t* fn_ptr, int64_t n_files, int64_t fn_bytes,
                  const int64_t* id_ptr, int64_t id_bytes, const int32_t* charge, const float* pm, const float* rt, const int64_t* cluster,
                  int64_t n, int64_t rows) {
    FAL_REQUIRE(ctx && n >= 0 && n < (int64_t(1) << 31) && rows >= 0 && n_files >= 0 && fn_bytes >= 0 && id_bytes >= 0, FAL_EINVAL,
                "%s: bad argument", who);
    FAL_REQUIRE(rows == 0 || (n > 0 && file_id && fn_ptr && id_ptr && charge && pm && rt && cluster), FAL_EINVAL, "%s: NULL column", who);
    return FAL_OK;
}

}  // namespace
}  // namespace fal

using namespace fal;

extern "C" int fal_csv_order(fal_ctx* ctx, const int32_t* file_rank, const uint8_t* id, const int64_t* id_ptr, int64_t id_bytes, int64_t n,
                             int32_t* order_out, int64_t* max_digit_run_out) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && n < (int64_t(1) << 31) && id_bytes >= 0 && max_digit_run_out, FAL_EINVAL, "fal_csv_order: bad argument");
    FAL_REQUIRE(n == 0 || (file_rank && id_ptr && order_out && (id || id_bytes == 0)), FAL_EINVAL, "fal_csv_order: NULL column");
    *max_digit_run_out = 0;
    if (n == 0) return FAL_OK;
    const CsvRowLess less{file_rank, id, id_ptr, n};
    size_t sort_bytes = 0;
    FAL_CHECK_HIP(rocprim::merge_sort<CsvSortConfig>(nullptr, sort_bytes, (int32_t*)nullptr, order_out, (size_t)n, less, ctx->stream));
    ScratchLayout L;                                        // every part on a 256-byte step
    const auto meta = L.array<unsigned long long>(8);
    L.align(256);
    const auto iota = L.array<int32_t>(n);
    L.align(256);
    const auto sort_tmp = L.array<unsigned char>((int64_t)sort_bytes);
    FAL_TRY(L.reserve(ctx, SLOT_CSVW));
    FAL_CHECK_HIP(hipMemsetAsync(meta, 0, 64, ctx->stream));
    hipLaunchKernelGGL(csv_check_ids_kernel, dim3(capped_grid(ctx, n, 256)), dim3(256), 0, ctx->stream, id, id_ptr, id_bytes, n, iota, meta);
    FAL_CHECK_HIP(hipGetLastError());
    const unsigned long long* h = nullptr;
    FAL_TRY(read_meta(ctx, meta, &h));
    FAL_REQUIRE(!(h[META_FLAGS] & TW_BAD_INPUT), FAL_EINVAL, "fal_csv_order: id_ptr not ascending inside the id blob");
    *max_digit_run_out = (int64_t)h[META_DIGITS];
    FAL_CHECK_HIP(rocprim::merge_sort<CsvSortConfig>(sort_tmp, sort_bytes, iota.get(), order_out, (size_t)n, less, ctx->stream));
    return FAL_OK;
}

extern "C" int fal_csv_write_sizes(fal_ctx* ctx, const int32_t* order, int64_t rows, const int32_t* file_id, const uint8_t* fn,
                                   const int64_t* fn_ptr, int64_t n_files, int64_t fn_bytes, const uint8_t* id, const int64_t* id_ptr,
                                   int64_t id_bytes, const int32_t* charge, const float* precursor_mz, const float* retention_time,
                                   const int64_t* cluster, int64_t n, int quote_cr, int64_t* sizes_out, int64_t* offsets_out,
                                   int64_t* total_out) {
    fal::CallScope _call(ctx);
    FAL_TRY(check_columns("fal_csv_write_sizes", ctx, file_id, fn_ptr, n_files, fn_bytes, id_ptr, id_bytes, charge, precursor_mz,
                          retention_time, cluster, n, rows));
    FAL_REQUIRE(offsets_out && total_out && (rows == 0 || sizes_out) && (order || rows <= n), FAL_EINVAL,
                "fal_csv_write_sizes: NULL output, or more rows than the columns have and no order");
    *total_out = 0;
    if (rows == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(offsets_out, 0, sizeof(int64_t), ctx->stream));
        return FAL_OK;
    }
    unsigned long long* meta = nullptr;
    FAL_TRY(writer_meta(ctx, SLOT_CSVW, &meta));
    const CsvColumns c{order, file_id, fn, fn_ptr, n_files, fn_bytes, id, id_ptr, id_bytes, charge, precursor_mz, retention_time, cluster, n,
                       quote_cr != 0};
    hipLaunchKernelGGL(csv_write_sizes_kernel, dim3(capped_grid(ctx, rows, 256)), dim3(256), 0, ctx->stream, c, rows, sizes_out, meta);
    return finish_sizes(ctx, meta, sizes_out, rows, offsets_out, total_out,
                        "fal_csv_write_sizes: an order entry or a file id outside its range, or fn_ptr / id_ptr not ascending inside their blobs");
}

extern "C" int fal_csv_write(fal_ctx* ctx, const int32_t* order, int64_t rows, const int32_t* file_id, const uint8_t* fn, const int64_t* fn_ptr,
                             int64_t n_files, int64_t fn_bytes, const uint8_t* id, const int64_t* id_ptr, int64_t id_bytes,
                             const int32_t* charge, const float* precursor_mz, const float* retention_time, const int64_t* cluster, int64_t n,
                             int quote_cr, const int64_t* offsets, int64_t first, int64_t last, uint8_t* out, int64_t out_bytes,
                             uint8_t* host_out) {
    fal::CallScope _call(ctx);
    FAL_TRY(check_columns("fal_csv_write", ctx, file_id, fn_ptr, n_files, fn_bytes, id_ptr, id_bytes, charge, precursor_mz, retention_time,
                          cluster, n, rows));
    FAL_REQUIRE(offsets && first >= 0 && first <= last && last <= rows && out_bytes >= 0 && (out || out_bytes == 0) && (order || rows <= n) &&
                    (fn || fn_bytes == 0) && (id || id_bytes == 0),
                FAL_EINVAL, "fal_csv_write: bad argument");
    unsigned long long* meta = nullptr;
    FAL_TRY(writer_meta(ctx, SLOT_CSVW, &meta));
    const CsvColumns c{order, file_id, fn, fn_ptr, n_files, fn_bytes, id, id_ptr, id_bytes, charge, precursor_mz, retention_time, cluster, n,
                       quote_cr != 0};
    hipLaunchKernelGGL(csv_write_kernel, dim3(capped_grid(ctx, ceil_div(std::max<int64_t>(last - first, 1), (int64_t)64), 4)), dim3(256), 0,
                       ctx->stream, c, offsets, first, last, out, out_bytes, meta);
    return finish_write(ctx, meta, "fal_csv_write", "rows", "a row", first, last, out, out_bytes, host_out);
}
