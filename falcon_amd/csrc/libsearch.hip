// Library search of the cluster representatives (fal_library_search; DESIGN.md "Library search"; libsearch.h and netmatch.h hold
// the pure core, nettile.h the pair-tile core shared with network.hip: the bodies of the tile and greedy-list kernels, the host
// side of a call).
//
// Both sides are ordered by (precursor m/z, index) with fal_sort_by_precursor.  Query tile t holds sorted query positions 64 t ..
// 64 t + 63; it is set against the 64-position chunks of the range of sorted library positions that can hold a pair in scope of
// its first to last query (binary search on libsearch.h's window: a range, not a triangle -- the library lies on both sides of
// a query), counted per tile on the device and scanned, so that one launch has one workgroup per (query tile, library chunk).
// The orientation of a pair (netmatch.h's a is the side with the lower precursor) is libsearch.h's swap of the two sides.
//
// Hits are (query << 32 | library, sim bits << 32 | matched), sorted by their key.  A second, stable pass of the same sort by
// (query, sim descending) leaves a query's hits in rank order, equal similarities in ascending order of the library index; a
// hit's rank is its distance from the first entry of its query's run.
#include "libsearch.h"
#include "nettile.h"

namespace fal {
namespace {

// nettile.h's rule of the search: side A the queries, side B the library; tile t's chunks start at first[t] and end at end[t];
// libsearch.h turns a pair so that a is the side with the lower precursor; the key is (query, library)
struct LibRule {
    double tol, precursor_tol, max_shift, min_cosine;
    int tol_is_da, analog, min_matched;
    const int32_t *first, *end;
    static constexpr bool kDiagonal = false;
    __device__ void chunk(int64_t t, int64_t c, int64_t, int64_t* b0, int64_t* b1) const { *b0 = first[t] + c * kExTile, *b1 = end[t]; }
    __device__ bool in_scope(float pq, float pl) const { return lib_in_scope(pq, pl, analog, precursor_tol, tol_is_da, max_shift); }
    __device__ NetOriented orient(const NetRow& q, const NetRow& l) const { return lib_orient(analog, q, l); }
    __device__ static uint64_t key(int32_t query, int32_t library) { return ((uint64_t)(uint32_t)query << 32) | (uint32_t)library; }
};

// first position of the sorted precursors with (double)mz >= x (strict = false) or > x (strict = true)
__device__ __forceinline__ int64_t lib_lower(const float* __restrict__ mz, int64_t n, double x, bool strict) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const double v = (double)mz[mid];
        if (strict ? v <= x : v < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the library range [first, end) of query tile t (a superset of the pairs in scope of its queries) and its 64-row chunks
__global__ void lib_band_kernel(const float* __restrict__ q_pmzs, int64_t nq, int64_t n_tiles, const float* __restrict__ l_pmzs,
                                int64_t nl, LibRule rule, int32_t* __restrict__ first, int32_t* __restrict__ end,
                                int32_t* __restrict__ chunks) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tiles; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t last = std::min<int64_t>(t * kExTile + kExTile - 1, nq - 1);
        double lo = 0.0, hi = 0.0;
        int64_t a = 0, b = nl;
        if (lib_window(q_pmzs[t * kExTile], q_pmzs[last], rule.analog, rule.precursor_tol, rule.tol_is_da, rule.max_shift, &lo, &hi)) {
            a = lib_lower(l_pmzs, nl, lo, false);
            b = std::max<int64_t>(a, lib_lower(l_pmzs, nl, hi, true));
        }
        first[t] = (int32_t)a;
        end[t] = (int32_t)b;
        chunks[t] = (int32_t)((b - a + kExTile - 1) / kExTile);
    }
}

__global__ void lib_prepare_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                   int64_t n_csr_rows, int64_t n, int32_t* __restrict__ node, int64_t* __restrict__ crow,
                                   int32_t* __restrict__ err) {
    net_prepare_body(order, rows, indptr, n_csr_rows, n, node, crow, err);
}

__global__ __launch_bounds__(kNetBlock) void lib_tile_kernel(const int64_t* __restrict__ toff, int64_t n_tiles, NetSide q, NetSide l,
                                                             LibRule rule, NetOut out, int2* __restrict__ small, int64_t small_cap,
                                                             int2* __restrict__ large, int64_t large_cap, int32_t* __restrict__ err) {
    net_tile_body(toff, n_tiles, q, l, rule, out, small, small_cap, large, large_cap, err);
}

template <int kCap>
__global__ __launch_bounds__(64) void lib_greedy_kernel(const int2* __restrict__ list, const unsigned long long* __restrict__ n_list,
                                                        int64_t list_cap, NetOut out, NetSide q, NetSide l, LibRule rule) {
    net_greedy_body<kCap>(list, n_list, list_cap, q, l, rule, out);
}

// the m hits in (query, library) order -> the entries of the rank sort: key (query, sim descending), value the hit's number
__global__ void lib_rank_entries_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, int64_t m,
                                        uint64_t* __restrict__ rkey, uint64_t* __restrict__ rhit) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        rkey[e] = net_rank_key((int32_t)(keys[e] >> 32), __uint_as_float((uint32_t)(vals[e] >> 32)));
        rhit[e] = (uint64_t)e;
    }
}

// an entry's rank in its query's run; keep[x] = 1 when it is below top_n
__global__ void lib_rank_mark_kernel(const uint64_t* __restrict__ rkey, int64_t m, int top_n, int32_t* __restrict__ keep) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < m; x += (int64_t)gridDim.x * blockDim.x)
        keep[x] = x - net_run_start(rkey, x) < (int64_t)top_n;
}

// the kept entries into the caller's arrays: entry x (rank order) to place[x] (place NULL: to x)
__global__ void lib_output_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ rhit,
                                  int64_t m, const int32_t* __restrict__ keep, const int64_t* __restrict__ place,
                                  int32_t* __restrict__ hit_query, int32_t* __restrict__ hit_library, float* __restrict__ hit_sim,
                                  int32_t* __restrict__ hit_matched) {
    net_output_body<true>(keys, vals, rhit, m, keep, place, hit_query, hit_library, hit_sim, hit_matched);
}

}  // namespace
}  // namespace fal
FAL_WARM_KERNEL(fal::lib_tile_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_library_search(fal_ctx* ctx, const float* q_mz, const float* q_intensity, const int64_t* q_indptr,
                                  int64_t q_csr_rows, const int32_t* q_rows, const float* q_precursor_mz, int64_t nq,
                                  const float* l_mz, const float* l_intensity, const int64_t* l_indptr, int64_t l_csr_rows,
                                  const int32_t* l_rows, const float* l_precursor_mz, int64_t nl, double fragment_tol,
                                  double precursor_tol, int tol_is_da, int analog, double max_shift, double min_cosine,
                                  int min_matched, int top_n, int32_t* hit_query, int32_t* hit_library, float* hit_sim,
                                  int32_t* hit_matched, int64_t max_hits, int64_t* n_hits) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_hits && nq >= 0 && nq < (int64_t)INT32_MAX && nl >= 0 && nl < (int64_t)INT32_MAX && q_csr_rows >= 0 &&
                    l_csr_rows >= 0 && fragment_tol >= 0.0 && precursor_tol >= 0.0 && max_shift >= 0.0 && min_cosine >= 0.0 &&
                    min_cosine <= 1.0 && min_matched >= 0 && top_n >= 0 && max_hits >= 0,
                FAL_EINVAL, "fal_library_search: bad argument");
    *n_hits = 0;
    ctx->counters[14] = 0;
    if (nq == 0 || nl == 0) return FAL_OK;
    FAL_REQUIRE(q_indptr && q_rows && q_precursor_mz && l_indptr && l_rows && l_precursor_mz, FAL_EINVAL,
                "fal_library_search: NULL array");
    const NetCall call{"fal_library_search", "in scope", 14, SLOT_LIB2, SLOT_LIB3, SLOT_LIB4, SLOT_LIB6, SLOT_LIB7};
    hipStream_t st = ctx->stream;
    const int64_t n_tiles = ceil_div(nq, kExTile);
    ScratchLayout L;
    const auto words = L.array<unsigned char>(64);          // the call's words (NetWords)
    const auto q_order = L.array<int64_t>(nq), q_crow = L.array<int64_t>(nq), l_order = L.array<int64_t>(nl), l_crow = L.array<int64_t>(nl);
    const auto toff = L.array<int64_t>(n_tiles + 1);
    const auto q_pmzs = L.array<float>(nq), l_pmzs = L.array<float>(nl);
    const auto q_node = L.array<int32_t>(nq), l_node = L.array<int32_t>(nl);
    const auto chunks = L.array<int32_t>(n_tiles), first = L.array<int32_t>(n_tiles), end = L.array<int32_t>(n_tiles);
    L.pad(12);
    FAL_TRY(L.reserve(ctx, SLOT_LIB));
    NetWords w(words);
    FAL_CHECK_HIP(hipMemsetAsync(words, 0, 64, st));
    FAL_TRY(fal_sort_by_precursor(ctx, q_precursor_mz, nq, q_order, q_pmzs));
    ctx->release(SLOT_SORT);                                     // (the second sort may grow them: the first one's work is enqueued)
    ctx->release(SLOT_SORT2);
    FAL_TRY(fal_sort_by_precursor(ctx, l_precursor_mz, nl, l_order, l_pmzs));
    const LibRule rule{fragment_tol, precursor_tol, max_shift, min_cosine, tol_is_da != 0, analog != 0, min_matched, first, end};
    const NetSide q = net_side(ctx, lib_prepare_kernel, q_mz, q_intensity, q_indptr, q_csr_rows, q_rows, nq, q_order, q_crow, q_pmzs,
                               q_node, fragment_tol, min_matched, w.d_err);
    const NetSide l = net_side(ctx, lib_prepare_kernel, l_mz, l_intensity, l_indptr, l_csr_rows, l_rows, nl, l_order, l_crow, l_pmzs,
                               l_node, fragment_tol, min_matched, w.d_err);
    hipLaunchKernelGGL(lib_band_kernel, dim3(capped_grid(ctx, n_tiles, kNetBlock)), dim3(kNetBlock), 0, st, q_pmzs, nq, n_tiles, l_pmzs,
                       nl, rule, first, end, chunks);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, chunks, n_tiles, toff, SLOT_LIB6));
    FAL_TRY(net_first_wait(ctx, toff + n_tiles, &w));
    FAL_REQUIRE(*w.h_err == 0, FAL_EINVAL,
                "fal_library_search: a row lies outside the %lld (queries) / %lld (library) rows of its peak CSR, or indptr falls",
                (long long)q_csr_rows, (long long)l_csr_rows);
    NetOut ht;
    int64_t m = 0;
    FAL_TRY(net_settle(ctx, call, w, toff, n_tiles, q_mz && q_intensity && l_mz && l_intensity, lib_tile_kernel,
                       lib_greedy_kernel<kNetSmall>, lib_greedy_kernel<kNetMaxPeaks>, &ht, &m, q, l, rule));
    if (m == 0) return FAL_OK;
    // SLOT_LIB4: the hits in (query, library) order, s.flag = keep; the second, stable pass by (query, sim descending) keeps equal
    // similarities in that order.
    NetSorted s;
    ScratchLayout L5;
    const auto rkey = L5.array<uint64_t>(2 * m), rhit = L5.array<uint64_t>(2 * m);           // the sort's in and out, m each
    FAL_TRY(L5.reserve(ctx, SLOT_LIB5));
    FAL_TRY(net_sort_records(ctx, call, ht, m, &s));
    const unsigned hgrid = capped_grid(ctx, m, kNetBlock);
    hipLaunchKernelGGL(lib_rank_entries_kernel, dim3(hgrid), dim3(kNetBlock), 0, st, s.keys, s.vals, m, rkey, rhit);
    ctx->release(SLOT_LIB7);                           // (the hit sort is enqueued: its block is retired, not freed, if this one grows)
    // (the hit numbers travel through the sort as the bit patterns of doubles)
    FAL_TRY(sort_pairs_u64_f64(ctx, rkey, rkey + m, reinterpret_cast<double*>(rhit.get()), reinterpret_cast<double*>(rhit + m), m, SLOT_LIB7));
    int64_t kept = m;
    if (top_n > 0) {
        hipLaunchKernelGGL(lib_rank_mark_kernel, dim3(hgrid), dim3(kNetBlock), 0, st, rkey + m, m, top_n, s.flag);
        FAL_CHECK_HIP(hipGetLastError());
        FAL_TRY(net_count_kept(ctx, call, w, s, m, &kept));      // wait 5: the hits the ranks kept
    }
    *n_hits = kept;
    FAL_REQUIRE(kept <= max_hits, FAL_EINVAL, "fal_library_search: %lld hits do not fit max_hits %lld", (long long)kept,
                (long long)max_hits);
    if (kept == 0) return FAL_OK;
    FAL_REQUIRE(hit_query && hit_library && hit_sim && hit_matched, FAL_EINVAL, "fal_library_search: NULL hit array");
    hipLaunchKernelGGL(lib_output_kernel, dim3(hgrid), dim3(kNetBlock), 0, st, s.keys, s.vals, rhit + m, m,
                       top_n > 0 ? s.flag : (const int32_t*)nullptr, top_n > 0 ? s.place : (const int64_t*)nullptr, hit_query, hit_library,
                       hit_sim, hit_matched);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
