// Network of the cluster representatives (fal_network_edges; DESIGN.md "Representative network"; netmatch.h holds the pure core,
// nettile.h the pair-tile core shared with libsearch.hip: the bodies of the tile and greedy-list kernels, the host side of a call).
//
// The nodes are ordered by (precursor m/z, node index) with fal_sort_by_precursor.  Tile row t holds sorted positions 64 t ..
// 64 t + 63; it is set against the 64-position chunks from its own (the diagonal) up to the chunk that holds the last position
// within max_shift of the row's last position -- a band of the tile triangle, counted per tile row on the device and scanned, so
// that one launch has one workgroup per (tile row, chunk).  Sorted order makes the first node of a pair netmatch.h's a.
//
// Edges are (u << 32 | v, sim bits << 32 | matched), sorted by their key.  Mutual top-k: both directions of every edge, sorted
// by (node, sim descending) with a stable sort that was given them in ascending order of the other node; an edge whose rank in
// either run is top_k or more is dropped, the rest compacted in order.
#include "nettile.h"

namespace fal {
namespace {

// chunks of tile row t: from its own to the one that holds the last position in scope of the row's last position (the scope
// test is monotone along the sorted precursors: a binary search with the test itself; the per-pair test still decides)
__global__ void net_band_kernel(const float* __restrict__ pmzs, int64_t n, int64_t n_tiles, double max_shift, int32_t* __restrict__ chunks) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tiles; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t last = std::min<int64_t>(t * kExTile + kExTile - 1, n - 1);
        const float pa = pmzs[last];
        int64_t lo = last + 1, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (net_in_scope(pa, pmzs[mid], max_shift)) lo = mid + 1; else hi = mid;
        }
        chunks[t] = (int32_t)((lo + kExTile - 1) / kExTile - t);      // (lo > 64 t: at least the diagonal chunk)
    }
}

// nettile.h's rule of the network: both sides are the nodes; sorted order makes a the first of a pair, the key is (min, max) node
struct NetRule {
    double tol, max_shift, min_cosine;
    int min_matched;
    static constexpr bool kDiagonal = true;
    __device__ void chunk(int64_t t, int64_t c, int64_t nb, int64_t* b0, int64_t* b1) const { *b0 = (t + c) * kExTile, *b1 = nb; }
    __device__ bool in_scope(float pa, float pb) const { return net_in_scope(pa, pb, max_shift); }
    __device__ NetOriented orient(const NetRow& a, const NetRow& b) const { return net_orient(a, b); }
    __device__ static uint64_t key(int32_t na, int32_t nb) { return ((uint64_t)(uint32_t)min(na, nb) << 32) | (uint32_t)max(na, nb); }
};

__global__ void net_prepare_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                   int64_t n_csr_rows, int64_t n, int32_t* __restrict__ node, int64_t* __restrict__ crow,
                                   int32_t* __restrict__ err) {
    net_prepare_body(order, rows, indptr, n_csr_rows, n, node, crow, err);
}

__global__ __launch_bounds__(kNetBlock) void net_tile_kernel(const int64_t* __restrict__ toff, int64_t n_tiles, NetSide sd, NetRule rule,
                                                             NetOut out, int2* __restrict__ small, int64_t small_cap,
                                                             int2* __restrict__ large, int64_t large_cap, int32_t* __restrict__ err) {
    net_tile_body(toff, n_tiles, sd, sd, rule, out, small, small_cap, large, large_cap, err);
}

template <int kCap>
__global__ __launch_bounds__(64) void net_greedy_kernel(const int2* __restrict__ list, const unsigned long long* __restrict__ n_list,
                                                        int64_t list_cap, NetOut out, NetSide sd, NetRule rule) {
    net_greedy_body<kCap>(list, n_list, list_cap, sd, sd, rule, out);
}

// both directions of the m sorted edges for the rank sort: first every edge at its higher node, then every edge at its lower
// node -- a node's entries then stand in ascending order of the other node (lower ones first), which the stable sort keeps
__global__ void net_rank_entries_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, int64_t m,
                                        uint64_t* __restrict__ rkey, uint64_t* __restrict__ redge, int32_t* __restrict__ drop) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[e];
        const float sim = __uint_as_float((uint32_t)(vals[e] >> 32));
        rkey[e] = net_rank_key((int32_t)(uint32_t)k, sim);
        rkey[m + e] = net_rank_key((int32_t)(k >> 32), sim);
        redge[e] = redge[m + e] = (uint64_t)e;
        drop[e] = 0;
    }
}

// an entry's rank in its node's run; rank >= top_k drops the edge (every writer stores the same 1)
__global__ void net_rank_mark_kernel(const uint64_t* __restrict__ rkey, const uint64_t* __restrict__ redge, int64_t m2, int top_k,
                                     int32_t* __restrict__ drop) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < m2; x += (int64_t)gridDim.x * blockDim.x)
        if (x - net_run_start(rkey, x) >= (int64_t)top_k) drop[redge[x]] = 1;
}

__global__ void net_keep_kernel(int32_t* __restrict__ drop, int64_t m) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) drop[e] = !drop[e];
}

// the kept edges into the caller's arrays: edge e to place[e] (place NULL: to e)
__global__ void net_output_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, int64_t m,
                                  const int32_t* __restrict__ keep, const int64_t* __restrict__ place, int32_t* __restrict__ edge_u,
                                  int32_t* __restrict__ edge_v, float* __restrict__ edge_sim, int32_t* __restrict__ edge_matched) {
    net_output_body<false>(keys, vals, nullptr, m, keep, place, edge_u, edge_v, edge_sim, edge_matched);
}

}  // namespace
}  // namespace fal
FAL_WARM_KERNEL(fal::net_tile_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_network_edges(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_csr_rows,
                                 const int32_t* rows, const float* precursor_mz, int64_t n, double fragment_tol, double max_shift,
                                 double min_cosine, int min_matched, int top_k, int32_t* edge_u, int32_t* edge_v, float* edge_sim,
                                 int32_t* edge_matched, int64_t max_edges, int64_t* n_edges) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_edges && n >= 0 && n < (int64_t)INT32_MAX && n_csr_rows >= 0 && fragment_tol >= 0.0 && max_shift >= 0.0 &&
                    min_cosine >= 0.0 && min_cosine <= 1.0 && min_matched >= 0 && top_k >= 0 && max_edges >= 0,
                FAL_EINVAL, "fal_network_edges: bad argument");
    *n_edges = 0;
    if (n == 0) return FAL_OK;
    FAL_REQUIRE(indptr && rows && precursor_mz, FAL_EINVAL, "fal_network_edges: NULL array");
    const NetCall call{"fal_network_edges", "inside max_shift", 12, SLOT_NET2, SLOT_NET3, SLOT_NET4, SLOT_NET6, SLOT_NET7};
    hipStream_t st = ctx->stream;
    ctx->counters[12] = 0;
    const int64_t n_tiles = ceil_div(n, kExTile);
    ScratchLayout L;
    const auto words = L.array<unsigned char>(64);          // the call's words (NetWords)
    const auto order = L.array<int64_t>(n), crow = L.array<int64_t>(n), toff = L.array<int64_t>(n_tiles + 1);
    const auto pmzs = L.array<float>(n);
    const auto node = L.array<int32_t>(n), chunks = L.array<int32_t>(n_tiles);
    L.pad(4);
    FAL_TRY(L.reserve(ctx, SLOT_NET));
    NetWords w(words);
    FAL_CHECK_HIP(hipMemsetAsync(words, 0, 64, st));
    FAL_TRY(fal_sort_by_precursor(ctx, precursor_mz, n, order, pmzs));
    const NetSide sd = net_side(ctx, net_prepare_kernel, mz, intensity, indptr, n_csr_rows, rows, n, order, crow, pmzs, node, fragment_tol,
                                min_matched, w.d_err);
    hipLaunchKernelGGL(net_band_kernel, dim3(capped_grid(ctx, n_tiles, kNetBlock)), dim3(kNetBlock), 0, st, pmzs, n, n_tiles, max_shift,
                       chunks);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, chunks, n_tiles, toff, SLOT_NET6));
    FAL_TRY(net_first_wait(ctx, toff + n_tiles, &w));
    FAL_REQUIRE(*w.h_err == 0, FAL_EINVAL, "fal_network_edges: a node's row lies outside the %lld rows of the peak CSR, or indptr falls",
                (long long)n_csr_rows);
    NetOut ed;
    int64_t m = 0;
    FAL_TRY(net_settle(ctx, call, w, toff, n_tiles, mz && intensity, net_tile_kernel, net_greedy_kernel<kNetSmall>,
                       net_greedy_kernel<kNetMaxPeaks>, &ed, &m, sd, NetRule{fragment_tol, max_shift, min_cosine, min_matched}));
    if (m == 0) return FAL_OK;
    // SLOT_NET4: the edges in (u, v) order, s.flag = drop
    NetSorted s;
    FAL_TRY(net_sort_records(ctx, call, ed, m, &s));
    const unsigned egrid = capped_grid(ctx, m, kNetBlock);
    int64_t kept = m;
    if (top_k > 0) {
        ScratchLayout L5;
        const auto rkey = L5.array<uint64_t>(4 * m), redge = L5.array<uint64_t>(4 * m);      // the sort's in and out, 2 m each
        FAL_TRY(L5.reserve(ctx, SLOT_NET5));
        hipLaunchKernelGGL(net_rank_entries_kernel, dim3(egrid), dim3(kNetBlock), 0, st, s.keys, s.vals, m, rkey, redge, s.flag);
        ctx->release(SLOT_NET7);                       // (the edge sort is enqueued: its block is retired, not freed, if this one grows)
        // (the edge numbers travel through the sort as the bit patterns of doubles)
        FAL_TRY(sort_pairs_u64_f64(ctx, rkey, rkey + 2 * m, reinterpret_cast<double*>(redge.get()), reinterpret_cast<double*>(redge + 2 * m), 2 * m,
                                   SLOT_NET7));
        hipLaunchKernelGGL(net_rank_mark_kernel, dim3(capped_grid(ctx, 2 * m, kNetBlock)), dim3(kNetBlock), 0, st, rkey + 2 * m,
                           redge + 2 * m, 2 * m, top_k, s.flag);
        hipLaunchKernelGGL(net_keep_kernel, dim3(egrid), dim3(kNetBlock), 0, st, s.flag, m);
        FAL_CHECK_HIP(hipGetLastError());
        FAL_TRY(net_count_kept(ctx, call, w, s, m, &kept));      // wait 5: the edges the ranks kept
    }
    *n_edges = kept;
    FAL_REQUIRE(kept <= max_edges, FAL_EINVAL, "fal_network_edges: %lld edges do not fit max_edges %lld", (long long)kept,
                (long long)max_edges);
    if (kept == 0) return FAL_OK;
    FAL_REQUIRE(edge_u && edge_v && edge_sim && edge_matched, FAL_EINVAL, "fal_network_edges: NULL edge array");
    hipLaunchKernelGGL(net_output_kernel, dim3(egrid), dim3(kNetBlock), 0, st, s.keys, s.vals, m, top_k > 0 ? s.flag : (const int32_t*)nullptr,
                       top_k > 0 ? s.place : (const int64_t*)nullptr, edge_u, edge_v, edge_sim, edge_matched);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
