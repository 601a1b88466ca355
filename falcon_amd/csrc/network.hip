// Network of the cluster representatives (fal_network_edges; DESIGN.md "Representative network"; netmatch.h holds the pure core).
//
// The nodes are ordered by (precursor m/z, node index) with fal_sort_by_precursor.  Tile row t holds sorted positions 64 t ..
// 64 t + 63; it is set against the 64-position chunks from its own (the diagonal) up to the chunk that holds the last position
// within max_shift of the row's last position -- a band of the tile triangle, counted per tile row on the device and scanned, so
// that one launch has one workgroup per (tile row, chunk).  A workgroup stages both sides' peak lists in LDS (exwalk.h's scheme
// and budget) and every lane takes one pair at a time: the scope test, then netmatch.h's window walk over a's peaks, and when
// that leaves enough peaks with a partner the walk over b's.  A pair below the matched-peak threshold on either side ends there;
// a conflict-free pair is summed in the walk; every other pair goes to one of two compacted lists (sides of up to 64 peaks, larger
// sides), which net_greedy_kernel finishes with one wave per pair.
//
// Edges are appended (one atomic per wave in the tile kernel, one per pair in the greedy kernel) as (u << 32 | v, sim bits << 32
// | matched) and sorted by their key (exact.hip's 64-bit pair sort): the order of arrival decides nothing.  Mutual top-k: both directions of every edge, sorted
// by (node, sim descending) with a stable sort that was given them in ascending order of the other node; an edge whose rank in
// either run is top_k or more is dropped, the rest compacted in order.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "exwalk.h"
#include "ivf.h"
#include "netgreedy.h"
#include "netmatch.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kNetBlock = 256;
constexpr int kNetSmall = 64;                          // sides of the greedy kernel's register-sized form: one strip of 64 peaks
constexpr int64_t kNetListBudget = 1ll << 22;          // listed pairs / edges held before the host has seen a count (32 MB / 64 MB)
static_assert(kNetMaxPeaks % 64 == 0 && kNetSmall == 64 && kNetMaxPeaks == FAL_NET_MAX_PEAKS, "strips of one wave");
constexpr int64_t kNetRowPeaks = 1ll << 24;           // peaks of any node's row: the staging adds up 64 rows' counts in 32 bits
enum { NET_ERR_ROW = 1, NET_ERR_PEAKS = 2 };          // bits of the error word
enum { NET_N_EDGES = 0, NET_N_SMALL = 1, NET_N_LARGE = 2 };   // the call's counts (unsigned long long each)

// sorted position p -> its node, its row of the peak CSR; a row outside the CSR or with a falling indptr sets the error word
// (and is given row 0 of nothing: no kernel behind this one runs then)
__global__ void net_prepare_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                   int64_t n_csr_rows, int64_t n, int32_t* __restrict__ node, int64_t* __restrict__ crow,
                                   int32_t* __restrict__ err) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = order[p];
        const int64_t r = rows[v];
        bool ok = r >= 0 && r < n_csr_rows;
        if (ok) ok = indptr[r + 1] >= indptr[r] && indptr[r + 1] - indptr[r] <= kNetRowPeaks;
        if (!ok) atomicOr(err, NET_ERR_ROW);
        node[p] = (int32_t)v;
        crow[p] = ok ? r : 0;
    }
}

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

struct NetParams {
    double tol, max_shift, min_cosine;
    int min_matched;
};

struct NetEdges {
    uint64_t* keys;
    uint64_t* vals;
    int64_t cap;
    unsigned long long* counts;              // NET_N_*
};

__device__ __forceinline__ void net_put_edge(const NetEdges& e, unsigned long long slot, int32_t na, int32_t nb, float sim, int matched) {
    if (slot >= (unsigned long long)e.cap) return;
    const uint32_t u = (uint32_t)min(na, nb), v = (uint32_t)max(na, nb);
    e.keys[slot] = ((uint64_t)u << 32) | v;
    e.vals[slot] = ((uint64_t)__float_as_uint(sim) << 32) | (uint32_t)matched;
}

__global__ __launch_bounds__(kNetBlock) void net_tile_kernel(const int64_t* __restrict__ toff, int64_t n_tiles, ExactPeaks pk,
                                                             const float* __restrict__ pmzs, const int32_t* __restrict__ node,
                                                             int64_t n, NetParams prm, NetEdges ed, int2* __restrict__ small,
                                                             int64_t small_cap, int2* __restrict__ large, int64_t large_cap,
                                                             int32_t* __restrict__ err) {
    __shared__ float s_mz[2][kExLdsPeaks];
    __shared__ float s_it[2][kExLdsPeaks];
    __shared__ int64_t s_off[2][64];
    __shared__ int s_len[2][128];
    __shared__ int s_tot[2];
    __shared__ float s_pmz[2][64];
    // the tile row of this workgroup: the last t with toff[t] <= blockIdx.x
    int64_t lo = 0, hi = n_tiles;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (toff[mid] <= (int64_t)blockIdx.x) lo = mid; else hi = mid;
    }
    const int64_t a0 = lo * kExTile, b0 = (lo + ((int64_t)blockIdx.x - toff[lo])) * kExTile;
    if (b0 >= n) return;                                             // (never: the band ends inside the nodes; workgroup-uniform)
    const int na_rows = (int)min((int64_t)kExTile, n - a0), nb_rows = (int)min((int64_t)kExTile, n - b0);
    const bool diag = a0 == b0;
    const int sb = diag ? 0 : 1;
    if (threadIdx.x < 64) {
        s_pmz[0][threadIdx.x] = (int)threadIdx.x < na_rows ? pmzs[a0 + threadIdx.x] : 0.f;
        s_pmz[1][threadIdx.x] = (int)threadIdx.x < nb_rows ? pmzs[b0 + threadIdx.x] : 0.f;
    }
    const bool fa = ex_stage(pk, (int32_t)a0, na_rows, s_mz[0], s_it[0], s_off[0], s_len[0], &s_tot[0]);
    bool fbb = fa;
    if (!diag) fbb = ex_stage(pk, (int32_t)b0, nb_rows, s_mz[1], s_it[1], s_off[1], s_len[1], &s_tot[1]);
    const int need = net_need(prm.min_matched);
    for (int p = threadIdx.x; p < kExTile * kExTile; p += kNetBlock) {   // (uniform trip count: every lane reaches the ballots)
        const int i = p >> 6, j = p & 63;
        bool hit = false, to_small = false, to_large = false;
        float sim = 0.f;
        int matched = 0;
        if (i < na_rows && j < nb_rows && (!diag || j > i)) {
            const float pa = s_pmz[0][i], pb = s_pmz[1][j];
            const int la = s_len[0][i], lb = s_len[sb][j];
            if (net_in_scope(pa, pb, prm.max_shift)) {
                if (la > kNetMaxPeaks || lb > kNetMaxPeaks) {
                    atomicOr(err, NET_ERR_PEAKS);
                } else if (la >= need && lb >= need) {
                    const float* amz = fa ? s_mz[0] + s_len[0][64 + i] : pk.mz + s_off[0][i];
                    const float* ait = fa ? s_it[0] + s_len[0][64 + i] : pk.it + s_off[0][i];
                    const float* bmz = fbb ? s_mz[sb] + s_len[sb][64 + j] : pk.mz + s_off[sb][j];
                    const float* bit = fbb ? s_it[sb] + s_len[sb][64 + j] : pk.it + s_off[sb][j];
                    const float shift = net_shift(pa, pb);
                    const NetWalk wa = net_walk<true>(amz, ait, la, bmz, bit, lb, shift, prm.tol);
                    if (wa.hit >= need) {
                        const NetWalk wb = net_walk<false>(bmz, bit, lb, amz, ait, la, shift, prm.tol);
                        const int kind = net_classify(wa.hit, wa.widest, wb.hit, wb.widest, need);
                        if (kind == NET_INLINE) {
                            sim = net_similarity(wa.score);
                            matched = wa.matched;
                            hit = net_is_edge(sim, matched, prm.min_cosine, prm.min_matched);
                        } else if (kind == NET_GREEDY) {
                            to_small = la <= kNetSmall && lb <= kNetSmall;
                            to_large = !to_small;
                        }
                    }
                }
            }
        }
        const unsigned long long e = ex_wave_slot(hit, ed.counts + NET_N_EDGES);
        if (hit) net_put_edge(ed, e, node[a0 + i], node[b0 + j], sim, matched);
        const unsigned long long fs = ex_wave_slot(to_small, ed.counts + NET_N_SMALL);
        if (to_small && fs < (unsigned long long)small_cap) small[fs] = make_int2((int)(a0 + i), (int)(b0 + j));
        const unsigned long long fl = ex_wave_slot(to_large, ed.counts + NET_N_LARGE);
        if (to_large && fl < (unsigned long long)large_cap) large[fl] = make_int2((int)(a0 + i), (int)(b0 + j));
    }
}

// One wave per listed pair (sorted positions a < b): netgreedy.h's rounds, then the edge rule in lane 0.
template <int kCap>
__global__ __launch_bounds__(64) void net_greedy_kernel(const int2* __restrict__ list, const unsigned long long* __restrict__ n_list,
                                                        int64_t list_cap, ExactPeaks pk, const float* __restrict__ pmzs,
                                                        const int32_t* __restrict__ node, NetParams prm, NetEdges ed) {
    __shared__ float s_w[kCap];
    __shared__ int s_j[kCap];
    __shared__ uint32_t s_used[kCap / 32];
    const int64_t cnt = min((int64_t)*n_list, list_cap);
    for (int64_t x = blockIdx.x; x < cnt; x += gridDim.x) {                   // (wave-uniform control flow)
        const int2 ab = list[x];
        const int64_t ra = pk.order[ab.x], rb = pk.order[ab.y];
        const int64_t ga = pk.indptr[ra], gb = pk.indptr[rb];
        const int la = (int)(pk.indptr[ra + 1] - ga), lb = (int)(pk.indptr[rb + 1] - gb);
        float sim = 0.f;
        int matched = 0;
        if (!net_greedy_pair<kCap>(pk.mz + ga, pk.it + ga, la, pk.mz + gb, pk.it + gb, lb, net_shift(pmzs[ab.x], pmzs[ab.y]), prm.tol,
                                   s_w, s_j, s_used, &sim, &matched))
            continue;                                                         // (never: the tile kernel lists by size)
        if (threadIdx.x == 0 && net_is_edge(sim, matched, prm.min_cosine, prm.min_matched))
            net_put_edge(ed, atomicAdd(ed.counts + NET_N_EDGES, 1ull), node[ab.x], node[ab.y], sim, matched);
        wave_lds_sync();                                                      // the next pair's state goes over this one's
    }
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
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < m2; x += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t nd = (uint32_t)(rkey[x] >> 32);
        int64_t lo = 0, hi = x;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((uint32_t)(rkey[mid] >> 32) < nd) lo = mid + 1; else hi = mid;
        }
        if (x - lo >= (int64_t)top_k) drop[redge[x]] = 1;
    }
}

__global__ void net_keep_kernel(int32_t* __restrict__ drop, int64_t m) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) drop[e] = !drop[e];
}

// the kept edges into the caller's arrays: edge e to place[e] (place NULL: to e)
__global__ void net_output_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, int64_t m,
                                  const int32_t* __restrict__ keep, const int64_t* __restrict__ place, int32_t* __restrict__ edge_u,
                                  int32_t* __restrict__ edge_v, float* __restrict__ edge_sim, int32_t* __restrict__ edge_matched) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        if (keep && !keep[e]) continue;
        const int64_t o = place ? place[e] : e;
        const uint64_t k = keys[e], v = vals[e];
        edge_u[o] = (int32_t)(k >> 32);
        edge_v[o] = (int32_t)(uint32_t)k;
        edge_sim[o] = __uint_as_float((uint32_t)(v >> 32));
        edge_matched[o] = (int32_t)(uint32_t)v;
    }
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
    hipStream_t st = ctx->stream;
    ctx->counters[12] = 0;
    const int64_t n_tiles = ceil_div(n, kExTile);
    // SLOT_NET: misc 64 B | order, crow i64[n] | toff i64[n_tiles + 1] | pmzs f32[n] | node i32[n] | chunks i32[n_tiles]
    unsigned char* blk = nullptr;
    FAL_TRY(ctx->reserve(SLOT_NET, 64 + 24 * (size_t)n + 12 * (size_t)(n_tiles + 1), (void**)&blk));
    int32_t* d_err = reinterpret_cast<int32_t*>(blk);
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(blk + 8);       // NET_N_*: 3 words
    int64_t* order = reinterpret_cast<int64_t*>(blk + 64);
    int64_t* crow = order + n;
    int64_t* toff = crow + n;
    float* pmzs = reinterpret_cast<float*>(toff + n_tiles + 1);
    int32_t* node = reinterpret_cast<int32_t*>(pmzs + n);
    int32_t* chunks = node + n;
    FAL_CHECK_HIP(hipMemsetAsync(blk, 0, 64, st));
    FAL_TRY(fal_sort_by_precursor(ctx, precursor_mz, n, order, pmzs));
    hipLaunchKernelGGL(net_prepare_kernel, dim3(capped_grid(ctx, n, kNetBlock)), dim3(kNetBlock), 0, st, order, rows, indptr, n_csr_rows,
                       n, node, crow, d_err);
    hipLaunchKernelGGL(net_band_kernel, dim3(capped_grid(ctx, n_tiles, kNetBlock)), dim3(kNetBlock), 0, st, pmzs, n, n_tiles, max_shift,
                       chunks);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, chunks, n_tiles, toff, SLOT_NET6));
    unsigned char* pin = nullptr;
    FAL_TRY(ctx->pinned_reserve(64, (void**)&pin));
    int64_t* h_total = reinterpret_cast<int64_t*>(pin);
    unsigned long long* h_counts = reinterpret_cast<unsigned long long*>(pin + 8);
    int32_t* h_err = reinterpret_cast<int32_t*>(pin + 32);
    // wait 1: the workgroups of the tile launch, and whether every node names a row of the CSR
    FAL_CHECK_HIP(hipMemcpyAsync(h_total, toff + n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipMemcpyAsync(h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipStreamSynchronize(st));
    FAL_REQUIRE(*h_err == 0, FAL_EINVAL, "fal_network_edges: a node's row lies outside the %lld rows of the peak CSR, or indptr falls",
                (long long)n_csr_rows);
    const int64_t wgs = *h_total;
    FAL_REQUIRE(wgs < (int64_t)INT32_MAX, FAL_EUNSUPPORTED, "fal_network_edges: %lld tiles inside max_shift are more than one launch holds",
                (long long)wgs);
    FAL_REQUIRE(mz && intensity, FAL_EINVAL, "fal_network_edges: NULL peak array");
    ExactPeaks pk;
    pk.mz = mz;
    pk.it = intensity;
    pk.indptr = indptr;
    pk.order = crow;
    pk.tol = fragment_tol;
    pk.min_matches = min_matched;
    pk.err = d_err;
    const NetParams prm{fragment_tol, max_shift, min_cosine, min_matched};
    // the tile and greedy launches: once, again when a list was too short (its count is exact: slots past the end are counted,
    // not written), and once more when the edges of the listed pairs, unknown until then, did not fit -- the same pairs give the
    // same edges every time
    const int64_t pairs_bound = std::min<int64_t>(wgs * kExTile * kExTile, kNetListBudget);
    int64_t small_cap = std::max<int64_t>(1, pairs_bound), large_cap = std::max<int64_t>(1, pairs_bound / 16),
            edge_cap = std::max<int64_t>(1, pairs_bound);
    NetEdges ed{nullptr, nullptr, 0, d_counts};
    int64_t m = 0;
    ctx->stage_reset(ST_KERNEL);
    ctx->stage_reset(ST_TAIL);
    for (int run = 0;; ++run) {
        FAL_REQUIRE(run < 3, FAL_EINTERNAL, "fal_network_edges: the lists did not settle");
        int2* lists = nullptr;
        FAL_TRY(ctx->reserve(SLOT_NET2, sizeof(int2) * (size_t)(small_cap + large_cap), (void**)&lists));
        FAL_TRY(ctx->reserve(SLOT_NET3, 2 * sizeof(uint64_t) * (size_t)edge_cap, (void**)&ed.keys));
        ed.vals = ed.keys + edge_cap;
        ed.cap = edge_cap;
        int2* small = lists;
        int2* large = lists + small_cap;
        FAL_CHECK_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), st));
        if (wgs > 0) {
            StageScope ts(ctx, ST_KERNEL);
            hipLaunchKernelGGL(net_tile_kernel, dim3((unsigned)wgs), dim3(kNetBlock), 0, st, toff, n_tiles, pk, pmzs, node, n, prm, ed,
                               small, small_cap, large, large_cap, d_err);
        }
        {
            StageScope ts(ctx, ST_TAIL);
            hipLaunchKernelGGL(net_greedy_kernel<kNetSmall>, dim3((unsigned)std::min<int64_t>(small_cap, (int64_t)ctx->num_cus * 64)),
                               dim3(64), 0, st, small, d_counts + NET_N_SMALL, small_cap, pk, pmzs, node, prm, ed);
            hipLaunchKernelGGL(net_greedy_kernel<kNetMaxPeaks>, dim3((unsigned)std::min<int64_t>(large_cap, (int64_t)ctx->num_cus * 4)),
                               dim3(64), 0, st, large, d_counts + NET_N_LARGE, large_cap, pk, pmzs, node, prm, ed);
        }
        FAL_CHECK_HIP(hipGetLastError());
        // waits 2 to 4: the counts and the error word
        FAL_CHECK_HIP(hipMemcpyAsync(h_counts, d_counts, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipMemcpyAsync(h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        FAL_REQUIRE(*h_err == 0, FAL_EUNSUPPORTED, "fal_network_edges: a pair inside max_shift has a spectrum of more than %d peaks",
                    kNetMaxPeaks);
        const int64_t ns = (int64_t)h_counts[NET_N_SMALL], nl = (int64_t)h_counts[NET_N_LARGE];
        m = (int64_t)h_counts[NET_N_EDGES];
        ctx->counters[12] = ns + nl;
        if (ns <= small_cap && nl <= large_cap && m <= edge_cap) break;
        small_cap = std::max(small_cap, ns);
        large_cap = std::max(large_cap, nl);
        edge_cap = std::max(edge_cap, m);
        ctx->release(SLOT_NET2);
        ctx->release(SLOT_NET3);
    }
    if (m == 0) return FAL_OK;
    // deterministic order: (u, v) keys are unique, a radix sort puts them in place.
    // SLOT_NET4: keys, vals u64[m] | place i64[m + 1] | drop i32[m];  SLOT_NET5: rkey in / out u64[2 m] | redge in / out u64[2 m]
    unsigned char* sb = nullptr;
    FAL_TRY(ctx->reserve(SLOT_NET4, 28 * (size_t)m + 64, (void**)&sb));
    uint64_t* kout = reinterpret_cast<uint64_t*>(sb);
    uint64_t* vout = kout + m;
    int64_t* place = reinterpret_cast<int64_t*>(vout + m);
    int32_t* drop = reinterpret_cast<int32_t*>(place + m + 1);
    uint64_t* rkey = nullptr;
    uint64_t* redge = nullptr;
    // (the sorts are exact.hip's: the 8-byte values and edge numbers travel as the bit patterns of doubles)
    FAL_TRY(sort_pairs_u64_f64(ctx, ed.keys, kout, reinterpret_cast<double*>(ed.vals), reinterpret_cast<double*>(vout), m, SLOT_NET7));
    if (top_k > 0) {
        FAL_TRY(ctx->reserve(SLOT_NET5, 64 * (size_t)m, (void**)&rkey));
        redge = rkey + 4 * m;
    }
    const unsigned egrid = capped_grid(ctx, m, kNetBlock);
    int64_t kept = m;
    if (top_k > 0) {
        hipLaunchKernelGGL(net_rank_entries_kernel, dim3(egrid), dim3(kNetBlock), 0, st, kout, vout, m, rkey, redge, drop);
        ctx->release(SLOT_NET7);                       // (the edge sort is enqueued: its block is retired, not freed, if this one grows)
        FAL_TRY(sort_pairs_u64_f64(ctx, rkey, rkey + 2 * m, reinterpret_cast<double*>(redge), reinterpret_cast<double*>(redge + 2 * m), 2 * m,
                                   SLOT_NET7));
        hipLaunchKernelGGL(net_rank_mark_kernel, dim3(capped_grid(ctx, 2 * m, kNetBlock)), dim3(kNetBlock), 0, st, rkey + 2 * m,
                           redge + 2 * m, 2 * m, top_k, drop);
        hipLaunchKernelGGL(net_keep_kernel, dim3(egrid), dim3(kNetBlock), 0, st, drop, m);
        FAL_CHECK_HIP(hipGetLastError());
        ctx->release(SLOT_NET6);
        FAL_TRY(device_scan_i32(ctx, drop, m, place, SLOT_NET6));
        // wait 5: the edges the ranks kept
        FAL_CHECK_HIP(hipMemcpyAsync(h_total, place + m, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        kept = *h_total;
    }
    *n_edges = kept;
    FAL_REQUIRE(kept <= max_edges, FAL_EINVAL, "fal_network_edges: %lld edges do not fit max_edges %lld", (long long)kept,
                (long long)max_edges);
    if (kept == 0) return FAL_OK;
    FAL_REQUIRE(edge_u && edge_v && edge_sim && edge_matched, FAL_EINVAL, "fal_network_edges: NULL edge array");
    hipLaunchKernelGGL(net_output_kernel, dim3(egrid), dim3(kNetBlock), 0, st, kout, vout, m, top_k > 0 ? drop : (const int32_t*)nullptr,
                       top_k > 0 ? place : (const int64_t*)nullptr, edge_u, edge_v, edge_sim, edge_matched);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
