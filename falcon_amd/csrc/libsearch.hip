// Library search of the cluster representatives (fal_library_search; DESIGN.md "Library search"; libsearch.h and netmatch.h hold
// the pure core).
//
// Both sides are ordered by (precursor m/z, index) with fal_sort_by_precursor.  Query tile t holds sorted query positions 64 t ..
// 64 t + 63; it is set against the 64-position chunks of the range of sorted library positions that can hold a pair in scope of
// its first to last query (binary search on libsearch.h's window: a range, not a triangle -- the library lies on both sides of
// a query), counted per tile on the device and scanned, so that one launch has one workgroup per (query tile, library chunk).
// A workgroup stages both sides' peak lists in LDS (exwalk.h's scheme and budget) and every lane takes one pair at a time: the
// scope test, the peak limit, the orientation (netmatch.h's a is the side with the lower precursor: a swap of pointers), then
// the window walk over a's peaks and, when that leaves enough peaks with a partner, over b's.  A pair below the matched-peak
// threshold on either side ends there; a conflict-free pair is summed in the walk; every other pair goes to one of two compacted
// lists (sides of up to 64 peaks, larger sides), which lib_greedy_kernel finishes with one wave per pair (netgreedy.h's rounds,
// the ones of the network).
//
// Hits are appended (one atomic per wave in the tile kernel, one per pair in the greedy kernel) as (query << 32 | library, sim
// bits << 32 | matched) and sorted by their key (exact.hip's 64-bit pair sort): the order of arrival decides nothing.  A second,
// stable pass of the same sort by (query, sim descending) leaves a query's hits in rank order, equal similarities in ascending
// order of the library index; a hit's rank is its distance from the first entry of its query's run.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "exwalk.h"
#include "ivf.h"
#include "libsearch.h"
#include "netgreedy.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kLibBlock = 256;
constexpr int kLibSmall = 64;                          // sides of the greedy kernel's register-sized form: one strip of 64 peaks
constexpr int64_t kLibListBudget = 1ll << 22;          // listed pairs / hits held before the host has seen a count (32 MB / 64 MB)
static_assert(kNetMaxPeaks % 64 == 0 && kNetMaxPeaks == FAL_NET_MAX_PEAKS, "strips of one wave");
constexpr int64_t kLibRowPeaks = 1ll << 24;           // peaks of any row: the staging adds up 64 rows' counts in 32 bits
enum { LIB_ERR_ROW = 1, LIB_ERR_PEAKS = 2 };          // bits of the error word
enum { LIB_N_HITS = 0, LIB_N_SMALL = 1, LIB_N_LARGE = 2 };   // the call's counts (unsigned long long each)

// one side: sorted position p -> its index, its row of the side's peak CSR; a row outside the CSR or with a falling indptr sets
// the error word (and is given row 0 of nothing: no kernel behind this one runs then)
__global__ void lib_prepare_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                   int64_t n_csr_rows, int64_t n, int32_t* __restrict__ node, int64_t* __restrict__ crow,
                                   int32_t* __restrict__ err) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = order[p];
        const int64_t r = rows[v];
        bool ok = r >= 0 && r < n_csr_rows;
        if (ok) ok = indptr[r + 1] >= indptr[r] && indptr[r + 1] - indptr[r] <= kLibRowPeaks;
        if (!ok) atomicOr(err, LIB_ERR_ROW);
        node[p] = (int32_t)v;
        crow[p] = ok ? r : 0;
    }
}

struct LibRule {
    double tol, precursor_tol, max_shift, min_cosine;
    int tol_is_da, analog, min_matched;
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

struct LibSide {
    ExactPeaks pk;              // the side's peak CSR + order (sorted position -> row of the CSR)
    const float* pmzs;          // precursor m/z by sorted position
    const int32_t* node;        // the side's index by sorted position
    int64_t n;
};

struct LibHits {
    uint64_t* keys;
    uint64_t* vals;
    int64_t cap;
    unsigned long long* counts;              // LIB_N_*
};

__device__ __forceinline__ void lib_put_hit(const LibHits& h, unsigned long long slot, int32_t query, int32_t library, float sim,
                                            int matched) {
    if (slot >= (unsigned long long)h.cap) return;
    h.keys[slot] = ((uint64_t)(uint32_t)query << 32) | (uint32_t)library;
    h.vals[slot] = ((uint64_t)__float_as_uint(sim) << 32) | (uint32_t)matched;
}

__global__ __launch_bounds__(kLibBlock) void lib_tile_kernel(const int64_t* __restrict__ toff, int64_t n_tiles,
                                                             const int32_t* __restrict__ first, const int32_t* __restrict__ end,
                                                             LibSide q, LibSide l, LibRule rule, LibHits ht, int2* __restrict__ small,
                                                             int64_t small_cap, int2* __restrict__ large, int64_t large_cap,
                                                             int32_t* __restrict__ err) {
    __shared__ float s_mz[2][kExLdsPeaks];
    __shared__ float s_it[2][kExLdsPeaks];
    __shared__ int64_t s_off[2][64];
    __shared__ int s_len[2][128];
    __shared__ int s_tot[2];
    __shared__ float s_pmz[2][64];
    // the query tile of this workgroup: the last t with toff[t] <= blockIdx.x
    int64_t lo = 0, hi = n_tiles;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (toff[mid] <= (int64_t)blockIdx.x) lo = mid; else hi = mid;
    }
    const int64_t q0 = lo * kExTile, l0 = (int64_t)first[lo] + ((int64_t)blockIdx.x - toff[lo]) * kExTile, l1 = end[lo];
    if (q0 >= q.n || l0 >= l1 || l1 > l.n) return;                   // (never: the chunks end inside the range; workgroup-uniform)
    const int nq_rows = (int)min((int64_t)kExTile, q.n - q0), nl_rows = (int)min((int64_t)kExTile, l1 - l0);
    if (threadIdx.x < 64) {
        s_pmz[0][threadIdx.x] = (int)threadIdx.x < nq_rows ? q.pmzs[q0 + threadIdx.x] : 0.f;
        s_pmz[1][threadIdx.x] = (int)threadIdx.x < nl_rows ? l.pmzs[l0 + threadIdx.x] : 0.f;
    }
    const bool fq = ex_stage(q.pk, (int32_t)q0, nq_rows, s_mz[0], s_it[0], s_off[0], s_len[0], &s_tot[0]);
    const bool fl = ex_stage(l.pk, (int32_t)l0, nl_rows, s_mz[1], s_it[1], s_off[1], s_len[1], &s_tot[1]);
    const int need = net_need(rule.min_matched);
    for (int p = threadIdx.x; p < kExTile * kExTile; p += kLibBlock) {   // (uniform trip count: every lane reaches the ballots)
        const int i = p >> 6, j = p & 63;
        bool hit = false, to_small = false, to_large = false;
        float sim = 0.f;
        int matched = 0;
        if (i < nq_rows && j < nl_rows) {
            const float pq = s_pmz[0][i], pl = s_pmz[1][j];
            const int lq = s_len[0][i], ll = s_len[1][j];
            if (lib_in_scope(pq, pl, rule.analog, rule.precursor_tol, rule.tol_is_da, rule.max_shift)) {
                if (lq > kNetMaxPeaks || ll > kNetMaxPeaks) {
                    atomicOr(err, LIB_ERR_PEAKS);
                } else if (lq >= need && ll >= need) {
                    const float* qmz = fq ? s_mz[0] + s_len[0][64 + i] : q.pk.mz + s_off[0][i];
                    const float* qit = fq ? s_it[0] + s_len[0][64 + i] : q.pk.it + s_off[0][i];
                    const float* lmz = fl ? s_mz[1] + s_len[1][64 + j] : l.pk.mz + s_off[1][j];
                    const float* lit = fl ? s_it[1] + s_len[1][64 + j] : l.pk.it + s_off[1][j];
                    const bool qa = lib_query_is_a(pq, pl);                  // the orientation: a swap of pointers
                    const float* amz = qa ? qmz : lmz;
                    const float* ait = qa ? qit : lit;
                    const float* bmz = qa ? lmz : qmz;
                    const float* bit = qa ? lit : qit;
                    const int la = qa ? lq : ll, lb = qa ? ll : lq;
                    const float shift = lib_shift(rule.analog, qa ? pq : pl, qa ? pl : pq);
                    const NetWalk wa = net_walk<true>(amz, ait, la, bmz, bit, lb, shift, rule.tol);
                    if (wa.hit >= need) {
                        const NetWalk wb = net_walk<false>(bmz, bit, lb, amz, ait, la, shift, rule.tol);
                        const int kind = net_classify(wa.hit, wa.widest, wb.hit, wb.widest, need);
                        if (kind == NET_INLINE) {
                            sim = net_similarity(wa.score);
                            matched = wa.matched;
                            hit = net_is_edge(sim, matched, rule.min_cosine, rule.min_matched);
                        } else if (kind == NET_GREEDY) {
                            to_small = la <= kLibSmall && lb <= kLibSmall;
                            to_large = !to_small;
                        }
                    }
                }
            }
        }
        const unsigned long long e = ex_wave_slot(hit, ht.counts + LIB_N_HITS);
        if (hit) lib_put_hit(ht, e, q.node[q0 + i], l.node[l0 + j], sim, matched);
        const unsigned long long fs = ex_wave_slot(to_small, ht.counts + LIB_N_SMALL);
        if (to_small && fs < (unsigned long long)small_cap) small[fs] = make_int2((int)(q0 + i), (int)(l0 + j));
        const unsigned long long fg = ex_wave_slot(to_large, ht.counts + LIB_N_LARGE);
        if (to_large && fg < (unsigned long long)large_cap) large[fg] = make_int2((int)(q0 + i), (int)(l0 + j));
    }
}

// One wave per listed pair (sorted query position, sorted library position): the two sides' peaks in the pair's orientation
// through netgreedy.h's rounds, then the hit rule in lane 0.
template <int kCap>
__global__ __launch_bounds__(64) void lib_greedy_kernel(const int2* __restrict__ list, const unsigned long long* __restrict__ n_list,
                                                        int64_t list_cap, LibSide q, LibSide l, LibRule rule, LibHits ht) {
    __shared__ float s_w[kCap];
    __shared__ int s_j[kCap];
    __shared__ uint32_t s_used[kCap / 32];
    const int64_t cnt = min((int64_t)*n_list, list_cap);
    for (int64_t x = blockIdx.x; x < cnt; x += gridDim.x) {                   // (wave-uniform control flow)
        const int2 ql = list[x];
        const int64_t rq = q.pk.order[ql.x], rl = l.pk.order[ql.y];
        const int64_t gq = q.pk.indptr[rq], gl = l.pk.indptr[rl];
        const int lq = (int)(q.pk.indptr[rq + 1] - gq), ll = (int)(l.pk.indptr[rl + 1] - gl);
        const float pq = q.pmzs[ql.x], pl = l.pmzs[ql.y];
        const bool qa = lib_query_is_a(pq, pl);
        const float* amz = qa ? q.pk.mz + gq : l.pk.mz + gl;
        const float* ait = qa ? q.pk.it + gq : l.pk.it + gl;
        const float* bmz = qa ? l.pk.mz + gl : q.pk.mz + gq;
        const float* bit = qa ? l.pk.it + gl : q.pk.it + gq;
        float sim = 0.f;
        int matched = 0;
        if (!net_greedy_pair<kCap>(amz, ait, qa ? lq : ll, bmz, bit, qa ? ll : lq, lib_shift(rule.analog, qa ? pq : pl, qa ? pl : pq),
                                   rule.tol, s_w, s_j, s_used, &sim, &matched))
            continue;                                                         // (never: the tile kernel lists by size)
        if (threadIdx.x == 0 && net_is_edge(sim, matched, rule.min_cosine, rule.min_matched))
            lib_put_hit(ht, atomicAdd(ht.counts + LIB_N_HITS, 1ull), q.node[ql.x], l.node[ql.y], sim, matched);
        wave_lds_sync();                                                      // the next pair's state goes over this one's
    }
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
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < m; x += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t nd = (uint32_t)(rkey[x] >> 32);
        int64_t lo = 0, hi = x;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((uint32_t)(rkey[mid] >> 32) < nd) lo = mid + 1; else hi = mid;
        }
        keep[x] = x - lo < (int64_t)top_n;
    }
}

// the kept entries into the caller's arrays: entry x (rank order) to place[x] (place NULL: to x)
__global__ void lib_output_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ rhit,
                                  int64_t m, const int32_t* __restrict__ keep, const int64_t* __restrict__ place,
                                  int32_t* __restrict__ hit_query, int32_t* __restrict__ hit_library, float* __restrict__ hit_sim,
                                  int32_t* __restrict__ hit_matched) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < m; x += (int64_t)gridDim.x * blockDim.x) {
        if (keep && !keep[x]) continue;
        const int64_t o = place ? place[x] : x;
        const uint64_t e = rhit[x];
        const uint64_t k = keys[e], v = vals[e];
        hit_query[o] = (int32_t)(k >> 32);
        hit_library[o] = (int32_t)(uint32_t)k;
        hit_sim[o] = __uint_as_float((uint32_t)(v >> 32));
        hit_matched[o] = (int32_t)(uint32_t)v;
    }
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
    hipStream_t st = ctx->stream;
    const int64_t n_tiles = ceil_div(nq, kExTile);
    // SLOT_LIB: misc 64 B | q_order, q_crow i64[nq] | l_order, l_crow i64[nl] | toff i64[n_tiles + 1] | q_pmzs f32[nq] | l_pmzs
    // f32[nl] | q_node i32[nq] | l_node i32[nl] | chunks, first, end i32[n_tiles]
    unsigned char* blk = nullptr;
    FAL_TRY(ctx->reserve(SLOT_LIB, 64 + 24 * (size_t)(nq + nl) + 20 * (size_t)(n_tiles + 1), (void**)&blk));
    int32_t* d_err = reinterpret_cast<int32_t*>(blk);
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(blk + 8);       // LIB_N_*: 3 words
    int64_t* q_order = reinterpret_cast<int64_t*>(blk + 64);
    int64_t* q_crow = q_order + nq;
    int64_t* l_order = q_crow + nq;
    int64_t* l_crow = l_order + nl;
    int64_t* toff = l_crow + nl;
    float* q_pmzs = reinterpret_cast<float*>(toff + n_tiles + 1);
    float* l_pmzs = q_pmzs + nq;
    int32_t* q_node = reinterpret_cast<int32_t*>(l_pmzs + nl);
    int32_t* l_node = q_node + nq;
    int32_t* chunks = l_node + nl;
    int32_t* first = chunks + n_tiles;
    int32_t* end = first + n_tiles;
    FAL_CHECK_HIP(hipMemsetAsync(blk, 0, 64, st));
    FAL_TRY(fal_sort_by_precursor(ctx, q_precursor_mz, nq, q_order, q_pmzs));
    ctx->release(SLOT_SORT);                                     // (the second sort may grow them: the first one's work is enqueued)
    ctx->release(SLOT_SORT2);
    FAL_TRY(fal_sort_by_precursor(ctx, l_precursor_mz, nl, l_order, l_pmzs));
    const LibRule rule{fragment_tol, precursor_tol, max_shift, min_cosine, tol_is_da != 0, analog != 0, min_matched};
    hipLaunchKernelGGL(lib_prepare_kernel, dim3(capped_grid(ctx, nq, kLibBlock)), dim3(kLibBlock), 0, st, q_order, q_rows, q_indptr,
                       q_csr_rows, nq, q_node, q_crow, d_err);
    hipLaunchKernelGGL(lib_prepare_kernel, dim3(capped_grid(ctx, nl, kLibBlock)), dim3(kLibBlock), 0, st, l_order, l_rows, l_indptr,
                       l_csr_rows, nl, l_node, l_crow, d_err);
    hipLaunchKernelGGL(lib_band_kernel, dim3(capped_grid(ctx, n_tiles, kLibBlock)), dim3(kLibBlock), 0, st, q_pmzs, nq, n_tiles, l_pmzs,
                       nl, rule, first, end, chunks);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, chunks, n_tiles, toff, SLOT_LIB6));
    unsigned char* pin = nullptr;
    FAL_TRY(ctx->pinned_reserve(64, (void**)&pin));
    int64_t* h_total = reinterpret_cast<int64_t*>(pin);
    unsigned long long* h_counts = reinterpret_cast<unsigned long long*>(pin + 8);
    int32_t* h_err = reinterpret_cast<int32_t*>(pin + 32);
    // wait 1: the workgroups of the tile launch, and whether every query and library entry names a row of its CSR
    FAL_CHECK_HIP(hipMemcpyAsync(h_total, toff + n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipMemcpyAsync(h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipStreamSynchronize(st));
    FAL_REQUIRE(*h_err == 0, FAL_EINVAL,
                "fal_library_search: a row lies outside the %lld (queries) / %lld (library) rows of its peak CSR, or indptr falls",
                (long long)q_csr_rows, (long long)l_csr_rows);
    const int64_t wgs = *h_total;
    FAL_REQUIRE(wgs < (int64_t)INT32_MAX, FAL_EUNSUPPORTED, "fal_library_search: %lld tiles in scope are more than one launch holds",
                (long long)wgs);
    FAL_REQUIRE(q_mz && q_intensity && l_mz && l_intensity, FAL_EINVAL, "fal_library_search: NULL peak array");
    const LibSide q{ExactPeaks{q_mz, q_intensity, q_indptr, q_crow, fragment_tol, min_matched, d_err}, q_pmzs, q_node, nq};
    const LibSide l{ExactPeaks{l_mz, l_intensity, l_indptr, l_crow, fragment_tol, min_matched, d_err}, l_pmzs, l_node, nl};
    // the tile and greedy launches: once, again when a list was too short (its count is exact: slots past the end are counted,
    // not written), and once more when the hits of the listed pairs, unknown until then, did not fit -- the same pairs give the
    // same hits every time
    const int64_t pairs_bound = std::min<int64_t>(wgs * kExTile * kExTile, kLibListBudget);
    int64_t small_cap = std::max<int64_t>(1, pairs_bound), large_cap = std::max<int64_t>(1, pairs_bound / 16),
            hit_cap = std::max<int64_t>(1, pairs_bound);
    LibHits ht{nullptr, nullptr, 0, d_counts};
    int64_t m = 0;
    ctx->stage_reset(ST_KERNEL);
    ctx->stage_reset(ST_TAIL);
    for (int run = 0;; ++run) {
        FAL_REQUIRE(run < 3, FAL_EINTERNAL, "fal_library_search: the lists did not settle");
        int2* lists = nullptr;
        FAL_TRY(ctx->reserve(SLOT_LIB2, sizeof(int2) * (size_t)(small_cap + large_cap), (void**)&lists));
        FAL_TRY(ctx->reserve(SLOT_LIB3, 2 * sizeof(uint64_t) * (size_t)hit_cap, (void**)&ht.keys));
        ht.vals = ht.keys + hit_cap;
        ht.cap = hit_cap;
        int2* small = lists;
        int2* large = lists + small_cap;
        FAL_CHECK_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), st));
        if (wgs > 0) {
            StageScope ts(ctx, ST_KERNEL);
            hipLaunchKernelGGL(lib_tile_kernel, dim3((unsigned)wgs), dim3(kLibBlock), 0, st, toff, n_tiles, first, end, q, l, rule, ht,
                               small, small_cap, large, large_cap, d_err);
        }
        {
            StageScope ts(ctx, ST_TAIL);
            hipLaunchKernelGGL(lib_greedy_kernel<kLibSmall>, dim3((unsigned)std::min<int64_t>(small_cap, (int64_t)ctx->num_cus * 64)),
                               dim3(64), 0, st, small, d_counts + LIB_N_SMALL, small_cap, q, l, rule, ht);
            hipLaunchKernelGGL(lib_greedy_kernel<kNetMaxPeaks>, dim3((unsigned)std::min<int64_t>(large_cap, (int64_t)ctx->num_cus * 4)),
                               dim3(64), 0, st, large, d_counts + LIB_N_LARGE, large_cap, q, l, rule, ht);
        }
        FAL_CHECK_HIP(hipGetLastError());
        // waits 2 to 4: the counts and the error word
        FAL_CHECK_HIP(hipMemcpyAsync(h_counts, d_counts, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipMemcpyAsync(h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        FAL_REQUIRE(*h_err == 0, FAL_EUNSUPPORTED, "fal_library_search: a pair in scope has a spectrum of more than %d peaks",
                    kNetMaxPeaks);
        const int64_t ns = (int64_t)h_counts[LIB_N_SMALL], ng = (int64_t)h_counts[LIB_N_LARGE];
        m = (int64_t)h_counts[LIB_N_HITS];
        ctx->counters[14] = ns + ng;
        if (ns <= small_cap && ng <= large_cap && m <= hit_cap) break;
        small_cap = std::max(small_cap, ns);
        large_cap = std::max(large_cap, ng);
        hit_cap = std::max(hit_cap, m);
        ctx->release(SLOT_LIB2);
        ctx->release(SLOT_LIB3);
    }
    if (m == 0) return FAL_OK;
    // deterministic order: (query, library) keys are unique, a radix sort puts them in place; the second, stable pass by (query,
    // sim descending) keeps equal similarities in that order.
    // SLOT_LIB4: keys, vals u64[m] | place i64[m + 1] | keep i32[m];  SLOT_LIB5: rkey in / out u64[m] | rhit in / out u64[m]
    unsigned char* sb = nullptr;
    FAL_TRY(ctx->reserve(SLOT_LIB4, 28 * (size_t)m + 64, (void**)&sb));
    uint64_t* kout = reinterpret_cast<uint64_t*>(sb);
    uint64_t* vout = kout + m;
    int64_t* place = reinterpret_cast<int64_t*>(vout + m);
    int32_t* keep = reinterpret_cast<int32_t*>(place + m + 1);
    uint64_t* rkey = nullptr;
    FAL_TRY(ctx->reserve(SLOT_LIB5, 32 * (size_t)m, (void**)&rkey));
    uint64_t* rhit = rkey + 2 * m;
    // (the sorts are exact.hip's: the 8-byte values and hit numbers travel as the bit patterns of doubles)
    FAL_TRY(sort_pairs_u64_f64(ctx, ht.keys, kout, reinterpret_cast<double*>(ht.vals), reinterpret_cast<double*>(vout), m, SLOT_LIB7));
    const unsigned hgrid = capped_grid(ctx, m, kLibBlock);
    hipLaunchKernelGGL(lib_rank_entries_kernel, dim3(hgrid), dim3(kLibBlock), 0, st, kout, vout, m, rkey, rhit);
    ctx->release(SLOT_LIB7);                           // (the hit sort is enqueued: its block is retired, not freed, if this one grows)
    FAL_TRY(sort_pairs_u64_f64(ctx, rkey, rkey + m, reinterpret_cast<double*>(rhit), reinterpret_cast<double*>(rhit + m), m, SLOT_LIB7));
    int64_t kept = m;
    if (top_n > 0) {
        hipLaunchKernelGGL(lib_rank_mark_kernel, dim3(hgrid), dim3(kLibBlock), 0, st, rkey + m, m, top_n, keep);
        FAL_CHECK_HIP(hipGetLastError());
        ctx->release(SLOT_LIB6);
        FAL_TRY(device_scan_i32(ctx, keep, m, place, SLOT_LIB6));
        // wait 5: the hits the ranks kept
        FAL_CHECK_HIP(hipMemcpyAsync(h_total, place + m, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        kept = *h_total;
    }
    *n_hits = kept;
    FAL_REQUIRE(kept <= max_hits, FAL_EINVAL, "fal_library_search: %lld hits do not fit max_hits %lld", (long long)kept,
                (long long)max_hits);
    if (kept == 0) return FAL_OK;
    FAL_REQUIRE(hit_query && hit_library && hit_sim && hit_matched, FAL_EINVAL, "fal_library_search: NULL hit array");
    hipLaunchKernelGGL(lib_output_kernel, dim3(hgrid), dim3(kLibBlock), 0, st, kout, vout, rhit + m, m,
                       top_n > 0 ? keep : (const int32_t*)nullptr, top_n > 0 ? place : (const int64_t*)nullptr, hit_query, hit_library,
                       hit_sim, hit_matched);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
