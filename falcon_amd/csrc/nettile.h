// The pair-tile core of the representative network (network.hip) and the library search (libsearch.hip): the one copy of the
// record, the constants, the bodies of the prepare, tile, greedy-list, rank and output kernels and the host side of a call.
//
// One workgroup per (tile row of 64 sorted positions of side A, chunk of 64 of side B) stages both sides' peak lists in LDS
// (exwalk.h's scheme and budget); every lane takes one pair at a time: the scope test, the peak limit, the orientation, then
// netmatch.h's net_pair -- the window walk over a's peaks and, when that leaves enough peaks with a partner, over b's.  A pair
// below the matched-peak threshold on either side ends there; a conflict-free pair is summed in the walk; every other pair goes
// to one of two compacted lists (sides of up to 64 peaks, larger sides), which the greedy kernel finishes with one wave per pair
// (net_greedy_pair's rounds).  Records are appended (one atomic per wave in the tile kernel, one per pair in the greedy kernel) and
// sorted by their key (exact.hip's 64-bit pair sort): the order of arrival decides nothing.
//
// A unit supplies its __global__ entry points (one-line wrappers: a kernel launches from the unit that defines it) and a *rule*,
// a struct of the call's tol, min_cosine and min_matched with
//   kDiagonal                     chunk 0 of a tile row is the row itself: only pairs j > i, side 0 is staged once for both
//   chunk(t, c, nb, &b0, &b1)     chunk c of tile row t: positions [b0, b0 + 64) of the second side's [0, b1), b1 <= nb
//   in_scope(pa, pb)              the precursor test of a pair (first side, second side)
//   orient(x, y)                  the first and the second side's NetRow -> NetOriented (netmatch.h): a, b and the shift
//   key(nx, ny)                   the 64-bit key of the record from the two sides' indices
// Compile-time: the network's orientation is the identity and its kernels gain no select; the library has no diagonal.
#pragma once
#include <algorithm>
#include "common.h"
#include "exwalk.h"
#include "ivf.h"
#include "netmatch.h"
#include "util.h"

namespace fal {

constexpr int kNetBlock = 256;
constexpr int kNetSmall = 64;                          // sides of the greedy kernel's register-sized form: one strip of 64 peaks
constexpr int64_t kNetListBudget = 1ll << 22;          // listed pairs / records held before the host has seen a count (32 MB / 64 MB)
static_assert(kNetMaxPeaks % 64 == 0 && kNetSmall == 64 && kNetMaxPeaks == FAL_NET_MAX_PEAKS, "strips of one wave");
constexpr int64_t kNetRowPeaks = 1ll << 24;           // peaks of any row: the staging adds up 64 rows' counts in 32 bits
enum { NET_ERR_ROW = 1, NET_ERR_PEAKS = 2 };          // bits of the error word
enum { NET_N_OUT = 0, NET_N_SMALL = 1, NET_N_LARGE = 2 };     // the call's counts (unsigned long long each)

struct NetSide {
    ExactPeaks pk;              // the side's peak CSR + order (sorted position -> row of the CSR)
    const float* pmzs;          // precursor m/z by sorted position
    const int32_t* node;        // the side's index by sorted position
    int64_t n;
};

// the edges / hits of a call: (key, sim bits << 32 | matched); a slot >= cap is counted, not written
struct NetOut {
    uint64_t *keys, *vals;
    int64_t cap;
    unsigned long long* counts;              // NET_N_*
};

__device__ __forceinline__ void net_put(const NetOut& o, unsigned long long slot, uint64_t key, float sim, int matched) {
    if (slot >= (unsigned long long)o.cap) return;
    o.keys[slot] = key;
    o.vals[slot] = ((uint64_t)__float_as_uint(sim) << 32) | (uint32_t)matched;
}

// one side: sorted position p -> its index, its row of the side's peak CSR; a row outside the CSR or with a falling indptr sets
// the error word (and is given row 0 of nothing: no kernel behind this one runs then)
__device__ __forceinline__ void net_prepare_body(const int64_t* __restrict__ order, const int32_t* __restrict__ rows,
                                                 const int64_t* __restrict__ indptr, int64_t n_csr_rows, int64_t n,
                                                 int32_t* __restrict__ node, int64_t* __restrict__ crow, int32_t* __restrict__ err) {
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

// One workgroup per (tile row of side A, chunk of side B): both sides' peak lists staged in LDS, every lane one pair at a time.
template <class Rule>
__device__ __forceinline__ void net_tile_body(const int64_t* __restrict__ toff, int64_t n_tiles, const NetSide& A, const NetSide& B,
                                              const Rule& rule, const NetOut& out, int2* __restrict__ small, int64_t small_cap,
                                              int2* __restrict__ large, int64_t large_cap, int32_t* __restrict__ err) {
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
    const int64_t a0 = lo * kExTile;
    int64_t b0, b1;
    rule.chunk(lo, (int64_t)blockIdx.x - toff[lo], B.n, &b0, &b1);
    if (a0 >= A.n || b0 >= b1 || b1 > B.n) return;                   // (never: the chunks end inside the side; workgroup-uniform)
    const int na_rows = (int)min((int64_t)kExTile, A.n - a0), nb_rows = (int)min((int64_t)kExTile, b1 - b0);
    const bool diag = Rule::kDiagonal && a0 == b0;
    const int sb = diag ? 0 : 1;
    if (threadIdx.x < 64) {
        s_pmz[0][threadIdx.x] = (int)threadIdx.x < na_rows ? A.pmzs[a0 + threadIdx.x] : 0.f;
        s_pmz[1][threadIdx.x] = (int)threadIdx.x < nb_rows ? B.pmzs[b0 + threadIdx.x] : 0.f;
    }
    const bool fa = ex_stage(A.pk, (int32_t)a0, na_rows, s_mz[0], s_it[0], s_off[0], s_len[0], &s_tot[0]);
    bool fb = fa;
    if (!diag) fb = ex_stage(B.pk, (int32_t)b0, nb_rows, s_mz[1], s_it[1], s_off[1], s_len[1], &s_tot[1]);
    const int need = net_need(rule.min_matched);
    for (int p = threadIdx.x; p < kExTile * kExTile; p += kNetBlock) {   // (uniform trip count: every lane reaches the ballots)
        const int i = p >> 6, j = p & 63;
        bool hit = false, to_small = false, to_large = false;
        float sim = 0.f;
        int matched = 0;
        if (i < na_rows && j < nb_rows && (!diag || j > i)) {
            const float pa = s_pmz[0][i], pb = s_pmz[1][j];
            const int la = s_len[0][i], lb = s_len[sb][j];
            if (rule.in_scope(pa, pb)) {
                if (la > kNetMaxPeaks || lb > kNetMaxPeaks) {
                    atomicOr(err, NET_ERR_PEAKS);
                } else if (la >= need && lb >= need) {
                    const NetRow x{fa ? s_mz[0] + s_len[0][64 + i] : A.pk.mz + s_off[0][i],
                                   fa ? s_it[0] + s_len[0][64 + i] : A.pk.it + s_off[0][i], la, pa};
                    const NetRow y{fb ? s_mz[sb] + s_len[sb][64 + j] : B.pk.mz + s_off[sb][j],
                                   fb ? s_it[sb] + s_len[sb][64 + j] : B.pk.it + s_off[sb][j], lb, pb};
                    const NetPair r = net_pair(rule.orient(x, y), rule.tol, need);
                    sim = r.sim, matched = r.matched;                        // (0 matched unless NET_INLINE: no edge then)
                    hit = net_is_edge(sim, matched, rule.min_cosine, rule.min_matched);
                    to_small = r.kind == NET_GREEDY && la <= kNetSmall && lb <= kNetSmall;
                    to_large = r.kind == NET_GREEDY && !to_small;
                }
            }
        }
        const unsigned long long e = ex_wave_slot(hit, out.counts + NET_N_OUT);
        if (hit) net_put(out, e, rule.key(A.node[a0 + i], B.node[b0 + j]), sim, matched);
        const unsigned long long fs = ex_wave_slot(to_small, out.counts + NET_N_SMALL);
        if (to_small && fs < (unsigned long long)small_cap) small[fs] = make_int2((int)(a0 + i), (int)(b0 + j));
        const unsigned long long fl = ex_wave_slot(to_large, out.counts + NET_N_LARGE);
        if (to_large && fl < (unsigned long long)large_cap) large[fl] = make_int2((int)(a0 + i), (int)(b0 + j));
    }
}

// ---- the greedy matching of one listed pair by one wave (netmatch.h's order) --------------------------------------------------
// Peak i of a belongs to lane i mod 64 (strip i / 64).  s_j[i]: the best free partner the peak last found (>= 0), kNetStale
// before the first look, kNetNone when no free partner is left (none comes back: the used peaks only grow), kNetTaken once the
// peak is accepted -- s_w[i] is its weight then.  A round: every lane brings its peaks' offers up to date (an offer stands until
// its partner is used) and keeps the first in the order; the wave takes the largest weight, among equals the lowest i (its j is
// the lowest of that weight: the look goes through b in ascending order).
constexpr int kNetStale = -2, kNetNone = -1, kNetTaken = -3;

// a's peaks (the side with the lower precursor: shift <= 0) against b's; s_w, s_j: kCap entries, s_used: kCap / 32 words of the
// calling wave.  false = a side above kCap (nothing done).  *matched_out in every lane, *sim_out in lane 0 only.  The caller
// puts a wave_lds_sync() behind its use of the result, before the next pair's state goes over this one's.
template <int kCap>
__device__ __forceinline__ bool net_greedy_pair(const float* __restrict__ amz, const float* __restrict__ ait, int la,
                                                const float* __restrict__ bmz, const float* __restrict__ bit, int lb, float shift,
                                                double tol, float* s_w, int* s_j, uint32_t* s_used, float* sim_out, int* matched_out) {
    if (la > kCap || lb > kCap) return false;
    const int lane = threadIdx.x;
    for (int i = lane; i < la; i += 64) s_j[i] = kNetStale;
    for (int q = lane; q < (lb + 31) / 32; q += 64) s_used[q] = 0u;
    wave_lds_sync();
    int matched = 0;
    for (;;) {
        float bw = 0.f;
        int bi = 0x7FFFFFFF, bj = -1;
        for (int i = lane; i < la; i += 64) {
            int cj = s_j[i];
            if (cj == kNetNone || cj == kNetTaken) continue;
            float w = 0.f;
            if (cj >= 0 && !((s_used[cj >> 5] >> (cj & 31)) & 1u)) {
                w = s_w[i];
            } else {                                                      // look again: the free b peaks of both windows
                const float av = amz[i], ai = ait[i];
                int z0, z1, s0, s1;
                net_window(av, bmz, lb, tol, &z0, &z1);
                net_window(av - shift, bmz, lb, tol, &s0, &s1);           // (shift <= 0: this window is not below the other)
                cj = kNetNone;
                for (int q = z0; q < z1; ++q) {
                    if ((s_used[q >> 5] >> (q & 31)) & 1u) continue;
                    const float wq = net_weight(ai, bit[q]);
                    if (wq > w) w = wq, cj = q;
                }
                for (int q = max(s0, z1); q < s1; ++q) {
                    if ((s_used[q >> 5] >> (q & 31)) & 1u) continue;
                    const float wq = net_weight(ai, bit[q]);
                    if (wq > w) w = wq, cj = q;
                }
                s_j[i] = cj;
                s_w[i] = w;
            }
            if (cj >= 0 && w > bw) bw = w, bi = i, bj = cj;               // (ascending i: the first of equal weights stays)
        }
        const uint32_t top = wave_max_u32(__float_as_uint(bw));           // (weights > 0: the bits order like the values)
        if (top == 0u) break;
        const uint32_t win = wave_min_u32(__float_as_uint(bw) == top ? (uint32_t)bi : 0xFFFFFFFFu);
        const int j = __shfl(bj, (int)(win & 63u), 64);
        if (lane == (int)(win & 63u)) {
            s_j[win] = kNetTaken;
            s_used[j >> 5] |= 1u << (j & 31);
        }
        matched += 1;
        wave_lds_sync();
    }
    if (lane == 0) {
        double score = 0.0;
        for (int i = 0; i < la; ++i)
            if (s_j[i] == kNetTaken) net_sum_add(score, s_w[i]);
        *sim_out = net_similarity(score);
    }
    *matched_out = matched;
    return true;
}

// One wave per listed pair (sorted position of side A, of side B): the two rows' peaks in the pair's orientation through
// the rounds above, then the edge rule in lane 0.
template <int kCap, class Rule>
__device__ __forceinline__ void net_greedy_body(const int2* __restrict__ list, const unsigned long long* __restrict__ n_list,
                                                int64_t list_cap, const NetSide& A, const NetSide& B, const Rule& rule,
                                                const NetOut& out) {
    __shared__ float s_w[kCap];
    __shared__ int s_j[kCap];
    __shared__ uint32_t s_used[kCap / 32];
    const int64_t cnt = min((int64_t)*n_list, list_cap);
    for (int64_t x = blockIdx.x; x < cnt; x += gridDim.x) {                   // (wave-uniform control flow)
        const int2 ab = list[x];
        const int64_t ra = A.pk.order[ab.x], rb = B.pk.order[ab.y];
        const int64_t ga = A.pk.indptr[ra], gb = B.pk.indptr[rb];
        const NetOriented o = rule.orient(NetRow{A.pk.mz + ga, A.pk.it + ga, (int)(A.pk.indptr[ra + 1] - ga), A.pmzs[ab.x]},
                                          NetRow{B.pk.mz + gb, B.pk.it + gb, (int)(B.pk.indptr[rb + 1] - gb), B.pmzs[ab.y]});
        float sim = 0.f;
        int matched = 0;
        if (!net_greedy_pair<kCap>(o.a.mz, o.a.it, o.a.len, o.b.mz, o.b.it, o.b.len, o.shift, rule.tol, s_w, s_j, s_used, &sim, &matched))
            continue;                                                         // (never: the tile kernel lists by size)
        if (threadIdx.x == 0 && net_is_edge(sim, matched, rule.min_cosine, rule.min_matched))
            net_put(out, atomicAdd(out.counts + NET_N_OUT, 1ull), rule.key(A.node[ab.x], B.node[ab.y]), sim, matched);
        wave_lds_sync();                                                      // the next pair's state goes over this one's
    }
}

// the first position of the run of equal high 32 bits (the node or query of a rank key) that ends at x: x's rank is x - that
__device__ __forceinline__ int64_t net_run_start(const uint64_t* __restrict__ rkey, int64_t x) {
    const uint32_t nd = (uint32_t)(rkey[x] >> 32);
    int64_t lo = 0, hi = x;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint32_t)(rkey[mid] >> 32) < nd) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the kept entries into the caller's arrays: entry x (kPicked: record pick[x], else record x) to place[x] (place NULL: to x)
template <bool kPicked>
__device__ __forceinline__ void net_output_body(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                const uint64_t* __restrict__ pick, int64_t m, const int32_t* __restrict__ keep,
                                                const int64_t* __restrict__ place, int32_t* __restrict__ out_hi,
                                                int32_t* __restrict__ out_lo, float* __restrict__ out_sim,
                                                int32_t* __restrict__ out_matched) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < m; x += (int64_t)gridDim.x * blockDim.x) {
        if (keep && !keep[x]) continue;
        const int64_t o = place ? place[x] : x;
        const uint64_t e = kPicked ? pick[x] : (uint64_t)x;
        const uint64_t k = keys[e], v = vals[e];
        out_hi[o] = (int32_t)(k >> 32);
        out_lo[o] = (int32_t)(uint32_t)k;
        out_sim[o] = __uint_as_float((uint32_t)(v >> 32));
        out_matched[o] = (int32_t)(uint32_t)v;
    }
}

// ---- the host side of a call -------------------------------------------------------------------------------------------------
// what tells fal_network_edges from fal_library_search behind the first wait: its name and its word for "in scope" in the
// messages, its counter of listed pairs, its scratch slots (lists | records | sorted records | scan | sort)
struct NetCall { const char *name, *scope; int counter, slot_lists, slot_out, slot_sorted, slot_scan, slot_sort; };

// the call's words: the first 64 bytes of its block (zeroed by the caller) and, from net_first_wait on, 64 pinned bytes
struct NetWords {
    int32_t* d_err;
    unsigned long long* d_counts;            // NET_N_*: 3 words
    int64_t* h_total;
    unsigned long long* h_counts;
    int32_t* h_err;
    explicit NetWords(unsigned char* blk) : d_err((int32_t*)blk), d_counts((unsigned long long*)(blk + 8)) {}
};

// one side of a call: the prepare launch (the unit's entry point) and the side as the kernels take it
template <class Kernel>
inline NetSide net_side(fal_ctx* ctx, Kernel prepare, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_csr_rows,
                        const int32_t* rows, int64_t n, const int64_t* order, int64_t* crow, const float* pmzs, int32_t* node,
                        double tol, int min_matched, int32_t* d_err) {
    hipLaunchKernelGGL(prepare, dim3(capped_grid(ctx, n, kNetBlock)), dim3(kNetBlock), 0, ctx->stream, order, rows, indptr, n_csr_rows, n,
                       node, crow, d_err);
    return NetSide{ExactPeaks{mz, intensity, indptr, crow, tol, min_matched, d_err}, pmzs, node, n};
}

// wait 1: the workgroups of the tile launch (*d_total -> *w->h_total) and whether every sorted position names a row of its CSR
// (*w->h_err != 0: the caller's message)
inline int net_first_wait(fal_ctx* ctx, const int64_t* d_total, NetWords* w) {
    unsigned char* pin = nullptr;
    FAL_TRY(ctx->pinned_reserve(64, (void**)&pin));
    w->h_total = reinterpret_cast<int64_t*>(pin);
    w->h_counts = reinterpret_cast<unsigned long long*>(pin + 8);
    w->h_err = reinterpret_cast<int32_t*>(pin + 32);
    FAL_CHECK_HIP(hipMemcpyAsync(w->h_total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipMemcpyAsync(w->h_err, w->d_err, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return FAL_OK;
}

// The tile and greedy launches: once, again when a list was too short (its count is exact: slots past the end are counted, not
// written), and once more when the records of the listed pairs, unknown until then, did not fit -- the same pairs give the same
// records every time.  tile(toff, n_tiles, tail..., out, small, small_cap, large, large_cap, err) and greedy(list,
// n_list, list_cap, out, tail...) are the unit's entry points, tail its sides and rule.  -> *out (in slot_out), its h_counts[NET_N_OUT]
// (The tile kernels take sides and rule in front, as before the fold: with the record and lists in front the same pair loop, in
// other registers, ran 2 % slower on the MI355X in the library search; the greedy kernels measure the same either way.)
template <class TileKernel, class GreedyKernel, class... Tail>
inline int net_settle(fal_ctx* ctx, const NetCall& call, const NetWords& w, const int64_t* toff, int64_t n_tiles, bool peaks_given,
                      TileKernel tile, GreedyKernel greedy_small, GreedyKernel greedy_large, NetOut* out, int64_t* m, Tail... tail) {
    hipStream_t st = ctx->stream;
    const int64_t wgs = *w.h_total;
    FAL_REQUIRE(wgs < (int64_t)INT32_MAX, FAL_EUNSUPPORTED, "%s: %lld tiles %s are more than one launch holds", call.name, (long long)wgs,
                call.scope);
    FAL_REQUIRE(peaks_given, FAL_EINVAL, "%s: NULL peak array", call.name);
    const int64_t pairs_bound = std::min<int64_t>(wgs * kExTile * kExTile, kNetListBudget);
    int64_t small_cap = std::max<int64_t>(1, pairs_bound), large_cap = std::max<int64_t>(1, pairs_bound / 16),
            out_cap = std::max<int64_t>(1, pairs_bound);
    ctx->stage_reset(ST_KERNEL);
    ctx->stage_reset(ST_TAIL);
    for (int run = 0;; ++run) {
        FAL_REQUIRE(run < 3, FAL_EINTERNAL, "%s: the lists did not settle", call.name);
        ScratchLayout LL, LO;
        const auto small = LL.array<int2>(small_cap), large = LL.array<int2>(large_cap);
        FAL_TRY(LL.reserve(ctx, call.slot_lists));
        const auto keys = LO.array<uint64_t>(out_cap), vals = LO.array<uint64_t>(out_cap);
        FAL_TRY(LO.reserve(ctx, call.slot_out));
        *out = NetOut{keys, vals, out_cap, w.d_counts};
        FAL_CHECK_HIP(hipMemsetAsync(w.d_counts, 0, 3 * sizeof(unsigned long long), st));
        if (wgs > 0) {
            StageScope ts(ctx, ST_KERNEL);
            hipLaunchKernelGGL(tile, dim3((unsigned)wgs), dim3(kNetBlock), 0, st, toff, n_tiles, tail..., *out, small, small_cap, large,
                               large_cap, w.d_err);
        }
        {
            StageScope ts(ctx, ST_TAIL);
            hipLaunchKernelGGL(greedy_small, dim3((unsigned)std::min<int64_t>(small_cap, (int64_t)ctx->num_cus * 64)), dim3(64), 0, st,
                               (const int2*)small, (const unsigned long long*)(w.d_counts + NET_N_SMALL), small_cap, *out, tail...);
            hipLaunchKernelGGL(greedy_large, dim3((unsigned)std::min<int64_t>(large_cap, (int64_t)ctx->num_cus * 4)), dim3(64), 0, st,
                               (const int2*)large, (const unsigned long long*)(w.d_counts + NET_N_LARGE), large_cap, *out, tail...);
        }
        FAL_CHECK_HIP(hipGetLastError());
        // waits 2 to 4: the counts and the error word
        FAL_CHECK_HIP(hipMemcpyAsync(w.h_counts, w.d_counts, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipMemcpyAsync(w.h_err, w.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        FAL_REQUIRE(*w.h_err == 0, FAL_EUNSUPPORTED, "%s: a pair %s has a spectrum of more than %d peaks", call.name, call.scope,
                    kNetMaxPeaks);
        const int64_t ns = (int64_t)w.h_counts[NET_N_SMALL], nl = (int64_t)w.h_counts[NET_N_LARGE];
        *m = (int64_t)w.h_counts[NET_N_OUT];
        ctx->counters[call.counter] = ns + nl;
        if (ns <= small_cap && nl <= large_cap && *m <= out_cap) return FAL_OK;
        small_cap = std::max(small_cap, ns);
        large_cap = std::max(large_cap, nl);
        out_cap = std::max(out_cap, *m);
        ctx->release(call.slot_lists);
        ctx->release(call.slot_out);
    }
}

// the m records in the order of their keys (unique: a radix sort puts them in place; the order of arrival decides nothing), in
// slot_sorted.  (The sort is exact.hip's: the 8-byte values travel as the bit patterns of doubles.)
struct NetSorted { uint64_t *keys, *vals; int64_t* place; int32_t* flag; };
inline int net_sort_records(fal_ctx* ctx, const NetCall& call, const NetOut& out, int64_t m, NetSorted* s) {
    ScratchLayout L;
    const auto keys = L.array<uint64_t>(m), vals = L.array<uint64_t>(m);
    const auto place = L.array<int64_t>(m + 1);
    const auto flag = L.array<int32_t>(m);
    L.pad(56);
    FAL_TRY(L.reserve(ctx, call.slot_sorted));
    *s = NetSorted{keys, vals, place, flag};
    return sort_pairs_u64_f64(ctx, out.keys, s->keys, reinterpret_cast<double*>(out.vals), reinterpret_cast<double*>(s->vals), m,
                              call.slot_sort);
}

// wait 5: the records whose flag is 1, and their places
inline int net_count_kept(fal_ctx* ctx, const NetCall& call, const NetWords& w, const NetSorted& s, int64_t m, int64_t* kept) {
    ctx->release(call.slot_scan);
    FAL_TRY(device_scan_i32(ctx, s.flag, m, s.place, call.slot_scan));
    FAL_CHECK_HIP(hipMemcpyAsync(w.h_total, s.place + m, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *kept = *w.h_total;
    return FAL_OK;
}

}  // namespace fal
