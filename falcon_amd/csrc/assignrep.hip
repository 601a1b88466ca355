// Assign new spectra to the representatives of an existing clustering: for every query spectrum the nearest library spectrum,
// by the matched-peak cosine of exact mode, among the library rows inside its precursor (and retention-time) tolerance
// (DESIGN.md "Assigning to representatives" states the rule; assignrep.h holds its pure core).
//
// Both sides are sorted by precursor m/z.  A workgroup owns a tile of 64 consecutive sorted queries and every gridDim.y-th
// 64-row chunk of the library range that holds all their candidates (binary search on the sorted library precursors, a
// superset: the per-pair test decides).  The tile's and the chunk's peak lists are staged in LDS with exact mode's staging
// (exwalk.h); wave w scores query rows w, w + 4, ... of the tile, lane j against library row j of the chunk, with the scalar
// window walk.  A pair with a component of two or more query peaks goes to a fallback list that a second kernel finishes with
// the Hungarian solver.  A query's running minimum is the 64-bit key of assignrep.h: reduced over the wave on the DPP network,
// kept in a register of the lane that owns the row, one global atomicMin per query and workgroup at the end; the solver kernel
// mins into the same keys.  The minimum of a set of keys does not depend on the order they arrive in.
// exwalk.h's: the staging, the walk, the append, the 64-bit wave minimum and the host's settle loop of the fallback list.
#include <math.h>
#include <algorithm>
#include "assignrep.h"
#include "common.h"
#include "exwalk.h"
#include "ivf.h"
#include "peakmatch.h"

namespace fal {

struct AsSide {
    ExactPeaks pk;              // peaks CSR + order (sorted position -> row of the CSR)
    const float* pmz_sorted;    // precursor m/z by sorted position
    const float* rt;            // retention time by row (or NULL)
    int32_t n;
};

struct AsRule {
    double tol, rt_tol;
    int is_da;
};

__device__ __forceinline__ float as_lane_f32(float v, int lane) {            // (lane: wave-uniform)
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane));
}

// first position of the sorted precursors with (double)mz >= x (strict = false) or > x (strict = true)
__device__ __forceinline__ int32_t as_lower(const float* __restrict__ mz, int32_t n, double x, bool strict) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        const double v = (double)mz[mid];
        if (strict ? v <= x : v < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void assign_score_kernel(AsSide q, AsSide l, AsRule rule, unsigned long long* __restrict__ keys,
                                                           int32_t* __restrict__ n_cand, int2* __restrict__ fb, int64_t fb_cap,
                                                           unsigned long long* __restrict__ n_fb) {
    __shared__ float s_mz[2][kExLdsPeaks];
    __shared__ float s_it[2][kExLdsPeaks];
    __shared__ int64_t s_off[2][64];
    __shared__ int s_len[2][128];
    __shared__ int s_tot[2];
    __shared__ int32_t s_rng[2];
    const int32_t t0 = (int32_t)blockIdx.x * kExTile;
    const int nq_rows = min(kExTile, q.n - t0);
    if (threadIdx.x == 0) {                                            // the library range of the tile's candidates
        double lo = 0.0, hi = 0.0;
        int32_t a = 0, b = l.n;
        if (as_window(q.pmz_sorted[t0], q.pmz_sorted[t0 + nq_rows - 1], rule.tol, rule.is_da, &lo, &hi)) {
            a = as_lower(l.pmz_sorted, l.n, lo, false);
            b = as_lower(l.pmz_sorted, l.n, hi, true);
        }
        s_rng[0] = a;
        s_rng[1] = max(a, b);
    }
    __syncthreads();
    const int32_t lo = s_rng[0], hi = s_rng[1];
    const int32_t n_chunks = (hi - lo + kExTile - 1) / kExTile;
    if ((int32_t)blockIdx.y >= n_chunks) return;                       // (the whole workgroup)
    const bool fa = ex_stage(q.pk, t0, nq_rows, s_mz[0], s_it[0], s_off[0], s_len[0], &s_tot[0]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // lane k < 16 of wave w owns tile row w + 4 k: its precursor, retention time and dataset row, its running minimum and count
    const int my_i = w + 4 * lane;
    const bool mine = lane < 16 && my_i < nq_rows;
    const int32_t my_row = mine ? (int32_t)q.pk.order[t0 + my_i] : 0;
    const float my_pmz = mine ? q.pmz_sorted[t0 + my_i] : 0.f;
    const float my_rt = mine && q.rt ? q.rt[my_row] : 0.f;
    const bool has_rt = q.rt && l.rt;
    uint64_t best = kAsEmptyKey;
    int32_t cnt = 0;
    for (int32_t c = (int32_t)blockIdx.y; c < n_chunks; c += (int32_t)gridDim.y) {
        const int32_t l0 = lo + c * kExTile;
        const int nl_rows = min(kExTile, hi - l0);
        const bool fl = ex_stage(l.pk, l0, nl_rows, s_mz[1], s_it[1], s_off[1], s_len[1], &s_tot[1]);
        const bool row = lane < nl_rows;                               // lane j scores library row l0 + j
        const float l_pmz = row ? l.pmz_sorted[l0 + lane] : 0.f;
        const float l_rt = row && l.rt ? l.rt[l.pk.order[l0 + lane]] : 0.f;
        const float* bmz = fl ? s_mz[1] + s_len[1][64 + lane] : l.pk.mz + s_off[1][lane];
        const float* bit = fl ? s_it[1] + s_len[1][64 + lane] : l.pk.it + s_off[1][lane];
        const int nb = s_len[1][lane];
        for (int k = 0; k < kExTile / 4; ++k) {                        // (wave-uniform control flow: every lane reaches the ballots)
            const int i = w + 4 * k;
            if (i >= nq_rows) break;
            const float q_pmz = as_lane_f32(my_pmz, k), q_rt = as_lane_f32(my_rt, k);
            const int32_t q_row = __builtin_amdgcn_readlane(my_row, k);
            const bool valid = row && as_candidate(q_pmz, l_pmz, rule.tol, rule.is_da, has_rt, q_rt, l_rt, rule.rt_tol);
            const unsigned long long vm = __ballot(valid);
            if (vm == 0) continue;
            bool fall = false;
            uint64_t key = kAsEmptyKey;
            if (valid) {
                const float* amz = fa ? s_mz[0] + s_len[0][64 + i] : q.pk.mz + s_off[0][i];
                const float* ait = fa ? s_it[0] + s_len[0][64 + i] : q.pk.it + s_off[0][i];
                const PeakLists s{amz, ait, bmz, bit};
                double score = 0.0;
                int n_match = 0;
                if (ex_score_simple(s, s_len[0][i], nb, q.pk.tol, &score, &n_match))
                    key = as_pack((float)pair_distance(score, n_match, q.pk.min_matches), (uint32_t)(l0 + lane));
                else
                    fall = true;
            }
            const uint64_t wk = ex_wave_min_u64(key);
            if (lane == k) {
                best = wk < best ? wk : best;
                cnt += __popcll(vm);
            }
            const unsigned long long f = ex_wave_slot(fall, n_fb);
            if (fall && f < (unsigned long long)fb_cap) fb[f] = make_int2(q_row, l0 + lane);
        }
        __syncthreads();                                               // the next chunk is staged over this one
    }
    if (mine) {
        if (best != kAsEmptyKey) atomicMin(&keys[my_row], (unsigned long long)best);
        if (cnt) atomicAdd(&n_cand[my_row], cnt);
    }
}

// the fallback list: (query row, library position) pairs with a component of two or more query peaks
__global__ __launch_bounds__(256) void assign_fallback_kernel(const int2* __restrict__ fb, const unsigned long long* __restrict__ n_fb,
                                                              int64_t fb_cap, ExactPeaks qpk, ExactPeaks lpk,
                                                              unsigned long long* __restrict__ keys) {
    const int64_t m = min((int64_t)*n_fb, fb_cap);
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < m; x += (int64_t)gridDim.x * blockDim.x) {
        const int2 ij = fb[x];
        const int64_t a = ij.x, b = lpk.order[ij.y];
        const int64_t a0 = qpk.indptr[a], b0 = lpk.indptr[b];
        const PeakLists s{qpk.mz + a0, qpk.it + a0, lpk.mz + b0, lpk.it + b0};
        double score = 0.0;
        int n_match = 0;
        if (!pair_score(s, (int)(qpk.indptr[a + 1] - a0), (int)(lpk.indptr[b + 1] - b0), qpk.tol, &score, &n_match))
            atomicExch(qpk.err, 1);
        atomicMin(&keys[a], (unsigned long long)as_pack((float)pair_distance(score, n_match, qpk.min_matches), (uint32_t)ij.y));
    }
}

// keys -> the outputs, through the library's order
__global__ void assign_unpack_kernel(const unsigned long long* __restrict__ keys, int64_t nq, const int64_t* __restrict__ l_order,
                                     int32_t* __restrict__ best_row, float* __restrict__ best_dist) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        const bool none = key == kAsEmptyKey;
        best_row[i] = none ? -1 : (int32_t)l_order[as_key_pos(key)];
        best_dist[i] = none ? 1.0f : as_key_dist(key);
    }
}

}  // namespace fal
FAL_WARM_KERNEL(fal::assign_score_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_assign_nearest(fal_ctx* ctx, const float* q_mz, const float* q_intensity, const int64_t* q_indptr,
                                  const float* q_precursor_mz, const float* q_rt, int64_t nq, const float* l_mz,
                                  const float* l_intensity, const int64_t* l_indptr, const float* l_precursor_mz, const float* l_rt,
                                  int64_t nl, double tol, int tol_is_da, double rt_tol, double fragment_tol, int min_matches,
                                  int32_t* best_row, float* best_dist, int32_t* n_cand) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && nq >= 0 && nl >= 0 && nq < (int64_t)INT32_MAX && nl < (int64_t)INT32_MAX && tol >= 0.0 && fragment_tol >= 0.0,
                FAL_EINVAL, "fal_assign_nearest: bad argument");
    if (nq == 0) return FAL_OK;
    FAL_REQUIRE(q_mz && q_intensity && q_indptr && q_precursor_mz && best_row && best_dist && n_cand, FAL_EINVAL,
                "fal_assign_nearest: NULL array");
    FAL_REQUIRE(nl == 0 || (l_mz && l_intensity && l_indptr && l_precursor_mz), FAL_EINVAL, "fal_assign_nearest: NULL library array");
    FAL_REQUIRE(!(rt_tol >= 0.0) || nl == 0 || (q_rt && l_rt), FAL_EINVAL,
                "fal_assign_nearest: a retention-time tolerance needs the retention times of both sides");
    hipStream_t st = ctx->stream;
    ScratchLayout L;
    const auto keys = L.array<unsigned long long>(nq);
    const auto q_order = L.array<int64_t>(nq), l_order = L.array<int64_t>(nl);
    const auto q_pmzs = L.array<float>(nq), l_pmzs = L.array<float>(nl);
    L.pad(64);
    FAL_TRY(L.reserve(ctx, SLOT_ASSIGN));
    int32_t* misc = nullptr;                                     // [0] error word, [2..3] fallback pairs
    FAL_TRY(ctx->reserve(SLOT_EXACT5, 64, (void**)&misc));
    unsigned long long* d_fb = reinterpret_cast<unsigned long long*>(misc + 2);
    FAL_CHECK_HIP(hipMemsetAsync(misc, 0, 64, st));
    ctx->counters[9] = 0;
    const int ugrid = (int)std::min<int64_t>(ceil_div(nq, 256), (int64_t)ctx->num_cus * 8);
    if (nl > 0) {
        FAL_TRY(fal_sort_by_precursor(ctx, q_precursor_mz, nq, q_order, q_pmzs));
        ctx->release(SLOT_SORT);                                 // (the second sort may grow them: the first one's work is enqueued)
        ctx->release(SLOT_SORT2);
        FAL_TRY(fal_sort_by_precursor(ctx, l_precursor_mz, nl, l_order, l_pmzs));
        AsSide q{ExactPeaks{q_mz, q_intensity, q_indptr, q_order, fragment_tol, min_matches, misc}, q_pmzs, q_rt, (int32_t)nq};
        AsSide l{ExactPeaks{l_mz, l_intensity, l_indptr, l_order, fragment_tol, min_matches, misc}, l_pmzs, l_rt, (int32_t)nl};
        const AsRule rule{tol, rt_tol, tol_is_da != 0};
        const int64_t tiles = ceil_div(nq, kExTile), chunks = ceil_div(nl, kExTile);
        // slices of a tile's library range: one, unless the tiles alone leave compute units idle
        const int64_t slices = std::min<int64_t>(std::min<int64_t>(chunks, 65535), std::max<int64_t>(1, ceil_div(4ll * ctx->num_cus, tiles)));
        ctx->stage_reset(ST_KERNEL);
        // every round clears the keys and counts again: the keys are a minimum, the same pairs give the same result
        return ex_settle_fallback(ctx, SLOT_ASSIGN2, nq * nl, misc, "fal_assign_nearest", [&](int2* fb, int64_t fb_cap) -> int {
            FAL_CHECK_HIP(hipMemsetAsync(keys, 0xFF, sizeof(unsigned long long) * (size_t)nq, st));
            FAL_CHECK_HIP(hipMemsetAsync(n_cand, 0, sizeof(int32_t) * (size_t)nq, st));
            {
                StageScope ts(ctx, ST_KERNEL);
                hipLaunchKernelGGL(assign_score_kernel, dim3((unsigned)tiles, (unsigned)slices), dim3(256), 0, st, q, l, rule, keys, n_cand,
                                   fb, fb_cap, d_fb);
            }
            hipLaunchKernelGGL(assign_fallback_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(fb_cap, 256), (int64_t)ctx->num_cus * 8)),
                               dim3(256), 0, st, fb, d_fb, fb_cap, q.pk, l.pk, keys);
            hipLaunchKernelGGL(assign_unpack_kernel, dim3(ugrid), dim3(256), 0, st, keys, nq, l_order, best_row, best_dist);
            return FAL_OK;
        });
    }
    FAL_CHECK_HIP(hipMemsetAsync(keys, 0xFF, sizeof(unsigned long long) * (size_t)nq, st));
    FAL_CHECK_HIP(hipMemsetAsync(n_cand, 0, sizeof(int32_t) * (size_t)nq, st));
    hipLaunchKernelGGL(assign_unpack_kernel, dim3(ugrid), dim3(256), 0, st, keys, nq, l_order, best_row, best_dist);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
