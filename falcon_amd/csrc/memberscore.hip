// Member scores and cluster summary (fal_member_scores, fal_cluster_summary; DESIGN.md "Member scores and cluster summary";
// memberscore.h holds the pure core).
//
// Members are ordered by (label, row) with the context's stable radix sort.  A workgroup of one wave takes tiles of 64
// consecutive members of that order: lane j owns member j of the tile.  The labels of a tile do not decrease, so its distinct
// clusters are the runs of equal labels; the wave numbers them with one ballot, and the members' peak lists and the runs'
// representatives are staged in LDS once per tile (exwalk.h's scheme and budget: kExLdsPeaks peaks a side; a side that does not
// fit is read from global memory).  Every lane then scores its member against its run's representative with the scalar window
// walk.  A pair with a component of two or more query peaks goes to a fallback list that a second kernel finishes with the
// Hungarian solver; every member is written by exactly one of the two kernels.  exwalk.h's: the walk, the append, the 64-bit
// wave minimum and the host's settle loop of the fallback list; ms_stage below is its ex_stage for rows the lanes bring.
//
// The summary is one wave per cluster over the cluster's segment of the same order: lane l walks members l, l + 64, ... -- chain
// l of memberscore.h -- and the 64 chain sums are added in lane order, so a cluster's bits depend on its members alone.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "exwalk.h"
#include "ivf.h"
#include "memberscore.h"
#include "peakmatch.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kMsBlock = 256;
static_assert(kMsChains == 64, "one chain of the float64 sum per lane of the summary's wave");

struct MsCsr {
    const float* mz;
    const float* it;
    const int64_t* indptr;
    int64_t rows;
};

__global__ void ms_label_keys_kernel(const int32_t* __restrict__ labels, int64_t n, uint32_t* __restrict__ key,
                                     int32_t* __restrict__ row) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        key[i] = (uint32_t)labels[i];          // a negative label sorts behind every cluster
        row[i] = (int32_t)i;
    }
}

// first member of every cluster (and of the end) in the sorted rows: the first position whose key is >= c
__global__ void ms_cluster_start_kernel(const uint32_t* __restrict__ key, int64_t n, int64_t n_clusters, int64_t* __restrict__ cstart) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c <= n_clusters; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)key[mid] < c) lo = mid + 1; else hi = mid;
        }
        cstart[c] = lo;
    }
}

// peaks of a CSR row as (offset, count); a row outside the CSR or with a decreasing indptr holds none
__device__ __forceinline__ void ms_row_peaks(const MsCsr& s, int64_t r, int64_t* g, int* l) {
    *g = 0;
    *l = 0;
    if (r < 0 || r >= s.rows) return;
    const int64_t a = s.indptr[r], c = s.indptr[r + 1] - a;
    *g = a;
    *l = c > 0 ? (int)std::min<int64_t>(c, 0x7FFFFFFF) : 0;
}

// ex_stage's scheme for a workgroup of ONE wave whose lane t brings row t's (global offset, peaks) itself: the peaks of rows
// 0 .. nr into LDS when they fit; off[t] the global offset, len[t] the peaks, len[64 + t] the LDS offset
__device__ __forceinline__ bool ms_stage(const float* __restrict__ mz, const float* __restrict__ it, int64_t g, int l, int nr,
                                         float* lmz, float* lit, int64_t* off, int* len, int* tot) {
    const int tid = threadIdx.x;
    const int lc = min(l, kExLdsPeaks + 1);                      // (the sum of 64 of these cannot overflow; it fits only when lc == l)
    const int incl = wave_prefix_sum(lc);
    off[tid] = g;
    len[tid] = l;
    len[64 + tid] = incl - lc;
    if (tid == 63) *tot = incl;
    __syncthreads();
    const bool fits = *tot <= kExLdsPeaks;
    if (fits) {
        for (int r = 0; r < nr; ++r) {
            const int64_t gr = off[r];
            const int lr = len[r], lo = len[64 + r];
            for (int x = tid; x < lr; x += 64) {
                lmz[lo + x] = mz[gr + x];
                lit[lo + x] = it[gr + x];
            }
        }
    }
    __syncthreads();
    return fits;
}

__global__ __launch_bounds__(64) void ms_score_kernel(MsCsr m, MsCsr rep, const uint32_t* __restrict__ key,
                                                      const int32_t* __restrict__ row, int64_t n, int64_t n_clusters,
                                                      const int32_t* __restrict__ rep_row, double tol, float* __restrict__ similarity,
                                                      int32_t* __restrict__ matched, int2* __restrict__ fb, int64_t fb_cap,
                                                      unsigned long long* __restrict__ n_fb) {
    __shared__ float s_mz[2][kExLdsPeaks];
    __shared__ float s_it[2][kExLdsPeaks];
    __shared__ int64_t s_off[2][64];
    __shared__ int s_len[2][128];
    __shared__ int s_tot[2];
    __shared__ uint32_t s_run[64];           // cluster of the tile's r-th run
    __shared__ int32_t s_rrow[64];           // its representative's row of the representative CSR
    const int lane = threadIdx.x;
    const int64_t n_tiles = (n + kExTile - 1) / kExTile;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {         // (wave-uniform control flow down to the stores)
        const int64_t t0 = tile * kExTile;
        const int n_rows = (int)min((int64_t)kExTile, n - t0);
        const bool valid = lane < n_rows;
        const uint32_t k = valid ? key[t0 + lane] : 0xFFFFFFFFu;
        const int32_t r = valid ? row[t0 + lane] : 0;
        const bool in = valid && (int64_t)k < n_clusters;                         // (a label outside the clusters: 0 with 0 matches)
        int64_t ga = 0;
        int la = 0;
        if (in) ms_row_peaks(m, r, &ga, &la);
        const bool fa = ms_stage(m.mz, m.it, ga, la, n_rows, s_mz[0], s_it[0], s_off[0], s_len[0], &s_tot[0]);
        // the runs of equal labels: a head lane starts one; a lane's run is the number of heads up to it, less one
        const uint32_t k_prev = (uint32_t)__shfl_up((int)k, 1, 64);
        const bool head = in && (lane == 0 || k != k_prev);
        const unsigned long long heads = __ballot(head);
        const int n_runs = __popcll(heads);
        const int run = __popcll(heads & (~0ull >> (63 - lane))) - 1;             // (in: >= 0, the lanes of a run follow its head)
        if (head) s_run[run] = k;
        __syncthreads();
        int64_t gb = 0;
        int lb = 0;
        int32_t rr = -1;
        if (lane < n_runs) {
            rr = rep_row[s_run[lane]];                                            // (s_run holds clusters below n_clusters)
            ms_row_peaks(rep, rr, &gb, &lb);
        }
        s_rrow[lane] = rr;
        const bool fr = ms_stage(rep.mz, rep.it, gb, lb, n_runs, s_mz[1], s_it[1], s_off[1], s_len[1], &s_tot[1]);
        bool fall = false;
        float sim = 0.f;
        int nm = 0;
        int32_t pair_rep = -1;
        if (in) {
            const float* amz = fa ? s_mz[0] + s_len[0][64 + lane] : m.mz + ga;
            const float* ait = fa ? s_it[0] + s_len[0][64 + lane] : m.it + ga;
            const float* bmz = fr ? s_mz[1] + s_len[1][64 + run] : rep.mz + s_off[1][run];
            const float* bit = fr ? s_it[1] + s_len[1][64 + run] : rep.it + s_off[1][run];
            const PeakLists s{amz, ait, bmz, bit};
            double score = 0.0;
            int n_match = 0;
            if (ex_score_simple(s, la, s_len[1][run], tol, &score, &n_match)) {
                sim = ms_similarity(score);
                nm = n_match;
            } else {
                fall = true;
                pair_rep = s_rrow[run];
            }
        }
        const unsigned long long f = ex_wave_slot(fall, n_fb);
        if (fall && f < (unsigned long long)fb_cap) fb[f] = make_int2(r, pair_rep);
        if (valid && !fall) {
            similarity[r] = sim;
            matched[r] = nm;
        }
        __syncthreads();                                                          // the next tile is staged over this one
    }
}

// the fallback list: (member row, representative row) pairs with a component of two or more query peaks
__global__ __launch_bounds__(kMsBlock) void ms_fallback_kernel(const int2* __restrict__ fb, const unsigned long long* __restrict__ n_fb,
                                                               int64_t fb_cap, MsCsr m, MsCsr rep, double tol,
                                                               float* __restrict__ similarity, int32_t* __restrict__ matched,
                                                               int32_t* __restrict__ err) {
    const int64_t cnt = min((int64_t)*n_fb, fb_cap);
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < cnt; x += (int64_t)gridDim.x * blockDim.x) {
        const int2 ij = fb[x];
        int64_t ga, gb;
        int la, lb;
        ms_row_peaks(m, ij.x, &ga, &la);
        ms_row_peaks(rep, ij.y, &gb, &lb);
        const PeakLists s{m.mz + ga, m.it + ga, rep.mz + gb, rep.it + gb};
        double score = 0.0;
        int n_match = 0;
        if (!pair_score(s, la, lb, tol, &score, &n_match)) atomicExch(err, 1);
        if (ij.x >= 0 && (int64_t)ij.x < m.rows) {
            similarity[ij.x] = ms_similarity(score);
            matched[ij.x] = n_match;
        }
    }
}

__device__ __forceinline__ float ms_wave_fmin(float v) {
    return wave_xor_reduce(v, [](float a, float b) { return fminf(a, b); });
}

__device__ __forceinline__ float ms_wave_fmax(float v) {
    return wave_xor_reduce(v, [](float a, float b) { return fmaxf(a, b); });
}

// one wave per cluster: lane l folds members l, l + 64, ... of the cluster's segment (chain l), then the chains in lane order
__global__ __launch_bounds__(kMsBlock) void ms_summary_kernel(const int64_t* __restrict__ cstart, const int32_t* __restrict__ row,
                                                              int64_t n_clusters, const float* __restrict__ similarity,
                                                              const float* __restrict__ pmz, const float* __restrict__ rt,
                                                              int32_t* __restrict__ size, float* __restrict__ sim_min,
                                                              int32_t* __restrict__ worst_row, double* __restrict__ sim_mean,
                                                              float* __restrict__ pmz_min, float* __restrict__ pmz_max,
                                                              float* __restrict__ rt_min, float* __restrict__ rt_max) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)kMsBlock + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * kMsBlock) >> 6;
    for (int64_t c = wave; c < n_clusters; c += n_waves) {                        // (wave-uniform)
        const int64_t a = cstart[c], b = cstart[c + 1];
        MsFold f;
        double chain = 0.0;
        for (int64_t p = a + lane; p < b; p += kMsChains) {
            const int32_t r = row[p];
            const float s = similarity[r];
            ms_chain_add(chain, s);
            ms_fold_add(f, s, r, pmz[r], rt ? rt[r] : 0.f);
        }
        double total = 0.0;
        for (int l = 0; l < kMsChains; ++l) ms_total_add(total, __shfl(chain, l, 64));
        f.key = ex_wave_min_u64(f.key);
        f.pmz_min = ms_wave_fmin(f.pmz_min);
        f.pmz_max = ms_wave_fmax(f.pmz_max);
        f.rt_min = ms_wave_fmin(f.rt_min);
        f.rt_max = ms_wave_fmax(f.rt_max);
        if (lane == 0) {
            const MsRow o = ms_row(f, total, b - a);
            size[c] = o.size;
            sim_min[c] = o.sim_min;
            worst_row[c] = o.worst_row;
            sim_mean[c] = o.sim_mean;
            pmz_min[c] = o.pmz_min;
            pmz_max[c] = o.pmz_max;
            rt_min[c] = o.rt_min;
            rt_max[c] = o.rt_max;
        }
    }
}

// the members in (label, row) order: key u32[n] (the label), row i32[n]; with cstart_out, the first member of every cluster.
// One block of SLOT_MSCORE.
int ms_order(fal_ctx* ctx, const int32_t* labels, int64_t n, int64_t n_clusters, int32_t** misc_out, const uint32_t** key_out,
             const int32_t** row_out, const int64_t** cstart_out) {
    hipStream_t st = ctx->stream;
    const int64_t n1 = std::max<int64_t>(n, 1);
    ScratchLayout L;
    const auto misc = L.array<int32_t>(16);                // 64 B of meta words
    const auto cstart = L.array<int64_t>(n_clusters + 1);
    const auto key_in = L.array<uint32_t>(n1), key = L.array<uint32_t>(n1);
    const auto row_in = L.array<int32_t>(n1), row = L.array<int32_t>(n1);
    FAL_TRY(L.reserve(ctx, SLOT_MSCORE));
    FAL_CHECK_HIP(hipMemsetAsync(misc, 0, 64, st));
    if (n > 0) {
        hipLaunchKernelGGL(ms_label_keys_kernel, dim3(capped_grid(ctx, n, kMsBlock)), dim3(kMsBlock), 0, st, labels, n, key_in, row_in);
        FAL_CHECK_HIP(hipGetLastError());
        FAL_TRY(sort_pairs_u32_i32(ctx, key_in, key, row_in, row, n, 32, SLOT_SORT));
    }
    if (cstart_out) {
        hipLaunchKernelGGL(ms_cluster_start_kernel, dim3(capped_grid(ctx, n_clusters + 1, kMsBlock)), dim3(kMsBlock), 0, st, key, n,
                           n_clusters, cstart);
        FAL_CHECK_HIP(hipGetLastError());
        *cstart_out = cstart;
    }
    *misc_out = misc;
    *key_out = key;
    *row_out = row;
    return FAL_OK;
}

}  // namespace
}  // namespace fal
FAL_WARM_KERNEL(fal::ms_score_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_member_scores(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n,
                                 const int32_t* labels, int64_t n_clusters, const float* rep_mz, const float* rep_intensity,
                                 const int64_t* rep_indptr, int64_t n_rep, const int32_t* rep_row, double fragment_tol,
                                 float* similarity, int32_t* matched) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && n_clusters >= 0 && n_rep >= 0 && n < (int64_t)INT32_MAX && n_clusters < (int64_t)INT32_MAX &&
                    n_rep < (int64_t)INT32_MAX && fragment_tol >= 0.0,
                FAL_EINVAL, "fal_member_scores: bad argument");
    if (n == 0) return FAL_OK;
    FAL_REQUIRE(mz && intensity && indptr && labels && similarity && matched, FAL_EINVAL, "fal_member_scores: NULL array");
    FAL_REQUIRE(n_clusters == 0 || rep_row, FAL_EINVAL, "fal_member_scores: NULL rep_row");
    FAL_REQUIRE(n_rep == 0 || (rep_mz && rep_intensity && rep_indptr), FAL_EINVAL, "fal_member_scores: NULL representative array");
    hipStream_t st = ctx->stream;
    int32_t* misc = nullptr;                                         // [0] error word, [2..3] fallback pairs
    const uint32_t* key = nullptr;
    const int32_t* row = nullptr;
    FAL_TRY(ms_order(ctx, labels, n, n_clusters, &misc, &key, &row, nullptr));
    unsigned long long* d_fb = reinterpret_cast<unsigned long long*>(misc + 2);
    ctx->counters[9] = 0;
    const MsCsr m{mz, intensity, indptr, n}, rep{rep_mz, rep_intensity, rep_indptr, n_rep};
    const int64_t tiles = ceil_div(n, kExTile);
    const unsigned grid = (unsigned)std::min<int64_t>(tiles, (int64_t)ctx->num_cus * 12);
    ctx->stage_reset(ST_KERNEL);
    // every round runs both kernels again: every member is written again by one of the two, the same pairs give the same result
    return ex_settle_fallback(ctx, SLOT_MSCORE2, n, misc, "fal_member_scores", [&](int2* fb, int64_t fb_cap) -> int {
        {
            StageScope ts(ctx, ST_KERNEL);
            hipLaunchKernelGGL(ms_score_kernel, dim3(grid), dim3(64), 0, st, m, rep, key, row, n, n_clusters, rep_row, fragment_tol,
                               similarity, matched, fb, fb_cap, d_fb);
        }
        hipLaunchKernelGGL(ms_fallback_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(fb_cap, kMsBlock), (int64_t)ctx->num_cus * 8)),
                           dim3(kMsBlock), 0, st, fb, d_fb, fb_cap, m, rep, fragment_tol, similarity, matched, misc);
        return FAL_OK;
    });
}

extern "C" int fal_cluster_summary(fal_ctx* ctx, const int32_t* labels, int64_t n, int64_t n_clusters, const float* similarity,
                                   const float* precursor_mz, const float* retention_time, int32_t* size, float* sim_min,
                                   int32_t* worst_row, double* sim_mean, float* pmz_min, float* pmz_max, float* rt_min,
                                   float* rt_max) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && n_clusters >= 0 && n < (int64_t)INT32_MAX && n_clusters < (int64_t)INT32_MAX, FAL_EINVAL,
                "fal_cluster_summary: bad argument");
    if (n_clusters == 0) return FAL_OK;
    FAL_REQUIRE(n == 0 || (labels && similarity && precursor_mz), FAL_EINVAL, "fal_cluster_summary: NULL column");
    FAL_REQUIRE(size && sim_min && worst_row && sim_mean && pmz_min && pmz_max && rt_min && rt_max, FAL_EINVAL,
                "fal_cluster_summary: NULL output");
    int32_t* misc = nullptr;
    const uint32_t* key = nullptr;
    const int32_t* row = nullptr;
    const int64_t* cstart = nullptr;
    FAL_TRY(ms_order(ctx, labels, n, n_clusters, &misc, &key, &row, &cstart));
    hipLaunchKernelGGL(ms_summary_kernel, dim3(capped_grid(ctx, n_clusters * 64, kMsBlock)), dim3(kMsBlock), 0, ctx->stream, cstart, row,
                       n_clusters, similarity, precursor_mz, retention_time, size, sim_min, worst_row, sim_mean, pmz_min, pmz_max,
                       rt_min, rt_max);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
