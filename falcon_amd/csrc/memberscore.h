// Members scored against their cluster's representative, and the per-cluster summary (DESIGN.md "Member scores and cluster
// summary"): the pure core -- the clip of a pair's score, the 64-bit key whose minimum names a cluster's worst member, the fold of
// the per-cluster columns and the ONE order of the float64 sum behind sim_mean.  Pure functions, shared by memberscore.hip's
// kernels and the host build of the CPU tests (-ffp-contract=off in both).
#pragma once
#include <math.h>
#include "assignrep.h"
#include "peakmatch.h"

namespace fal {

// similarity of a scored pair: the score clipped to [0, 1] in float64 (similarity.py:78), then float32.  min_matched_peaks is
// not applied here: the matched-peak count is reported beside it.
__host__ __device__ __forceinline__ float ms_similarity(double score) { return (float)fmax(0.0, fmin(score, 1.0)); }

// key = (bits of the float32 similarity) << 32 | dataset row: similarities are >= 0, their bits order as unsigned integers, so
// the smallest key is the smallest similarity, then the lowest row (assignrep.h as_pack)
constexpr uint64_t kMsEmptyKey = kAsEmptyKey;
__host__ __device__ __forceinline__ uint64_t ms_key(float sim, int32_t row) { return as_pack(sim, (uint32_t)row); }
__host__ __device__ __forceinline__ float ms_key_sim(uint64_t key) { return as_key_dist(key); }
__host__ __device__ __forceinline__ int32_t ms_key_row(uint64_t key) { return (int32_t)as_key_pos(key); }

// The order of the float64 sum.  A cluster's members are taken in dataset-row order, member p = 0, 1, ...: member p is added to
// chain p mod kMsChains, every chain one member after the other; the kMsChains chain sums are then added one after the other,
// chain 0 first, starting from 0.0.  The order depends on the member's position in its cluster alone: not on the tile, the
// workgroup or the grid a launch happens to use.  (A cluster of up to kMsChains members: the plain sum in row order.)
constexpr int kMsChains = 64;
__host__ __device__ __forceinline__ void ms_chain_add(double& chain, float sim) { chain += (double)sim; }
__host__ __device__ __forceinline__ void ms_total_add(double& total, double chain) { total += chain; }
__host__ __device__ __forceinline__ double ms_mean(double total, int64_t size) { return size > 0 ? total / (double)size : 0.0; }

// the order-free columns of a cluster: minima, maxima and the key minimum
struct MsFold {
    uint64_t key = kMsEmptyKey;
    float pmz_min = INFINITY, pmz_max = -INFINITY, rt_min = INFINITY, rt_max = -INFINITY;
};

__host__ __device__ __forceinline__ void ms_fold_add(MsFold& f, float sim, int32_t row, float pmz, float rt) {
    const uint64_t k = ms_key(sim, row);
    f.key = k < f.key ? k : f.key;
    f.pmz_min = fminf(f.pmz_min, pmz);
    f.pmz_max = fmaxf(f.pmz_max, pmz);
    f.rt_min = fminf(f.rt_min, rt);
    f.rt_max = fmaxf(f.rt_max, rt);
}

__host__ __device__ __forceinline__ void ms_fold_merge(MsFold& f, const MsFold& g) {
    f.key = g.key < f.key ? g.key : f.key;
    f.pmz_min = fminf(f.pmz_min, g.pmz_min);
    f.pmz_max = fmaxf(f.pmz_max, g.pmz_max);
    f.rt_min = fminf(f.rt_min, g.rt_min);
    f.rt_max = fmaxf(f.rt_max, g.rt_max);
}

// one cluster's row of the summary; a cluster without members: zeros, worst_row -1
struct MsRow {
    int32_t size, worst_row;
    float sim_min, pmz_min, pmz_max, rt_min, rt_max;
    double sim_mean;
};

__host__ __device__ __forceinline__ MsRow ms_row(const MsFold& f, double total, int64_t size) {
    MsRow r;
    r.size = (int32_t)size;
    r.sim_mean = ms_mean(total, size);
    if (size > 0) {
        r.worst_row = ms_key_row(f.key);
        r.sim_min = ms_key_sim(f.key);
        r.pmz_min = f.pmz_min;
        r.pmz_max = f.pmz_max;
        r.rt_min = f.rt_min;
        r.rt_max = f.rt_max;
    } else {
        r.worst_row = -1;
        r.sim_min = r.pmz_min = r.pmz_max = r.rt_min = r.rt_max = 0.0f;
    }
    return r;
}

}  // namespace fal
