// The pair walk exact mode and the representative search share: the tile constants, the staging of a tile side's peak lists in
// LDS, pair_score's window walk with scalar state only, and the wave-compacted append.  Device code; one copy of the walk.
#pragma once
#include "common.h"
#include "peakmatch.h"

namespace fal {

constexpr int kExTile = 64;                  // rows of a tile side
constexpr int kExLdsPeaks = 3200;            // staged peaks per side (64 rows x 50 peaks): 2 sides x 3,200 x 8 B = 51 KB of LDS,
                                             // three workgroups per CU; a side with more peaks is read from global memory

// one 1 x 1 component: the query peak's best partner (solve_component's nr == 1 branch)
__device__ __forceinline__ void ex_close_1x1(const PeakLists& s, int r, int q0, int q1, double* score, int* n_match) {
    float best = 0.f;
    for (int q = q0; q < q1; ++q) best = fmaxf(best, s.ait[r] * s.bit[q]);
    if (best > 0.f) {
        *score += (double)best;
        *n_match += 1;
    }
}

// pair_score's walk with scalar state only: false = a component of two or more query peaks (the fallback list's)
__device__ __forceinline__ bool ex_score_simple(const PeakLists& s, int na, int nb, double tol, double* score_out, int* n_match_out) {
    double score = 0.0;
    int n_match = 0;
    if (na > 0 && nb > 0) {
        int nr = 0, qe = 0, o = 0, r0 = 0, rs0 = 0, re0 = 0;
        for (int p = 0; p < na; ++p) {                                   // similarity.py:45-63
            const float pm = s.amz[p];
            while (o < nb - 1 && (double)pm - tol > (double)s.bmz[o]) ++o;
            int q = o;
            while (q < nb && (double)fabsf(pm - s.bmz[q]) <= tol) ++q;
            if (q == o) continue;
            if (nr > 0 && o >= qe) {                                     // the open component closes as 1 x 1
                ex_close_1x1(s, r0, rs0, re0, &score, &n_match);
                nr = 0;
            }
            if (nr > 0) return false;                                    // a second query peak joins it
            r0 = p;
            rs0 = o;
            re0 = q;
            nr = 1;
            qe = q;
        }
        if (nr > 0) ex_close_1x1(s, r0, rs0, re0, &score, &n_match);
    }
    *score_out = score;
    *n_match_out = n_match;
    return true;
}

// append the wave's flagged pairs (one atomic per wave); slot >= cap is counted but not written
__device__ __forceinline__ unsigned long long ex_wave_slot(bool flag, unsigned long long* counter) {
    const unsigned long long mask = __ballot(flag);
    if (mask == 0) return ~0ull;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader, 64);
    return base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
}

// stage the peaks of rows r0 .. r0 + nr (sorted rows) into LDS when they fit; per row its offset (LDS or global)
__device__ __forceinline__ bool ex_stage(const ExactPeaks& pk, int32_t r0, int nr, float* lmz, float* lit, int64_t* off, int* len,
                                         int* tot) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        int l = 0;
        int64_t g = 0;
        if (tid < nr) {
            const int64_t a = pk.order[r0 + tid];
            g = pk.indptr[a];
            l = (int)(pk.indptr[a + 1] - g);
        }
        const int incl = wave_prefix_sum(l);
        off[tid] = g;                                            // global offset for now
        len[tid] = l;
        if (tid == 63) *tot = incl;
        len[64 + tid] = incl - l;                                // exclusive prefix: the LDS offset
    }
    __syncthreads();
    const bool fits = *tot <= kExLdsPeaks;
    if (fits) {
        for (int r = 0; r < nr; ++r) {
            const int64_t g = off[r];
            const int l = len[r], lo = len[64 + r];
            for (int x = tid; x < l; x += blockDim.x) {
                lmz[lo + x] = pk.mz[g + x];
                lit[lo + x] = pk.it[g + x];
            }
        }
    }
    __syncthreads();
    return fits;
}

}  // namespace fal
