// Network of the cluster representatives by greedy modified cosine (DESIGN.md "Representative network"): the pure core -- the
// scope test of a pair of precursors, the two candidate tests of a pair of peaks, the window walk that counts a pair's candidates
// (the cardinality prefilter and the conflict-free case), the decision of a pair, the order of the greedy matching, the clip of
// the score, the edge rule and the key of the mutual top-k ranks.  Pure functions, shared by the kernels of network.hip and
// libsearch.hip (nettile.h) and the host build of the CPU tests (-ffp-contract=off in both: every difference is one float32 subtraction).
#pragma once
#include <math.h>
#ifdef __HIPCC__
#include "common.h"
#else                        // plain host compiler (the CPU tests' shim): the qualifiers mean nothing there
#include <stdint.h>
#ifndef __host__
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#endif

namespace fal {

constexpr int kNetMaxPeaks = 4096;           // peaks of one side of a scored pair (FAL_NET_MAX_PEAKS)

// A pair is named (a, b) with a in front of b in (precursor m/z, node index) order.  In scope: the float32 difference of the
// precursors, compared in float64.  For a fixed a the test is monotone in b's precursor (a float32 subtraction is monotone).
__host__ __device__ __forceinline__ bool net_in_scope(float pmz_a, float pmz_b, double max_shift) {
    return fabs((double)(float)(pmz_b - pmz_a)) <= max_shift;
}

// the shift of the pair's second window: peak i of a meets peak j of b at amz[i] - shift (shift <= 0 in sorted order)
__host__ __device__ __forceinline__ float net_shift(float pmz_a, float pmz_b) { return pmz_a - pmz_b; }

// the two differences of a pair of peaks: float32 subtractions in this order
__host__ __device__ __forceinline__ float net_diff(float amz, float bmz, float shift, bool shifted) {
    return shifted ? (amz - shift) - bmz : amz - bmz;
}
__host__ __device__ __forceinline__ bool net_inside(float d, double tol) { return (double)fabsf(d) <= tol; }

__host__ __device__ __forceinline__ bool net_candidate_mz(float amz, float bmz, float shift, double tol) {
    return net_inside(net_diff(amz, bmz, shift, false), tol) || net_inside(net_diff(amz, bmz, shift, true), tol);
}
// the weight of a candidate: the float32 product; only candidates with w > 0 exist
__host__ __device__ __forceinline__ float net_weight(float ait, float bit) { return ait * bit; }

// ---- the window walk ---------------------------------------------------------------------------------------------------------
// One side's peaks x (ascending) against the other side's y (ascending).  kOverA: x = a's peaks, y = b's: the difference of
// (x[p], y[q]) falls as q grows, a y below the window has d > tol.  Otherwise x = b's peaks, y = a's: the difference of
// (y[q], x[p]) grows with q, a y below the window has -d > tol.  Both windows of x[p] are runs of y, and both ends of both runs
// do not move back as p grows: two moving pointers.  m/z only -- the weights do not enter the counts.
template <bool kOverA>
__host__ __device__ __forceinline__ float net_walk_diff(float xv, float yv, float shift, bool shifted) {
    return kOverA ? net_diff(xv, yv, shift, shifted) : net_diff(yv, xv, shift, shifted);
}
template <bool kOverA>
__host__ __device__ __forceinline__ bool net_walk_below(float d, double tol) {
    return kOverA ? (double)d > tol : (double)(-d) > tol;
}

struct NetWalk {
    int hit = 0;             // peaks of x with a y in one of their windows
    int widest = 0;          // the most y in the union of one x's windows
    double score = 0.0;      // kOverA, meaningful when the pair is conflict-free: the float64 sum, in ascending i, of the weights
    int matched = 0;         //   of the peaks with exactly one y, where that weight is > 0; and their number
};

template <bool kOverA>
__host__ __device__ __forceinline__ NetWalk net_walk(const float* x, const float* xit, int nx, const float* y, const float* yit, int ny,
                                                     float shift, double tol) {
    NetWalk r;
    int lz = 0, ls = 0;
    for (int p = 0; p < nx; ++p) {
        const float xv = x[p];
        while (lz < ny && net_walk_below<kOverA>(net_walk_diff<kOverA>(xv, y[lz], shift, false), tol)) ++lz;
        int hz = lz;
        while (hz < ny && net_inside(net_walk_diff<kOverA>(xv, y[hz], shift, false), tol)) ++hz;
        while (ls < ny && net_walk_below<kOverA>(net_walk_diff<kOverA>(xv, y[ls], shift, true), tol)) ++ls;
        int hs = ls;
        while (hs < ny && net_inside(net_walk_diff<kOverA>(xv, y[hs], shift, true), tol)) ++hs;
        const int lo = lz > ls ? lz : ls, hi = hz < hs ? hz : hs;
        const int u = (hz - lz) + (hs - ls) - (hi > lo ? hi - lo : 0);       // a y inside both windows is one candidate
        if (u > 0) r.hit += 1;
        if (u > r.widest) r.widest = u;
        if (kOverA && u == 1) {
            const float w = net_weight(xit[p], yit[hz > lz ? lz : ls]);
            if (w > 0.f) {
                r.score += (double)w;
                r.matched += 1;
            }
        }
    }
    return r;
}

// [lo, hi) of one window of a's peak (value av, already shifted or not: d = av - y[q]) in b's peaks, by binary search: the
// greedy kernel's form of the same two tests
__host__ __device__ __forceinline__ void net_window(float av, const float* y, int ny, double tol, int* lo_out, int* hi_out) {
    int lo = 0, hi = ny;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)(av - y[mid]) > tol) lo = mid + 1; else hi = mid;
    }
    int e = lo;
    hi = ny;
    while (e < hi) {
        const int mid = (e + hi) >> 1;
        if ((double)(-(av - y[mid])) > tol) hi = mid; else e = mid + 1;
    }
    *lo_out = lo;
    *hi_out = e;
}

// A pair after its two walks.  matched can exceed neither side's hit count, so a pair with fewer than `need` on a side is no edge
// (exact: the counts ignore the weights and only over-count).  A pair none of whose peaks, on either side, has two partners is
// conflict-free: the greedy matching accepts every candidate, the a-walk's sum is the score.  Every other pair is the greedy
// kernel's.
enum { NET_REJECT = 0, NET_INLINE = 1, NET_GREEDY = 2 };
__host__ __device__ __forceinline__ int net_need(int min_matched) { return min_matched > 1 ? min_matched : 1; }
__host__ __device__ __forceinline__ int net_classify(int hit_a, int widest_a, int hit_b, int widest_b, int need) {
    if (hit_a < need || hit_b < need) return NET_REJECT;
    return widest_a <= 1 && widest_b <= 1 ? NET_INLINE : NET_GREEDY;
}

// ---- the greedy matching -----------------------------------------------------------------------------------------------------
// Candidates are taken by (w descending, i ascending, j ascending): true when (w, i, j) comes before (bw, bi, bj).  w > 0, so
// the weights' bits order like the weights.
__host__ __device__ __forceinline__ bool net_before(float w, int i, int j, float bw, int bi, int bj) {
    return w > bw || (w == bw && (i < bi || (i == bi && j < bj)));
}

// the score: the accepted weights added in float64 in ascending i (pair_score's order), from 0.0
__host__ __device__ __forceinline__ void net_sum_add(double& score, float w) { score += (double)w; }
__host__ __device__ __forceinline__ float net_similarity(double score) { return (float)fmax(0.0, fmin(score, 1.0)); }

// a scored pair is an edge with at least min_matched (and at least one) accepted candidates and sim >= float32(min_cosine)
__host__ __device__ __forceinline__ bool net_is_edge(float sim, int matched, double min_cosine, int min_matched) {
    return matched >= net_need(min_matched) && sim >= (float)min_cosine;
}

// ---- the decision of one pair ------------------------------------------------------------------------------------------------
// One side of a pair: its peaks, their number, its precursor.  A pair in its orientation: a is the side with the lower precursor
// (the network's sorted order as it stands; libsearch.h's lib_orient turns a (query, library) pair into it).
struct NetRow { const float *mz, *it; int len; float pmz; };
struct NetOriented { NetRow a, b; float shift; };
__host__ __device__ __forceinline__ NetOriented net_orient(const NetRow& a, const NetRow& b) {
    return NetOriented{a, b, net_shift(a.pmz, b.pmz)};
}

// The one copy of the sequence: the walk over a's peaks, the walk over b's only when a's leaves enough peaks with a partner, the
// classification; sim and matched are the conflict-free pair's (NET_INLINE), 0 otherwise.
struct NetPair { int kind; float sim; int matched; };
__host__ __device__ __forceinline__ NetPair net_pair(const NetOriented& o, double tol, int need) {
    const NetWalk wa = net_walk<true>(o.a.mz, o.a.it, o.a.len, o.b.mz, o.b.it, o.b.len, o.shift, tol);
    if (wa.hit < need) return NetPair{NET_REJECT, 0.f, 0};
    const NetWalk wb = net_walk<false>(o.b.mz, o.b.it, o.b.len, o.a.mz, o.a.it, o.a.len, o.shift, tol);
    const int kind = net_classify(wa.hit, wa.widest, wb.hit, wb.widest, need);
    if (kind != NET_INLINE) return NetPair{kind, 0.f, 0};
    return NetPair{NET_INLINE, net_similarity(wa.score), wa.matched};
}

// ---- mutual top-k --------------------------------------------------------------------------------------------------------------
// A node's incident edges are ranked by (sim descending, other node ascending): the key orders (node, sim descending); entries
// of equal key are given to the stable sort in ascending order of the other node.  sim is in [0, 1]: its bits order as unsigned.
__host__ __device__ __forceinline__ uint64_t net_rank_key(int32_t node, float sim) {
    union { float f; uint32_t u; } v;
    v.f = sim;
    return ((uint64_t)(uint32_t)node << 32) | (uint64_t)(~v.u);
}

}  // namespace fal
