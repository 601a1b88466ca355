// Library search of the cluster representatives by greedy (modified) cosine (DESIGN.md "Library search"): the pure core -- the
// scope test of a (query, library) pair of precursors in its two modes, the library range that holds every pair in scope of a
// run of queries (a pre-filter: the per-pair test decides), the orientation of a pair (netmatch.h names the side with the lower
// precursor a) and its shift.  Everything behind the orientation -- candidates, walks, greedy order, sum, hit rule, rank key --
// is netmatch.h's, unchanged.  Pure functions, shared by libsearch.hip's kernels and the host build of the CPU tests
// (-ffp-contract=off in both).
#pragma once
#include "assignrep.h"
#include "netmatch.h"

namespace fal {

// exact mode: the precursor test of fal_assign_nearest without a retention-time rule; analog mode: the network's scope
__host__ __device__ __forceinline__ bool lib_in_scope(float pq, float pl, int analog, double precursor_tol, int tol_is_da,
                                                      double max_shift) {
    return analog ? net_in_scope(pq, pl, max_shift) : as_candidate(pq, pl, precursor_tol, tol_is_da, false, 0.f, 0.f, -1.0);
}

// Library precursors outside [*lo, *hi] are in scope of no query with q_min <= precursor <= q_max; false = no such range (the
// whole library).  Analog mode: |float32(pl - pq)| <= max_shift holds only where |pl - pq| <= max_shift / (1 - 2^-24), inside
// as_window's Da range (10^-5 of the tolerance wider than the real-number rule).
__host__ __device__ __forceinline__ bool lib_window(float q_min, float q_max, int analog, double precursor_tol, int tol_is_da,
                                                    double max_shift, double* lo, double* hi) {
    return analog ? as_window(q_min, q_max, max_shift, 1, lo, hi) : as_window(q_min, q_max, precursor_tol, tol_is_da, lo, hi);
}

// the pair's a is the side with the lower float32 precursor; with equal precursors the query
__host__ __device__ __forceinline__ bool lib_query_is_a(float pq, float pl) { return pq <= pl; }

// exact mode: no second window (with shift 0 both windows coincide and net_walk counts a peak of both once: the plain greedy
// cosine)
__host__ __device__ __forceinline__ float lib_shift(int analog, float pmz_a, float pmz_b) {
    return analog ? net_shift(pmz_a, pmz_b) : 0.0f;
}

// the orientation of a (query, library) pair: a swap of the sides, and the shift in that order
__host__ __device__ __forceinline__ NetOriented lib_orient(int analog, const NetRow& q, const NetRow& l) {
    const bool qa = lib_query_is_a(q.pmz, l.pmz);
    const NetRow &a = qa ? q : l, &b = qa ? l : q;
    return NetOriented{a, b, lib_shift(analog, a.pmz, b.pmz)};
}

}  // namespace fal
