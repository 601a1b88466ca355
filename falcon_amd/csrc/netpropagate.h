// Annotation propagation through the molecular families (DESIGN.md "Annotation propagation"): the pure core -- which links, seeds
// and options are valid, the score a link offers, when it counts, and the integer key the best offer is chosen by.  Pure
// functions, shared by propagate.hip's kernels and the host build of the CPU tests (-ffp-contract=off in both; the one product
// below is a float32 multiplication).
//
// The rule.  n nodes, m undirected links (u, v, sim), seed[n] (>= 0: annotated, -1: not).  Level 0: every annotated node has hops
// 0, source itself, parent -1, score 1.  Level d = 1 .. max_hops in this order: a link {a, b} with hops[a] == d - 1 and b not yet
// reached offers b the candidate (a, c = score[a] * sim); it counts when c >= (float)min_score; a node with a counting candidate
// takes the greatest c, equal c the lowest a: hops d, parent a, source source[a], score c.  A node reached at level d is no parent
// within level d.  A node never reached: source, hops, parent -1, score 0.
#pragma once
#include "netfamily.h"

namespace fal {

constexpr int kPropMaxHops = 64;

// the links are the families' links: both ends name nodes, no loop, sim finite and >= 0
__host__ __device__ __forceinline__ bool prop_valid_edge(int32_t u, int32_t v, float sim, int64_t n) { return fam_valid_edge(u, v, sim, n); }
__host__ __device__ __forceinline__ bool prop_valid_seed(int32_t seed) { return seed >= -1; }
__host__ __device__ __forceinline__ bool prop_valid_hops(int max_hops) { return max_hops >= 1 && max_hops <= kPropMaxHops; }
// (a NaN fails both comparisons)
__host__ __device__ __forceinline__ bool prop_valid_min_score(double min_score) { return min_score >= 0.0 && min_score <= 1.0; }

// what parent a (score score_a) offers across a link of similarity sim: one float32 product.  Not clamped: above 1 with a sim
// above 1, infinite when it overflows, NaN from infinity times 0 (which never counts)
__host__ __device__ __forceinline__ float prop_candidate(float score_a, float sim) { return score_a * sim; }

__host__ __device__ __forceinline__ bool prop_counts(float c, double min_score) { return c >= (float)min_score; }

// the key of a counting candidate, for one unsigned 64-bit maximum per candidate: c's bits above (they order like the value for
// c >= 0; a zero of either sign has +0's), 0xFFFFFFFF - a below, so that of equal c the lowest parent wins.  Never 0: a < 2^31
// leaves the low word at 2^31 or above -- 0 is the key of a node without a candidate
__host__ __device__ __forceinline__ unsigned long long prop_key(float c, int32_t a) {
    return ((unsigned long long)fam_key(c) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)a);
}
__host__ __device__ __forceinline__ float prop_key_score(unsigned long long key) { return fam_unbits((uint32_t)(key >> 32)); }
__host__ __device__ __forceinline__ int32_t prop_key_parent(unsigned long long key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)key); }

}  // namespace fal
