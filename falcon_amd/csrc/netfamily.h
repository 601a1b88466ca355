// Molecular families: the connected components of the representative network under a size cap (DESIGN.md "Molecular
// families"): the pure core -- which edges are valid, the integer key a similarity is ordered by, when a component is above
// the cap and when an edge of such a component is cut.  Pure functions, shared by families.hip's kernels and the host build of the
// CPU tests (-ffp-contract=off in both; the one sum below is a float64 addition).
//
// The rule.  n nodes, m edges (u, v, sim); every edge starts alive (round 0).  A pass: the components of (nodes, alive edges);
// root(x) = the smallest node of x's component, size(x) = its node count.  With max_size = 0, or no component above the cap, the
// passes end.  Otherwise the pass is a cutting round r = 1, 2, ...: lo(c) = the smallest sim among the alive edges of every
// oversized component c, and an alive edge of c is cut (round[e] = r) when fam_is_cut(sim[e], lo(c), delta); components within
// the cap keep every edge.  Components of two or more nodes are numbered 0, 1, ... by ascending root; a node without a
// surviving edge has family -1 and size 1.
#pragma once
#include <math.h>
#ifdef __HIPCC__
#include "common.h"
#else                        // plain host compiler (the CPU tests' shim): the qualifiers mean nothing there
#include <stdint.h>
#include <string.h>
#ifndef __host__
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#endif

namespace fal {

constexpr uint32_t kFamNoKey = 0xFFFFFFFFu;      // lo of a component before its first edge: above every valid key (a NaN's bits)
constexpr float kFamSimMax = 3.40282347e+38f;   // the largest finite float32

__host__ __device__ __forceinline__ uint32_t fam_bits(float x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(x);
#else
    uint32_t b;
    memcpy(&b, &x, sizeof b);
    return b;
#endif
}
__host__ __device__ __forceinline__ float fam_unbits(uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(b);
#else
    float x;
    memcpy(&x, &b, sizeof x);
    return x;
#endif
}

// an edge the rule accepts: both ends name nodes, no loop, sim finite and >= 0 (a NaN fails both comparisons)
__host__ __device__ __forceinline__ bool fam_valid_edge(int32_t u, int32_t v, float sim, int64_t n) {
    return u >= 0 && v >= 0 && (int64_t)u < n && (int64_t)v < n && u != v && sim >= 0.f && sim <= kFamSimMax;
}

// the key of a valid sim: its bit pattern, which orders like the value (-0 is given +0's key: its own would lie above every other)
__host__ __device__ __forceinline__ uint32_t fam_key(float sim) { return sim == 0.f ? 0u : fam_bits(sim); }
__host__ __device__ __forceinline__ float fam_key_sim(uint32_t key) { return fam_unbits(key); }

// max_size = 0: no cap
__host__ __device__ __forceinline__ bool fam_oversized(int32_t size, int32_t max_size) { return max_size > 0 && size > max_size; }

// an alive edge of an oversized component whose weakest alive edge has key lo_key: one float64 addition, one comparison
__host__ __device__ __forceinline__ bool fam_is_cut(float sim, uint32_t lo_key, double delta) {
    return (double)sim <= (double)fam_key_sim(lo_key) + delta;
}

// a numbered family: two or more nodes
__host__ __device__ __forceinline__ bool fam_is_family(int32_t size) { return size >= 2; }

}  // namespace fal
