// Nearest representative of a new spectrum (DESIGN.md "Assigning to representatives"): the pure core -- the per-pair
// precursor / retention-time test (the neighbour filter's, graph.hip filter_kernel, with the new spectrum in the query role),
// the precursor range that holds every candidate of a run of queries (a pre-filter: the per-pair test decides), and the 64-bit
// key whose minimum is the result.  Pure functions, shared by assignrep.hip's kernels and the host build of the CPU tests
// (-ffp-contract=off in both).
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

// mass_diff(query, library) against the tolerance: the difference and the division are float32, the product with 10^6 is
// float64 (cluster.py:190-195); the retention times differ in float32.  rt_tol < 0 (or has_rt false): no RT rule.
__host__ __device__ __forceinline__ bool as_candidate(float q_pmz, float l_pmz, double tol, int tol_is_da, bool has_rt, float q_rt,
                                                      float l_rt, double rt_tol) {
    const float diff = q_pmz - l_pmz;
    const double md = tol_is_da ? (double)diff : (double)(diff / l_pmz) * 1e6;
    bool ok = fabs(md) <= tol;
    if (ok && has_rt && rt_tol >= 0.0) ok = fabs((double)(q_rt - l_rt)) <= rt_tol;
    return ok;
}

// Library precursors outside [*lo, *hi] are no candidate of any query with q_min <= precursor <= q_max.  The float32 roundings
// of the rule move a pair's bound by parts in 10^7; the range is 10^-5 of the tolerance wider than the real-number rule.
// false = no such range (ppm of a library precursor <= 0 or a tolerance of 10^6 ppm and more): the whole library.
__host__ __device__ __forceinline__ bool as_window(float q_min, float q_max, double tol, int tol_is_da, double* lo, double* hi) {
    if (tol_is_da) {
        const double w = tol * (1.0 + 1e-5);
        *lo = (double)q_min - w;
        *hi = (double)q_max + w;
        return true;
    }
    const double r = tol * 1e-6 * (1.0 + 1e-5);                  // |q - l| <= r |l|
    if (!(r < 1.0) || !(q_min > 0.f)) return false;
    *lo = (double)q_min / (1.0 + r) * (1.0 - 1e-9);
    *hi = (double)q_max / (1.0 - r) * (1.0 + 1e-9);
    return true;
}

// key = (bits of the float32 distance) << 32 | rank of the library row in (precursor m/z, row) order.  d >= 0: its bits order
// as an unsigned integer, so the smallest key is the smallest distance, then the lowest precursor, then the lowest row.
constexpr uint64_t kAsEmptyKey = ~0ull;      // no candidate yet: above every real key (d <= 1 = 0x3F800000)

__host__ __device__ __forceinline__ uint64_t as_pack(float d, uint32_t pos) {
    union { float f; uint32_t u; } v;
    v.f = d == 0.0f ? 0.0f : d;              // (-0 = +0)
    return ((uint64_t)v.u << 32) | (uint64_t)pos;
}

__host__ __device__ __forceinline__ float as_key_dist(uint64_t key) {
    union { float f; uint32_t u; } v;
    v.u = (uint32_t)(key >> 32);
    return v.f;
}

__host__ __device__ __forceinline__ uint32_t as_key_pos(uint64_t key) { return (uint32_t)key; }

}  // namespace fal
