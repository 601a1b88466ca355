// Consensus spectrum of a cluster (DESIGN.md "Consensus representatives"): the pure arithmetic -- pooled order key, group
// boundary, quorum, group values, normalisation.  Every sum is a float64 chain in POOLED ORDER (m/z ascending, then dataset
// row, then peak index), one peak after the other, whatever the size of the cluster: there is one summation order.  Pure
// functions, shared by consensus.hip's kernels and the host build of the CPU tests (-ffp-contract=off in both).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/falcon_hip.h"
#ifndef __HIPCC__            // plain host compiler (the CPU tests' shim): the qualifiers mean nothing there
#ifndef __host__
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#endif

namespace fal {

// pooled peaks of a cluster that are sorted inside one workgroup's LDS (8-byte keys: 32 KiB per workgroup, five workgroups
// per 160 KiB CU); a larger cluster goes through the device-wide radix sort
constexpr int kConsLdsPeaks = FAL_CONS_LDS_PEAKS;

// m/z -> unsigned key with the order of the float compare (-0 = +0; NaN is outside the contract)
__host__ __device__ __forceinline__ uint32_t cons_mz_key(float mz) {
    if (mz == 0.0f) mz = 0.0f;
    union { float f; uint32_t u; } v;
    v.f = mz;
    return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}

// a new group starts at a pooled peak whose m/z lies more than the tolerance above its predecessor's (gap rule: peaks chain)
__host__ __device__ __forceinline__ bool cons_new_group(float mz, float mz_prev, double fragment_tol) {
    return (double)mz - (double)mz_prev > fragment_tol;
}

// peaks a group needs to be kept in a cluster of m members: max(1, ceil(q m))
__host__ __device__ __forceinline__ int64_t cons_need(double min_fraction, int64_t m) {
    const int64_t need = (int64_t)ceil(min_fraction * (double)m);
    return need < 1 ? 1 : need;
}

struct ConsGroup {
    double w = 0.0;          // sum of intensity
    double mw = 0.0;         // sum of m/z * intensity
    double ms = 0.0;         // sum of m/z (the m/z of a group without intensity)
    int64_t count = 0;
};

__host__ __device__ __forceinline__ void cons_group_add(ConsGroup& g, float mz, float intensity) {
    g.w += (double)intensity;
    g.mw += (double)mz * (double)intensity;
    g.ms += (double)mz;
    g.count += 1;
}

// support counts peaks, not distinct members: min(peaks of the group, m)
__host__ __device__ __forceinline__ bool cons_group_kept(const ConsGroup& g, int64_t m, int64_t need) {
    return (g.count < m ? g.count : m) >= need;
}

__host__ __device__ __forceinline__ float cons_group_mz(const ConsGroup& g) {
    return g.w == 0.0 ? (float)(g.ms / (double)g.count) : (float)(g.mw / g.w);
}

// mean intensity over ALL members (a member without a peak in the group counts as 0)
__host__ __device__ __forceinline__ double cons_group_raw(const ConsGroup& g, int64_t m) { return g.w / (double)m; }

__host__ __device__ __forceinline__ void cons_norm_add(double& norm2, double raw) { norm2 += raw * raw; }

__host__ __device__ __forceinline__ float cons_intensity(double raw, double norm2) {
    return norm2 == 0.0 ? 0.0f : (float)(raw / sqrt(norm2));
}

}  // namespace fal
