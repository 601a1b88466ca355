// The greedy matching of one listed pair by one wave (netmatch.h's order), shared by network.hip's net_greedy_kernel and
// libsearch.hip's lib_greedy_kernel: one copy of the rounds.  Device code.
//
// Peak i of a belongs to lane i mod 64 (strip i / 64).  s_j[i]: the best free partner the peak last found (>= 0), kNetStale
// before the first look, kNetNone when no free partner is left (none comes back: the used peaks only grow), kNetTaken once the
// peak is accepted -- s_w[i] is its weight then.  A round: every lane brings its peaks' offers up to date (an offer stands until
// its partner is used) and keeps the first in the order; the wave takes the largest weight, among equals the lowest i (its j is
// the lowest of that weight: the look goes through b in ascending order).
#pragma once
#include "common.h"
#include "netmatch.h"

namespace fal {

constexpr int kNetStale = -2, kNetNone = -1, kNetTaken = -3;

// a's peaks (the side with the lower precursor: shift <= 0) against b's; s_w, s_j: kCap entries, s_used: kCap / 32 words of the
// calling wave.  false = a side above kCap (nothing done).  *matched_out in every lane, *sim_out in lane 0 only.  The caller
// puts a wave_lds_sync() behind its use of the result, before the next pair's state goes over this one's.
template <int kCap>
__device__ __forceinline__ bool net_greedy_pair(const float* __restrict__ amz, const float* __restrict__ ait, int la,
                                                const float* __restrict__ bmz, const float* __restrict__ bit, int lb, float shift,
                                                double tol, float* s_w, int* s_j, uint32_t* s_used, float* sim_out, int* matched_out) {
    if (la > kCap || lb > kCap) return false;
    const int lane = threadIdx.x;
    for (int i = lane; i < la; i += 64) s_j[i] = kNetStale;
    for (int q = lane; q < (lb + 31) / 32; q += 64) s_used[q] = 0u;
    wave_lds_sync();
    int matched = 0;
    for (;;) {
        float bw = 0.f;
        int bi = 0x7FFFFFFF, bj = -1;
        for (int i = lane; i < la; i += 64) {
            int cj = s_j[i];
            if (cj == kNetNone || cj == kNetTaken) continue;
            float w = 0.f;
            if (cj >= 0 && !((s_used[cj >> 5] >> (cj & 31)) & 1u)) {
                w = s_w[i];
            } else {                                                      // look again: the free b peaks of both windows
                const float av = amz[i], ai = ait[i];
                int z0, z1, s0, s1;
                net_window(av, bmz, lb, tol, &z0, &z1);
                net_window(av - shift, bmz, lb, tol, &s0, &s1);           // (shift <= 0: this window is not below the other)
                cj = kNetNone;
                for (int q = z0; q < z1; ++q) {
                    if ((s_used[q >> 5] >> (q & 31)) & 1u) continue;
                    const float wq = net_weight(ai, bit[q]);
                    if (wq > w) w = wq, cj = q;
                }
                for (int q = max(s0, z1); q < s1; ++q) {
                    if ((s_used[q >> 5] >> (q & 31)) & 1u) continue;
                    const float wq = net_weight(ai, bit[q]);
                    if (wq > w) w = wq, cj = q;
                }
                s_j[i] = cj;
                s_w[i] = w;
            }
            if (cj >= 0 && w > bw) bw = w, bi = i, bj = cj;               // (ascending i: the first of equal weights stays)
        }
        const uint32_t top = wave_max_u32(__float_as_uint(bw));           // (weights > 0: the bits order like the values)
        if (top == 0u) break;
        const uint32_t win = wave_min_u32(__float_as_uint(bw) == top ? (uint32_t)bi : 0xFFFFFFFFu);
        const int j = __shfl(bj, (int)(win & 63u), 64);
        if (lane == (int)(win & 63u)) {
            s_j[win] = kNetTaken;
            s_used[j >> 5] |= 1u << (j & 31);
        }
        matched += 1;
        wave_lds_sync();
    }
    if (lane == 0) {
        double score = 0.0;
        for (int i = 0; i < la; ++i)
            if (s_j[i] == kNetTaken) net_sum_add(score, s_w[i]);
        *sim_out = net_similarity(score);
    }
    *matched_out = matched;
    return true;
}

}  // namespace fal
