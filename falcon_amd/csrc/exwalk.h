// What the matched-peak tile kernels share (exact mode, the representative search, the member scores, the network / library
// pair tile): the tile constants, the staging of a tile side's peak lists in LDS, pair_score's window walk with scalar state
// only, the wave-compacted append, the 64-bit wave minimum and, for the host, the error word's message and the settle loop of a
// fallback list.  Included by .hip units only; one copy of each.
#pragma once
#include <algorithm>
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

// minimum of the wave's 64-bit keys, in every lane: the high words first, then the low words of the lanes that hold that minimum
__device__ __forceinline__ uint64_t ex_wave_min_u64(uint64_t key) {
    const uint32_t hi = wave_min_u32((uint32_t)(key >> 32));
    const uint32_t lo = wave_min_u32((uint32_t)(key >> 32) == hi ? (uint32_t)key : 0xFFFFFFFFu);
    return ((uint64_t)hi << 32) | (uint64_t)lo;
}

// ---- the host side: the error word, and the fallback list of a call that settles in one wait ---------------------------------
constexpr int64_t kExFallbackBudget = 1ll << 22;   // fallback pairs the list holds before the host has seen a count (32 MB)

// the error word a solver kernel sets when a component has more than kMaxComp query peaks
inline int ex_check_err(int32_t err, const char* what) {
    FAL_REQUIRE(err == 0, FAL_EUNSUPPORTED, "%s: more than %d peaks of one spectrum chain inside the fragment tolerance", what, kMaxComp);
    return FAL_OK;
}

// The fallback list (in `slot`) of a call that scores at most max_pairs pairs: enqueue(fb, fb_cap) launches the caller's kernels,
// which count the listed pairs in misc[2..3] and set the error word misc[0] (misc: zeroed by the caller).  One wait for both;
// counters[9] = the listed pairs.  More of them than the list held (the count is exact: slots past the end are counted, not
// written): once more with room for all of them -- the same pairs give the same result.
template <class Enqueue>
inline int ex_settle_fallback(fal_ctx* ctx, int slot, int64_t max_pairs, int32_t* misc, const char* what, Enqueue enqueue) {
    hipStream_t st = ctx->stream;
    unsigned long long* d_fb = reinterpret_cast<unsigned long long*>(misc + 2);
    unsigned char* pin = nullptr;
    FAL_TRY(ctx->pinned_reserve(64, (void**)&pin));
    unsigned long long* h = reinterpret_cast<unsigned long long*>(pin);
    int32_t* h_err = reinterpret_cast<int32_t*>(pin + 32);
    int64_t fb_cap = std::max<int64_t>(1, std::min<int64_t>(max_pairs, kExFallbackBudget));
    for (;;) {
        int2* fb = nullptr;
        FAL_TRY(ctx->reserve(slot, sizeof(int2) * (size_t)fb_cap, (void**)&fb));
        FAL_CHECK_HIP(hipMemsetAsync(d_fb, 0, sizeof(unsigned long long), st));
        FAL_TRY(enqueue(fb, fb_cap));
        FAL_CHECK_HIP(hipGetLastError());
        FAL_CHECK_HIP(hipMemcpyAsync(h, d_fb, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipMemcpyAsync(h_err, misc, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        FAL_TRY(ex_check_err(*h_err, what));
        ctx->counters[9] = (int64_t)*h;
        if ((int64_t)*h <= fb_cap) return FAL_OK;
        fb_cap = (int64_t)*h;
        ctx->release(slot);
    }
}

}  // namespace fal
