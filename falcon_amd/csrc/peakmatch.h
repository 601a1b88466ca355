// Matched-peak cosine of one spectrum pair -- the reference snapshot's `cosine_fast` (similarity.py:17-80), shared by
// the re-scoring of the ANN neighbours (rescore.hip) and exact mode (exact.hip).
//
// The reference fills a dense cost matrix and calls scipy's linear_sum_assignment on it; here the same optimum is reached
// without the matrix: both peak lists are sorted, so the pairs inside the fragment tolerance form runs ("components":
// consecutive query peaks whose windows chain through shared neighbour peaks) and the assignment decomposes into one small
// problem per component -- almost always 1x1, solved in place; the general case runs the Hungarian algorithm on the
// component (<= kMaxComp peaks a side, per-lane scratch).  Window arithmetic is the reference's: `peak_mz - tol` in float64,
// `abs(peak_mz - other_mz)` in float32 against the float64 tolerance; pair costs are float32 products; the positive pair
// scores are summed in query-peak order in float64.
//
// Pure functions, compiled for both sides: tests/test_peakmatch_cpu.py builds this header with the host compiler and checks
// it against the oracle's `cosine_fast`.
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

constexpr int kMaxComp = 32;

struct PeakLists {
    const float* amz;
    const float* ait;
    const float* bmz;
    const float* bit;
};

__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }     // (HIP's own max is device-only)

// weight of (component row r, column q): the float32 product inside the row's window, else 0
__host__ __device__ __forceinline__ float comp_w(const PeakLists& s, const int* rp, const int* rs, const int* re, int r, int q) {
    return (q >= rs[r] && q < re[r]) ? s.ait[rp[r]] * s.bit[q] : 0.f;
}

// maximum-weight assignment of one component (rows = query peaks rp[0..nr), columns [qs, qe)); adds the
// positive pair scores in row order.  Returns false when the component is larger than kMaxComp.
__host__ __device__ inline bool solve_component(const PeakLists& s, const int* rp, const int* rs, const int* re, int nr, int qs,
                                                int qe, double* score, int* n_match) {
    const int nc = qe - qs;
    if (nr == 1) {                                    // one query peak: its best partner
        float best = 0.f;
        for (int q = rs[0]; q < re[0]; ++q) best = fmaxf(best, s.ait[rp[0]] * s.bit[q]);
        if (best > 0.f) {
            *score += (double)best;
            *n_match += 1;
        }
        return true;
    }
    if (nr > kMaxComp || nc > kMaxComp) return false;
    // Hungarian algorithm (potentials, O(n^2 m)), minimising -w; n = the smaller side
    const bool tr = nr > nc;                          // transposed: "rows" of the solver are the columns
    const int n = tr ? nc : nr, m = tr ? nr : nc;
    double u[kMaxComp + 1], v[kMaxComp + 1], minv[kMaxComp + 1];
    int p[kMaxComp + 1], way[kMaxComp + 1];
    bool used[kMaxComp + 1];
    for (int j = 0; j <= m; ++j) {
        v[j] = 0.0;
        p[j] = 0;
    }
    for (int i = 0; i <= n; ++i) u[i] = 0.0;
    auto cost = [&](int i, int j) -> double {         // 1-based solver indices
        const int r = tr ? j - 1 : i - 1, q = qs + (tr ? i - 1 : j - 1);
        return -(double)comp_w(s, rp, rs, re, r, q);
    };
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        for (int j = 0; j <= m; ++j) {
            minv[j] = INFINITY;
            used[j] = false;
        }
        do {
            used[j0] = true;
            const int i0 = p[j0];
            double delta = INFINITY;
            int j1 = 0;
            for (int j = 1; j <= m; ++j) {
                if (!used[j]) {
                    const double cur = cost(i0, j) - u[i0] - v[j];
                    if (cur < minv[j]) {
                        minv[j] = cur;
                        way[j] = j0;
                    }
                    if (minv[j] < delta) {
                        delta = minv[j];
                        j1 = j;
                    }
                }
            }
            for (int j = 0; j <= m; ++j) {
                if (used[j]) {
                    u[p[j]] += delta;
                    v[j] -= delta;
                } else {
                    minv[j] -= delta;
                }
            }
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }
    // p[j] = solver row assigned to solver column j.  Sum in query-peak (component row) order.
    if (!tr) {
        int col_of[kMaxComp];
        for (int r = 0; r < nr; ++r) col_of[r] = -1;
        for (int j = 1; j <= m; ++j)
            if (p[j] != 0) col_of[p[j] - 1] = qs + j - 1;
        for (int r = 0; r < nr; ++r) {
            const float w = col_of[r] >= 0 ? comp_w(s, rp, rs, re, r, col_of[r]) : 0.f;
            if (w > 0.f) {
                *score += (double)w;
                *n_match += 1;
            }
        }
    } else {
        for (int j = 1; j <= m; ++j) {                // solver column j = component row j - 1
            const float w = p[j] != 0 ? comp_w(s, rp, rs, re, j - 1, qs + p[j] - 1) : 0.f;
            if (w > 0.f) {
                *score += (double)w;
                *n_match += 1;
            }
        }
    }
    return true;
}

// The whole pair: score (before clipping) and matched peaks.  Returns false when a component is larger than kMaxComp.
__host__ __device__ inline bool pair_score(const PeakLists& s, int na, int nb, double tol, double* score_out, int* n_match_out) {
    double score = 0.0;
    int n_match = 0;
    bool ok = true;
    if (na > 0 && nb > 0) {
        int rp[kMaxComp], rs[kMaxComp], re[kMaxComp];
        int nr = 0, qs = 0, qe = 0, o = 0;
        for (int p = 0; p < na; ++p) {                                   // similarity.py:45-63
            const float pm = s.amz[p];
            while (o < nb - 1 && (double)pm - tol > (double)s.bmz[o]) ++o;
            int q = o;
            while (q < nb && (double)fabsf(pm - s.bmz[q]) <= tol) ++q;
            if (q == o) continue;                                        // nothing inside this peak's window
            if (nr > 0 && o >= qe) {                                     // window starts past the component: close it
                ok = solve_component(s, rp, rs, re, nr, qs, qe, &score, &n_match) && ok;
                nr = 0;
            }
            if (nr == 0) qs = o;
            if (nr < kMaxComp) {
                rp[nr] = p;
                rs[nr] = o;
                re[nr] = q;
            }
            ++nr;
            qe = nr == 1 ? q : imax(qe, q);
        }
        if (nr > 0) ok = solve_component(s, rp, rs, re, nr, qs, qe, &score, &n_match) && ok;
    }
    *score_out = score;
    *n_match_out = n_match;
    return ok;
}

// cosine distance of a scored pair: 1 - sim, sim clipped to [0, 1] (similarity.py:78) and 0 below min_matches (cluster.py:624-626)
__host__ __device__ __forceinline__ double pair_distance(double score, int n_match, int min_matches) {
    double sim = fmax(0.0, fmin(score, 1.0));
    if (n_match < min_matches) sim = 0.0;
    return 1.0 - sim;
}

// The peak lists of a pass in sorted-row space: row i is dataset row order[i], its peaks mz / it[indptr[order[i]] ..).
struct ExactPeaks {
    const float* mz;
    const float* it;
    const int64_t* indptr;
    const int64_t* order;
    double tol;
    int min_matches;
    int32_t* err;           // set to 1 when a pair has a component of more than kMaxComp peaks
};

// the reference's pair distance of sorted rows i < j (i is the query spectrum, cluster.py:593-639); *ok cleared when a
// component is larger than kMaxComp
__host__ __device__ inline double exact_distance(const ExactPeaks& pk, int64_t i, int64_t j, bool* ok) {
    const int64_t a = pk.order[i], b = pk.order[j];
    const int64_t a0 = pk.indptr[a], b0 = pk.indptr[b];
    const PeakLists s{pk.mz + a0, pk.it + a0, pk.mz + b0, pk.it + b0};
    double score = 0.0;
    int n_match = 0;
    if (!pair_score(s, (int)(pk.indptr[a + 1] - a0), (int)(pk.indptr[b + 1] - b0), pk.tol, &score, &n_match)) *ok = false;
    return pair_distance(score, n_match, pk.min_matches);
}

}  // namespace fal
