// The per-spectrum peak sort of the peak-file readers (peakdecode.hip, mgfparse.hip): one wave sorts one spectrum by m/z,
// stable -- what np.lexsort((mz, row)) does in falcon._raw_csr: NaN last, ties in input order.  Already-sorted spectra (nearly
// all) are copied, the rest ranked within the wave.
#pragma once
#include <math.h>
#include "common.h"

namespace fal {

// np.sort order on float64: NaN after every number, NaNs equal among themselves, -0.0 == 0.0
__device__ __forceinline__ bool peak_key_less(double a, double b) { return a < b || (isnan(b) && !isnan(a)); }

// mz_at(j) -> double, it_at(j) -> float for j in [0, n): the spectrum's peaks in input order; out_mz / out_it: its n output peaks.
// Called by all 64 lanes of a wave with the same n.
template <class MzAt, class ItAt>
__device__ __forceinline__ void wave_sort_peaks(int64_t n, int lane, const MzAt& mz_at, const ItAt& it_at, double* __restrict__ out_mz,
                                                float* __restrict__ out_it) {
    bool unsorted = false;
    for (int64_t j = 1 + lane; j < n; j += 64) unsorted |= peak_key_less(mz_at(j), mz_at(j - 1));
    if (__ballot(unsorted) == 0) {
        for (int64_t j = lane; j < n; j += 64) {
            out_mz[j] = mz_at(j);
            out_it[j] = it_at(j);
        }
    } else {
        // stable rank: peaks with a smaller key, plus equal keys earlier in the array
        for (int64_t j = lane; j < n; j += 64) {
            const double kj = mz_at(j);
            int64_t r = 0;
            for (int64_t k = 0; k < n; ++k) {
                const double kk = mz_at(k);
                r += peak_key_less(kk, kj) || (k < j && !peak_key_less(kj, kk));
            }
            out_mz[r] = kj;
            out_it[r] = it_at(j);
        }
    }
}

}  // namespace fal
