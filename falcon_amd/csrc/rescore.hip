// f4: exact re-scoring of the ANN neighbour lists with the matched-peak cosine the reference snapshot
// ships (similarity.py:17-80 `cosine_fast`; its use cluster.py:593-639: dist = 1 - sim, sim = 0 when
// fewer than min_matches peaks match).
//
// One lane per stored (query, neighbour) pair; the pair scorer (components, Hungarian fallback, the reference's
// window arithmetic) is peakmatch.h's, shared with exact mode.  Latency/L2-bound gather work (peaks of a bucket's
// spectra are shared by its rows).
#include <math.h>
#include <algorithm>
#include "common.h"
#include "ivf.h"
#include "peakmatch.h"

namespace fal {

__global__ __launch_bounds__(256) void rescore_kernel(const int32_t* __restrict__ nb_idx, float* __restrict__ nb_dist, int64_t n,
                                                      int k, const float* __restrict__ mz, const float* __restrict__ intensity,
                                                      const int64_t* __restrict__ indptr, const int64_t* __restrict__ order,
                                                      double tol, int min_matches, int32_t* __restrict__ err) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n * k; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t j = nb_idx[t];
        if (j < 0) continue;
        const int64_t a = order[t / k], b = order[j];
        const int64_t a0 = indptr[a], b0 = indptr[b];
        const int na = (int)(indptr[a + 1] - a0), nb = (int)(indptr[b + 1] - b0);
        PeakLists s{mz + a0, intensity + a0, mz + b0, intensity + b0};
        double score = 0.0;
        int n_match = 0;
        const bool ok = pair_score(s, na, nb, tol, &score, &n_match);
        if (!ok) atomicExch(err, 1);
        double sim = fmax(0.0, fmin(score, 1.0));                            // similarity.py:78
        if (n_match < min_matches) sim = 0.0;                                // cluster.py:624-626
        nb_dist[t] = (float)(1.0 - sim);
    }
}

}  // namespace fal
FAL_WARM_KERNEL(fal::rescore_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_rescore_neighbors(fal_ctx* ctx, const int32_t* nb_idx, float* nb_dist, int64_t n, int k, const float* mz,
                                     const float* intensity, const int64_t* indptr, const int64_t* row_order,
                                     double fragment_tol, int min_matches) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && k >= 1 && fragment_tol >= 0.0, FAL_EINVAL, "fal_rescore_neighbors: bad argument");
    if (n == 0) return FAL_OK;
    FAL_REQUIRE(nb_idx && nb_dist && indptr && row_order, FAL_EINVAL, "fal_rescore_neighbors: NULL array");
    int32_t* err = nullptr;
    FAL_TRY(ctx->reserve(SLOT_MISC2, sizeof(int32_t), (void**)&err));
    FAL_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int32_t), ctx->stream));
    ctx->stage_reset(ST_FILTER);
    {
        StageScope ts(ctx, ST_FILTER);
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n * k, 256), (int64_t)ctx->num_cus * 32);
        hipLaunchKernelGGL(rescore_kernel, dim3(grid), dim3(256), 0, ctx->stream, nb_idx, nb_dist, n, k, mz, intensity, indptr,
                           row_order, fragment_tol, min_matches, err);
        FAL_CHECK_HIP(hipGetLastError());
    }
    int32_t h = 0;
    FAL_CHECK_HIP(hipMemcpyAsync(&h, err, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    FAL_REQUIRE(h == 0, FAL_EUNSUPPORTED,
                "fal_rescore_neighbors: more than %d peaks of one spectrum chain inside the fragment tolerance", kMaxComp);
    return FAL_OK;
}
