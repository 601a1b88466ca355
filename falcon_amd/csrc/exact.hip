// Exact mode: the snapshot's own clustering at scale -- the matched-peak cosine of EVERY pair of a precursor block
// (reference cluster.py:212-331 + 593-639: `compute_condensed_distance_matrix`, then
// `fcluster(linkage(pdist, linkage), distance_threshold, "distance")`, refinement, medoids over the full matrix).
//
// Blocks are the bucket table of the pass.  The upper triangle of every bucket is cut into 64 x 64 tiles, enumerated on the host
// into one flat launch; a workgroup stages both tiles' peak lists in LDS and every lane scores one pair at a time with the
// window walk of peakmatch.h.  1 x 1 components (nearly all) are solved inline -- the hot loop holds no per-lane arrays; a pair
// with a larger component goes to a fallback list that a second kernel finishes with the shared Hungarian solver.  Only pairs
// with d = 1 - sim <= t are kept (wave-compacted, one atomic per wave), as two directed (row, col) entries with their float64
// distance.  Complete linkage cut at t < 1 is exact from those edges alone (missing = 1.0: any height above t blocks a merge
// whatever its value); average linkage scores every member pair of a connected group again (linkage.hip, exact fill).
#include <math.h>
#include <algorithm>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include "common.h"
#include "ivf.h"
#include "exwalk.h"
#include "peakmatch.h"
#include "util.h"

namespace fal {

constexpr int64_t kExEdgeBudget = 1ll << 25; // undirected edges held per batch of tiles before the host looks at the count

struct ExTile {
    int32_t a0, b0, end, pad;                // first row of the A side, of the B side (b0 >= a0), end of the bucket
};

__device__ __forceinline__ void ex_put_edge(uint64_t* keys, double* vals, unsigned long long slot, int32_t i, int32_t j, double d) {
    keys[2 * slot] = ((uint64_t)(uint32_t)i << 32) | (uint32_t)j;
    vals[2 * slot] = d;
    keys[2 * slot + 1] = ((uint64_t)(uint32_t)j << 32) | (uint32_t)i;
    vals[2 * slot + 1] = d;
}

__global__ __launch_bounds__(256) void exact_edges_kernel(const ExTile* __restrict__ tiles, ExactPeaks pk, double t,
                                                          uint64_t* __restrict__ keys, double* __restrict__ vals, int64_t cap,
                                                          unsigned long long* __restrict__ n_edges, int2* __restrict__ fb,
                                                          int64_t fb_cap, unsigned long long* __restrict__ n_fb) {
    __shared__ float s_mz[2][kExLdsPeaks];
    __shared__ float s_it[2][kExLdsPeaks];
    __shared__ int64_t s_off[2][64];
    __shared__ int s_len[2][128];
    __shared__ int s_tot[2];
    const ExTile tl = tiles[blockIdx.x];
    const int na_rows = min(kExTile, tl.end - tl.a0), nb_rows = min(kExTile, tl.end - tl.b0);
    const bool diag = tl.a0 == tl.b0;
    const bool fa = ex_stage(pk, tl.a0, na_rows, s_mz[0], s_it[0], s_off[0], s_len[0], &s_tot[0]);
    bool fbb = fa;
    if (!diag) fbb = ex_stage(pk, tl.b0, nb_rows, s_mz[1], s_it[1], s_off[1], s_len[1], &s_tot[1]);
    const int sb = diag ? 0 : 1;
    for (int p = threadIdx.x; p < kExTile * kExTile; p += 256) {      // (uniform trip count: every lane reaches the ballots)
        const int i = p >> 6, j = p & 63;
        const bool valid = i < na_rows && j < nb_rows && (!diag || j > i);
        bool hit = false, fall = false;
        double d = 1.0;
        if (valid) {
            const float* amz = fa ? s_mz[0] + s_len[0][64 + i] : pk.mz + s_off[0][i];
            const float* ait = fa ? s_it[0] + s_len[0][64 + i] : pk.it + s_off[0][i];
            const float* bmz = fbb ? s_mz[sb] + s_len[sb][64 + j] : pk.mz + s_off[sb][j];
            const float* bit = fbb ? s_it[sb] + s_len[sb][64 + j] : pk.it + s_off[sb][j];
            const PeakLists s{amz, ait, bmz, bit};
            double score = 0.0;
            int n_match = 0;
            if (ex_score_simple(s, s_len[0][i], s_len[sb][j], pk.tol, &score, &n_match)) {
                d = pair_distance(score, n_match, pk.min_matches);
                hit = d <= t;
            } else {
                fall = true;
            }
        }
        const unsigned long long e = ex_wave_slot(hit, n_edges);
        if (hit && e < (unsigned long long)cap) ex_put_edge(keys, vals, e, tl.a0 + i, tl.b0 + j, d);
        const unsigned long long f = ex_wave_slot(fall, n_fb);
        if (fall && f < (unsigned long long)fb_cap) fb[f] = make_int2(tl.a0 + i, tl.b0 + j);
    }
}

// the fallback list: pairs with a component of two or more query peaks, scored with the Hungarian solver
__global__ __launch_bounds__(256) void exact_fallback_kernel(const int2* __restrict__ fb, const unsigned long long* __restrict__ n_fb,
                                                             int64_t fb_cap, ExactPeaks pk, double t, uint64_t* __restrict__ keys,
                                                             double* __restrict__ vals, int64_t cap,
                                                             unsigned long long* __restrict__ n_edges) {
    const int64_t m = min((int64_t)*n_fb, fb_cap);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, rounds = (m + stride - 1) / stride;
    for (int64_t r = 0; r < rounds; ++r) {                              // (uniform trip count: every lane reaches the ballot)
        const int64_t x = (r * gridDim.x + blockIdx.x) * (int64_t)blockDim.x + threadIdx.x;
        bool hit = false;
        double d = 1.0;
        int2 ij = make_int2(0, 0);
        if (x < m) {
            ij = fb[x];
            bool ok = true;
            d = exact_distance(pk, ij.x, ij.y, &ok);
            if (!ok) atomicExch(pk.err, 1);
            hit = ok && d <= t;
        }
        const unsigned long long e = ex_wave_slot(hit, n_edges);
        if (hit && e < (unsigned long long)cap) ex_put_edge(keys, vals, e, ij.x, ij.y, d);
    }
}

// directed entries (key = row << 32 | col) -> CSR rows: degree histogram, then scatter (any order inside a row)
__global__ void ex_degree_kernel(const uint64_t* __restrict__ keys, const unsigned long long* __restrict__ n_edges, int64_t cap,
                                 int32_t* __restrict__ deg) {
    const int64_t m = 2 * min((int64_t)*n_edges, cap);
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&deg[keys[e] >> 32], 1);
}

__global__ void ex_scatter_kernel(const uint64_t* __restrict__ keys, const double* __restrict__ vals,
                                  const unsigned long long* __restrict__ n_edges, int64_t cap, const int64_t* __restrict__ ptr,
                                  int32_t* __restrict__ cursor, int32_t* __restrict__ idx, double* __restrict__ dist) {
    const int64_t m = 2 * min((int64_t)*n_edges, cap);
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[e];
        const uint32_t row = (uint32_t)(k >> 32);
        const int64_t pos = ptr[row] + atomicAdd(&cursor[row], 1);
        idx[pos] = (int32_t)(uint32_t)k;
        dist[pos] = vals[e];
    }
}

// sorted keys -> CSR (the staged call's deterministic form: rows ascending, columns ascending inside a row)
__global__ void ex_unpack_kernel(const uint64_t* __restrict__ keys, const double* __restrict__ vals, int64_t m,
                                 int32_t* __restrict__ idx, double* __restrict__ dist) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        idx[e] = (int32_t)(uint32_t)keys[e];
        dist[e] = vals[e];
    }
}

// ---- exact medoids -------------------------------------------------------------------------------------------------------
__global__ void ex_member_scatter_kernel(const int32_t* __restrict__ labels, int64_t n, const int64_t* __restrict__ off,
                                         int32_t* __restrict__ cursor, int32_t* __restrict__ mem) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = labels[i];
        if (l >= 0) mem[off[l] + atomicAdd(&cursor[l], 1)] = (int32_t)i;
    }
}

// members of every cluster in ascending row order (rank by counting inside the cluster)
__global__ void ex_member_sort_kernel(const int32_t* __restrict__ labels, int64_t n, const int64_t* __restrict__ off,
                                      const int32_t* __restrict__ size, const int32_t* __restrict__ mem, int32_t* __restrict__ sorted) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = labels[i];
        if (l < 0) continue;
        const int32_t* mu = mem + off[l];
        const int m = size[l];
        int rank = 0;
        for (int y = 0; y < m; ++y) rank += mu[y] < (int32_t)i;
        sorted[off[l] + rank] = (int32_t)i;
    }
}

// score_i = float32 sum, ascending member order, of float32(d(i, y)) over the other members y (reference medoids over the
// full block matrix, cluster.py:512-553); argmin per cluster with ties to the lowest row
__global__ __launch_bounds__(256) void ex_medoid_score_kernel(const int32_t* __restrict__ labels, int64_t n,
                                                              const int64_t* __restrict__ off, const int32_t* __restrict__ size,
                                                              const int32_t* __restrict__ sorted, ExactPeaks pk,
                                                              unsigned long long* __restrict__ best) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = labels[i];
        if (l < 0) continue;
        const int32_t* mu = sorted + off[l];
        const int m = size[l];
        float s = 0.f;
        bool ok = true;
        for (int y = 0; y < m; ++y) {
            const int64_t r = mu[y];
            if (r == i) continue;
            s += (float)(r < i ? exact_distance(pk, r, i, &ok) : exact_distance(pk, i, r, &ok));
        }
        if (!ok) atomicExch(pk.err, 1);
        const unsigned long long key = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(uint32_t)i;
        atomicMin(&best[l], key);
    }
}

int exact_medoids_dev(fal_ctx* ctx, const ExactPeaks& pk, const int32_t* labels_sorted, int64_t n, const int32_t* size,
                      unsigned long long* best) {
    hipStream_t st = ctx->stream;
    const int64_t cmax = n + 1;
    ScratchLayout L;
    const auto off = L.array<int64_t>(cmax + 1);
    const auto cursor = L.array<int32_t>(cmax), mem = L.array<int32_t>(n), sorted = L.array<int32_t>(n);
    L.pad(32);
    FAL_TRY(L.reserve(ctx, SLOT_EXACT6));
    const int grid = (int)std::min<int64_t>(ceil_div(n, 256), (int64_t)ctx->num_cus * 16);
    FAL_CHECK_HIP(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)cmax, st));
    FAL_TRY(device_scan_i32(ctx, size, cmax, off, SLOT_TAIL3));
    hipLaunchKernelGGL(ex_member_scatter_kernel, dim3(grid), dim3(256), 0, st, labels_sorted, n, off, cursor, mem);
    hipLaunchKernelGGL(ex_member_sort_kernel, dim3(grid), dim3(256), 0, st, labels_sorted, n, off, size, mem, sorted);
    hipLaunchKernelGGL(ex_medoid_score_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(n, 64), (int64_t)ctx->num_cus * 64)), dim3(64),
                       0, st, labels_sorted, n, off, size, sorted, pk, best);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}

// ---- the edge pass -------------------------------------------------------------------------------------------------------
struct ExEdges {
    uint64_t* keys = nullptr;           // 2 * cap directed entries (unsorted)
    double* vals = nullptr;
    int64_t cap = 0;                    // undirected edges the buffers hold
    unsigned long long* d_count = nullptr;   // undirected edges found (device)
    int32_t* d_err = nullptr;
};

// every pair of every bucket [splits[b], splits[b + 1]); edges d <= t into library scratch.  The tiles run in batches whose
// pair count fits the room left in the buffers: one launch when every pair fits, otherwise the host reads the count between
// batches (and grows the buffers when a single tile no longer fits).  No pair is scored twice.
static int exact_edges_dev(fal_ctx* ctx, const ExactPeaks& pk_in, int64_t n, const int64_t* splits, int64_t n_splits, double t,
                           ExEdges* out) {
    hipStream_t st = ctx->stream;
    std::vector<ExTile> tiles;
    std::vector<int64_t> tpairs;
    for (int64_t b = 0; b + 1 < n_splits; ++b) {
        const int64_t s0 = splits[b], s1 = splits[b + 1];
        FAL_REQUIRE(s0 >= 0 && s1 >= s0 && s1 <= n, FAL_EINVAL, "exact edges: the bucket table must ascend within [0, n]");
        for (int64_t a0 = s0; a0 < s1; a0 += kExTile)
            for (int64_t b0 = a0; b0 < s1; b0 += kExTile) {
                const int64_t ra = std::min<int64_t>(kExTile, s1 - a0), rb = std::min<int64_t>(kExTile, s1 - b0);
                const int64_t pairs = a0 == b0 ? ra * (ra - 1) / 2 : ra * rb;
                if (pairs == 0) continue;
                tiles.push_back(ExTile{(int32_t)a0, (int32_t)b0, (int32_t)s1, 0});
                tpairs.push_back(pairs);
            }
    }
    int64_t total = 0;
    for (int64_t p : tpairs) total += p;
    int32_t* misc = nullptr;
    FAL_TRY(ctx->reserve(SLOT_EXACT5, 64, (void**)&misc));
    out->d_err = misc;
    out->d_count = reinterpret_cast<unsigned long long*>(misc + 2);
    unsigned long long* d_fb = out->d_count + 1;
    FAL_CHECK_HIP(hipMemsetAsync(misc, 0, 64, st));
    ExactPeaks pk = pk_in;
    pk.err = out->d_err;
    const int64_t cap0 = std::max<int64_t>(1, std::min<int64_t>(total, kExEdgeBudget));
    auto reserve_edges = [&](int64_t cap) -> int {
        ScratchLayout L;
        const auto keys = L.array<uint64_t>(2 * cap);
        const auto vals = L.array<double>(2 * cap);
        FAL_TRY(L.reserve(ctx, SLOT_EXACT));
        out->keys = keys;
        out->vals = vals;
        out->cap = cap;
        return FAL_OK;
    };
    FAL_TRY(reserve_edges(cap0));
    if (tiles.empty()) return FAL_OK;
    const int64_t fb_cap = cap0;                          // a batch never holds more pairs than that
    int2* fb = nullptr;
    ExTile* d_tiles = nullptr;
    FAL_TRY(ctx->reserve(SLOT_EXACT2, sizeof(int2) * (size_t)fb_cap, (void**)&fb));
    FAL_TRY(ctx->reserve(SLOT_EXACT3, sizeof(ExTile) * tiles.size(), (void**)&d_tiles));
    FAL_TRY(ctx->upload(d_tiles, tiles.data(), sizeof(ExTile) * tiles.size()));
    unsigned long long* h_count = nullptr;
    FAL_TRY(ctx->pinned_reserve(sizeof(unsigned long long), (void**)&h_count));
    int64_t used = 0;                                     // edges known to be stored (host)
    size_t pos = 0;
    while (pos < tiles.size()) {
        const int64_t room = std::min<int64_t>(out->cap - used, fb_cap);
        if (tpairs[pos] > room) {                         // grow: the stored edges move to the larger block
            const int64_t cap = std::max<int64_t>(2 * out->cap, used + fb_cap);
            uint64_t* ok = out->keys;
            double* ov = out->vals;
            ctx->release(SLOT_EXACT);
            FAL_TRY(reserve_edges(cap));
            FAL_CHECK_HIP(hipMemcpyAsync(out->keys, ok, sizeof(uint64_t) * 2 * (size_t)used, hipMemcpyDeviceToDevice, st));
            FAL_CHECK_HIP(hipMemcpyAsync(out->vals, ov, sizeof(double) * 2 * (size_t)used, hipMemcpyDeviceToDevice, st));
            continue;
        }
        size_t end = pos;
        int64_t pairs = 0;
        while (end < tiles.size() && pairs + tpairs[end] <= room) pairs += tpairs[end++];
        FAL_CHECK_HIP(hipMemsetAsync(d_fb, 0, sizeof(unsigned long long), st));
        {
            StageScope ts(ctx, ST_KERNEL);
            hipLaunchKernelGGL(exact_edges_kernel, dim3((unsigned)(end - pos)), dim3(256), 0, st, d_tiles + pos, pk, t, out->keys,
                               out->vals, out->cap, out->d_count, fb, fb_cap, d_fb);
        }
        hipLaunchKernelGGL(exact_fallback_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(pairs, 256), (int64_t)ctx->num_cus * 8)),
                           dim3(256), 0, st, fb, d_fb, fb_cap, pk, t, out->keys, out->vals, out->cap, out->d_count);
        FAL_CHECK_HIP(hipGetLastError());
        pos = end;
        if (pos < tiles.size()) {                         // more batches: how much room is left
            FAL_CHECK_HIP(hipMemcpyAsync(h_count, out->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            FAL_CHECK_HIP(hipStreamSynchronize(st));
            used = (int64_t)*h_count;
        }
    }
    return FAL_OK;
}

// (the error word lands behind the first 32 bytes of the pinned buffer: the callers' counts use those)
static int read_err(fal_ctx* ctx, const int32_t* d_err, const char* what) {
    unsigned char* pin = nullptr;
    FAL_TRY(ctx->pinned_reserve(64, (void**)&pin));
    int32_t* h = reinterpret_cast<int32_t*>(pin + 32);
    FAL_CHECK_HIP(hipMemcpyAsync(h, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return ex_check_err(*h, what);
}

// unsorted directed entries -> CSR rows (columns in any order), all on the device; the arrays live in SLOT_EXACT4
static int exact_csr_dev(fal_ctx* ctx, const ExEdges& ed, int64_t n, int64_t** ptr_out, int32_t** idx_out, double** dist_out) {
    hipStream_t st = ctx->stream;
    const int64_t m = 2 * ed.cap;
    ScratchLayout L;
    const auto ptr = L.array<int64_t>(n + 1);
    const auto dist = L.array<double>(m);
    const auto deg = L.array<int32_t>(n), cursor = L.array<int32_t>(n);      // one memset clears both
    const auto idx = L.array<int32_t>(m);
    L.pad(64);
    FAL_TRY(L.reserve(ctx, SLOT_EXACT4));
    FAL_CHECK_HIP(hipMemsetAsync(deg, 0, sizeof(int32_t) * (size_t)(2 * n), st));
    const int egrid = (int)std::min<int64_t>(ceil_div(m, 256), (int64_t)ctx->num_cus * 32);
    hipLaunchKernelGGL(ex_degree_kernel, dim3(egrid), dim3(256), 0, st, ed.keys, ed.d_count, ed.cap, deg);
    FAL_TRY(device_scan_i32(ctx, deg, n, ptr, SLOT_DB3));
    hipLaunchKernelGGL(ex_scatter_kernel, dim3(egrid), dim3(256), 0, st, ed.keys, ed.vals, ed.d_count, ed.cap, ptr, cursor, idx, dist);
    FAL_CHECK_HIP(hipGetLastError());
    *ptr_out = ptr;
    *idx_out = idx;
    *dist_out = dist;
    return FAL_OK;
}

// util.h: the library's one instantiation of the 64-bit pair sort (exact mode's edges; network.hip's edges and rank entries)
int sort_pairs_u64_f64(fal_ctx* ctx, uint64_t* kin, uint64_t* kout, double* vin, double* vout, int64_t n, int scratch_slot) {
    size_t bytes = 0;
    FAL_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, (size_t)n, 0, 64, ctx->stream));
    void* tmp = nullptr;
    FAL_TRY(ctx->reserve(scratch_slot, bytes + 16, &tmp));
    FAL_CHECK_HIP(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0, 64, ctx->stream));
    return FAL_OK;
}

static ExactPeaks make_peaks(const float* mz, const float* intensity, const int64_t* indptr, const int64_t* row_order,
                             double fragment_tol, int min_matches) {
    ExactPeaks pk;
    pk.mz = mz;
    pk.it = intensity;
    pk.indptr = indptr;
    pk.order = row_order;
    pk.tol = fragment_tol;
    pk.min_matches = min_matches;
    pk.err = nullptr;
    return pk;
}

}  // namespace fal
FAL_WARM_KERNEL(fal::exact_edges_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" {

int fal_exact_edges(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, const int64_t* row_order, int64_t n,
                    const int64_t* splits, int64_t n_splits, double fragment_tol, int min_matches, double threshold,
                    int64_t* csr_indptr, int32_t* csr_idx, double* csr_dist, int64_t max_edges, int64_t* n_edges) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_edges && n >= 0 && n < (int64_t)INT32_MAX && fragment_tol >= 0.0 && max_edges >= 0, FAL_EINVAL,
                "fal_exact_edges: bad argument");
    FAL_REQUIRE(threshold < 1.0, FAL_EUNSUPPORTED, "fal_exact_edges: the threshold must be below 1 (the distance of a missing pair)");
    *n_edges = 0;
    FAL_REQUIRE(csr_indptr, FAL_EINVAL, "fal_exact_edges: NULL csr_indptr");
    if (n == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(csr_indptr, 0, sizeof(int64_t), ctx->stream));
        FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        return FAL_OK;
    }
    FAL_REQUIRE(mz && intensity && indptr && row_order && splits && n_splits >= 2, FAL_EINVAL, "fal_exact_edges: NULL array");
    FAL_REQUIRE(splits[0] == 0 && splits[n_splits - 1] == n, FAL_EINVAL, "fal_exact_edges: the bucket table must run from 0 to n");
    const ExactPeaks pk = make_peaks(mz, intensity, indptr, row_order, fragment_tol, min_matches);
    ExEdges ed;
    ctx->stage_reset(ST_KERNEL);
    FAL_TRY(exact_edges_dev(ctx, pk, n, splits, n_splits, threshold, &ed));
    FAL_TRY(read_err(ctx, ed.d_err, "fal_exact_edges"));
    unsigned long long* h = nullptr;
    FAL_TRY(ctx->pinned_reserve(sizeof(unsigned long long), (void**)&h));
    FAL_CHECK_HIP(hipMemcpyAsync(h, ed.d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t m = 2 * (int64_t)*h;
    *n_edges = m;
    FAL_REQUIRE(m <= max_edges, FAL_EINVAL, "fal_exact_edges: %lld directed edges do not fit max_edges %lld", (long long)m,
                (long long)max_edges);
    FAL_REQUIRE(m == 0 || (csr_idx && csr_dist), FAL_EINVAL, "fal_exact_edges: NULL csr_idx / csr_dist");
    hipStream_t st = ctx->stream;
    // deterministic order: (row, col) keys are unique, a radix sort puts them in place
    ScratchLayout L;
    const auto kout = L.array<uint64_t>(m);
    const auto vout = L.array<double>(m);
    const auto deg = L.array<int32_t>(n);
    L.pad(64);
    FAL_TRY(L.reserve(ctx, SLOT_EXACT4));
    if (m > 0) FAL_TRY(sort_pairs_u64_f64(ctx, ed.keys, kout, ed.vals, vout, m, SLOT_EXACT6));
    const int egrid = (int)std::min<int64_t>(ceil_div(std::max<int64_t>(m, 1), 256), (int64_t)ctx->num_cus * 32);
    FAL_CHECK_HIP(hipMemsetAsync(deg, 0, sizeof(int32_t) * (size_t)n, st));
    if (m > 0) {
        // (the degree kernel reads the undirected count from the device: m / 2 of the sorted keys' pairs)
        hipLaunchKernelGGL(ex_degree_kernel, dim3(egrid), dim3(256), 0, st, kout, ed.d_count, ed.cap, deg);
        hipLaunchKernelGGL(ex_unpack_kernel, dim3(egrid), dim3(256), 0, st, kout, vout, m, csr_idx, csr_dist);
    }
    FAL_TRY(device_scan_i32(ctx, deg, n, csr_indptr, SLOT_DB3));
    FAL_CHECK_HIP(hipGetLastError());
    FAL_CHECK_HIP(hipStreamSynchronize(st));
    return FAL_OK;
}

int fal_linkage_cluster_csr(fal_ctx* ctx, const int64_t* csr_indptr, const int32_t* csr_idx, const double* csr_dist, int64_t n,
                            double threshold, int method, const float* mz, const float* intensity, const int64_t* indptr,
                            const int64_t* row_order, double fragment_tol, int min_matches, int32_t* labels, int64_t* n_clusters) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && n < (int64_t)INT32_MAX, FAL_EINVAL, "fal_linkage_cluster_csr: bad argument");
    FAL_REQUIRE(method >= 0 && method <= 2, FAL_EINVAL, "fal_linkage_cluster_csr: method must be 0 (single), 1 (complete) or 2 (average)");
    FAL_REQUIRE(threshold < 1.0, FAL_EUNSUPPORTED, "fal_linkage_cluster_csr: the threshold must be below 1 (the distance of a missing pair)");
    if (n_clusters) *n_clusters = 0;
    if (n == 0) return FAL_OK;
    FAL_REQUIRE(csr_indptr && csr_idx && csr_dist && labels, FAL_EINVAL, "fal_linkage_cluster_csr: NULL array");
    FAL_REQUIRE(method != 2 || (mz && intensity && indptr && row_order), FAL_EINVAL,
                "fal_linkage_cluster_csr: average linkage scores every member pair again and needs the peak lists");
    int32_t* err = nullptr;
    FAL_TRY(ctx->reserve(SLOT_EXACT5, 64, (void**)&err));
    FAL_CHECK_HIP(hipMemsetAsync(err, 0, 64, ctx->stream));
    LinkageSource src;
    src.csr_ptr = csr_indptr;
    src.csr_idx = csr_idx;
    src.csr_dist = csr_dist;
    src.exact_fill = method == 2;
    src.peaks = make_peaks(mz, intensity, indptr, row_order, fragment_tol, min_matches);
    src.peaks.err = err;
    int64_t* d_count = nullptr;
    FAL_TRY(linkage_dev_src(ctx, src, n, threshold, method, labels, &d_count));
    int64_t* h = nullptr;
    FAL_TRY(ctx->pinned_reserve(sizeof(int64_t), (void**)&h));
    FAL_CHECK_HIP(hipMemcpyAsync(h, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_TRY(read_err(ctx, err, "fal_linkage_cluster_csr"));
    if (n_clusters) *n_clusters = *h;
    return FAL_OK;
}

int fal_cluster_exact(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, const int64_t* row_order, int64_t n,
                      const int64_t* splits, int64_t n_splits, double fragment_tol, int min_matches, double threshold, int method,
                      const float* precursor_mz_sorted, const float* rt_sorted, double tol, int tol_is_da, double rt_tol,
                      int32_t* labels_sorted_scratch, int32_t* labels_out, int32_t* medoids_out, int64_t* n_clusters,
                      int64_t* n_labels) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && n < (int64_t)INT32_MAX && n_clusters && n_labels && fragment_tol >= 0.0, FAL_EINVAL,
                "fal_cluster_exact: bad argument");
    FAL_REQUIRE(method >= 0 && method <= 2, FAL_EINVAL, "fal_cluster_exact: method must be 0 (single), 1 (complete) or 2 (average)");
    FAL_REQUIRE(threshold < 1.0, FAL_EUNSUPPORTED, "fal_cluster_exact: the threshold must be below 1 (the distance of a missing pair)");
    *n_clusters = *n_labels = 0;
    if (n == 0) return FAL_OK;
    FAL_REQUIRE(mz && intensity && indptr && row_order && splits && n_splits >= 2 && precursor_mz_sorted && labels_sorted_scratch &&
                labels_out && medoids_out, FAL_EINVAL, "fal_cluster_exact: NULL array");
    FAL_REQUIRE(splits[0] == 0 && splits[n_splits - 1] == n, FAL_EINVAL, "fal_cluster_exact: the bucket table must run from 0 to n");
    ExactPeaks pk = make_peaks(mz, intensity, indptr, row_order, fragment_tol, min_matches);
    ExEdges ed;
    ctx->stage_reset(ST_KERNEL);
    ctx->stage_reset(ST_SCAN);
    {
        StageScope ts(ctx, ST_SCAN);
        FAL_TRY(exact_edges_dev(ctx, pk, n, splits, n_splits, threshold, &ed));
    }
    pk.err = ed.d_err;
    int64_t* ptr = nullptr;
    int32_t* idx = nullptr;
    double* dist = nullptr;
    FAL_TRY(exact_csr_dev(ctx, ed, n, &ptr, &idx, &dist));
    LinkageSource src;
    src.csr_ptr = ptr;
    src.csr_idx = idx;
    src.csr_dist = dist;
    src.exact_fill = method == 2;
    src.peaks = pk;
    int64_t *d_db = nullptr, *d_cl = nullptr, *d_noise = nullptr;
    ctx->stage_reset(ST_TAIL);
    FAL_TRY(linkage_dev_src(ctx, src, n, threshold, method, labels_sorted_scratch, &d_db));
    FAL_TRY(refine_dev(ctx, labels_sorted_scratch, n, precursor_mz_sorted, rt_sorted, tol, tol_is_da, rt_tol, d_db, &d_cl));
    FAL_TRY(finalize_dev(ctx, labels_sorted_scratch, n, d_cl, row_order, nullptr, nullptr, 1, labels_out, medoids_out, &d_noise,
                         nullptr, &pk));
    int64_t* h = nullptr;
    FAL_TRY(ctx->pinned_reserve(2 * sizeof(int64_t), (void**)&h));
    FAL_CHECK_HIP(hipMemcpyAsync(&h[0], d_cl, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipMemcpyAsync(&h[1], d_noise, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_TRY(read_err(ctx, ed.d_err, "fal_cluster_exact"));         // (synchronises)
    *n_clusters = h[0];
    *n_labels = h[0] + h[1];
    return FAL_OK;
}

}  // extern "C"
