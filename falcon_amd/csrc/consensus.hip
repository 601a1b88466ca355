// Consensus representatives (fal_consensus_spectra; DESIGN.md "Consensus representatives"): the members of every cluster merged
// peak by peak.  Rows are sorted by label (stable radix sort: members in dataset-row order), their peaks pooled cluster by
// cluster, every cluster's pool sorted by (m/z, pooled position) -- inside one workgroup's LDS up to kConsLdsPeaks peaks, by two
// stable device-wide radix passes above that --, and one thread per group start then walks its group in pooled order with the
// arithmetic of consensus.h.  Count, scan, emit: the output sizes stay on the device.
#include <algorithm>
#include "common.h"
#include "consensus.h"
#include "ivf.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kConsBlock = 256;

// first position of the sorted keys that is >= v
__device__ __forceinline__ int64_t cons_lower_bound(const uint32_t* __restrict__ a, int64_t n, uint32_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// last position of the non-decreasing offsets a[0 .. n) with a[pos] <= v (a[0] <= v)
__device__ __forceinline__ int64_t cons_segment_of(const int64_t* __restrict__ a, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__global__ void cons_label_keys_kernel(const int32_t* __restrict__ labels, int64_t n, uint32_t* __restrict__ key,
                                       int32_t* __restrict__ row) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        key[i] = (uint32_t)labels[i];          // a negative label sorts behind every cluster
        row[i] = (int32_t)i;
    }
}

// peaks of the i-th member in (label, row) order; rows outside [0, n_clusters) pool nothing
__global__ void cons_member_counts_kernel(const uint32_t* __restrict__ key, const int32_t* __restrict__ row, int64_t n,
                                          int64_t n_clusters, const int64_t* __restrict__ indptr, int32_t* __restrict__ count) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = row[i];
        const int64_t c = indptr[r + 1] - indptr[r];
        count[i] = ((int64_t)key[i] < n_clusters && c > 0) ? (int32_t)c : 0;
    }
}

// first member of every cluster (and of the end) in the sorted rows
__global__ void cons_cluster_start_kernel(const uint32_t* __restrict__ key, int64_t n, int64_t n_clusters,
                                          int64_t* __restrict__ cstart) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c <= n_clusters; c += (int64_t)gridDim.x * blockDim.x)
        cstart[c] = cons_lower_bound(key, n, (uint32_t)c);
}

// pool offset of every cluster; the pool sizes of the clusters the device-wide sort takes (0 for the others)
__global__ void cons_cluster_sizes_kernel(const int64_t* __restrict__ cstart, const int64_t* __restrict__ pool_off,
                                          int64_t n_clusters, int64_t* __restrict__ cpool, int64_t* __restrict__ big_size,
                                          int32_t* __restrict__ kept_count) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c <= n_clusters; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = pool_off[cstart[c]];
        cpool[c] = p;
        if (c == n_clusters) break;
        const int64_t m = cstart[c + 1] - cstart[c], size = pool_off[cstart[c + 1]] - p;
        const bool big = m > 1 && size > kConsLdsPeaks;
        big_size[c] = big ? size : 0;
        kept_count[c] = 0;
    }
}

// pooled position k -> its peak in the CSR and its cluster
__global__ void cons_pool_kernel(const int64_t* __restrict__ pool_off, const uint32_t* __restrict__ key,
                                 const int32_t* __restrict__ row, int64_t n, int64_t pooled, const int64_t* __restrict__ indptr,
                                 int32_t* __restrict__ pool_peak, int32_t* __restrict__ pool_cluster) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < pooled; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = cons_segment_of(pool_off, n + 1, k);       // (members without peaks share an offset: the last one holds k)
        pool_peak[k] = (int32_t)(indptr[row[i]] + (k - pool_off[i]));
        pool_cluster[k] = (int32_t)key[i];
    }
}

// one workgroup per cluster of 2+ members and at most kConsLdsPeaks pooled peaks: bitonic sort of (m/z key, pooled position)
// in LDS; the pool is in (row, peak index) order, so the position breaks m/z ties the way the pooled order asks
__global__ __launch_bounds__(kConsBlock) void cons_sort_lds_kernel(const int64_t* __restrict__ cstart, const int64_t* __restrict__ cpool,
                                                                   int64_t n_clusters, const int32_t* __restrict__ pool_peak,
                                                                   const float* __restrict__ mz, const float* __restrict__ intensity,
                                                                   float* __restrict__ smz, float* __restrict__ sint) {
    __shared__ uint64_t keys[kConsLdsPeaks];
    for (int64_t c = blockIdx.x; c < n_clusters; c += gridDim.x) {
        const int64_t p = cpool[c], size = cpool[c + 1] - p;
        if (cstart[c + 1] - cstart[c] < 2 || size < 1 || size > kConsLdsPeaks) continue;      // (uniform over the workgroup)
        int np = 1;
        while (np < (int)size) np <<= 1;
        __syncthreads();                                                                       // the previous cluster's reads
        for (int t = threadIdx.x; t < np; t += kConsBlock)
            keys[t] = t < (int)size ? ((uint64_t)cons_mz_key(mz[pool_peak[p + t]]) << 32) | (uint32_t)t : ~0ull;
        __syncthreads();
        for (int kk = 2; kk <= np; kk <<= 1)
            for (int j = kk >> 1; j > 0; j >>= 1) {
                for (int t = threadIdx.x; t < np; t += kConsBlock) {
                    const int u = t ^ j;
                    if (u > t) {
                        const uint64_t a = keys[t], b = keys[u];
                        if ((a > b) == ((t & kk) == 0)) {
                            keys[t] = b;
                            keys[u] = a;
                        }
                    }
                }
                __syncthreads();
            }
        for (int t = threadIdx.x; t < (int)size; t += kConsBlock) {
            const int32_t g = pool_peak[p + (int64_t)(uint32_t)keys[t]];
            smz[p + t] = mz[g];
            sint[p + t] = intensity[g];
        }
    }
}

// the device-wide path: slot q of the big clusters' pools (cluster-major, like the pool) -> (m/z key, pooled position)
__global__ void cons_big_keys_kernel(const int64_t* __restrict__ big_off, const int64_t* __restrict__ cpool, int64_t n_clusters,
                                     int64_t n_big, const int32_t* __restrict__ pool_peak, const float* __restrict__ mz,
                                     uint32_t* __restrict__ key, int32_t* __restrict__ val) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_big; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = cons_segment_of(big_off, n_clusters + 1, q);      // (the others hold no slot: the last offset <= q is c's)
        const int64_t k = cpool[c] + (q - big_off[c]);
        key[q] = cons_mz_key(mz[pool_peak[k]]);
        val[q] = (int32_t)k;
    }
}

__global__ void cons_big_cluster_keys_kernel(const int32_t* __restrict__ val, int64_t n_big, const int32_t* __restrict__ pool_cluster,
                                             uint32_t* __restrict__ key) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_big; q += (int64_t)gridDim.x * blockDim.x)
        key[q] = (uint32_t)pool_cluster[val[q]];
}

// slot q of the sorted (cluster, m/z, pooled position) sequence is the (q - big_off[c])-th peak of cluster c's pooled order
__global__ void cons_big_scatter_kernel(const uint32_t* __restrict__ key, const int32_t* __restrict__ val, int64_t n_big,
                                        const int64_t* __restrict__ big_off, const int64_t* __restrict__ cpool,
                                        const int32_t* __restrict__ pool_peak, const float* __restrict__ mz,
                                        const float* __restrict__ intensity, float* __restrict__ smz, float* __restrict__ sint) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_big; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = key[q];
        const int64_t k = cpool[c] + (q - big_off[c]);
        const int32_t g = pool_peak[val[q]];
        smz[k] = mz[g];
        sint[k] = intensity[g];
    }
}

// one thread per pooled peak: the peak that starts a group walks the group in pooled order (consensus.h) and, where the group
// reaches the quorum, leaves its m/z and raw intensity at its own position
__global__ void cons_groups_kernel(const int32_t* __restrict__ pool_cluster, int64_t pooled, const int64_t* __restrict__ cstart,
                                   const int64_t* __restrict__ cpool, const float* __restrict__ smz, const float* __restrict__ sint,
                                   double fragment_tol, double min_fraction, uint8_t* __restrict__ kept, float* __restrict__ gmz,
                                   double* __restrict__ graw, int32_t* __restrict__ kept_count) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < pooled; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = pool_cluster[k];
        const int64_t m = cstart[c + 1] - cstart[c], p = cpool[c], end = cpool[c + 1];
        kept[k] = 0;
        if (m < 2) continue;
        float prev = smz[k];
        if (k > p && !cons_new_group(prev, smz[k - 1], fragment_tol)) continue;
        ConsGroup g;
        cons_group_add(g, prev, sint[k]);
        for (int64_t j = k + 1; j < end; ++j) {
            const float x = smz[j];
            if (cons_new_group(x, prev, fragment_tol)) break;
            cons_group_add(g, x, sint[j]);
            prev = x;
        }
        if (!cons_group_kept(g, m, cons_need(min_fraction, m))) continue;
        kept[k] = 1;
        gmz[k] = cons_group_mz(g);
        graw[k] = cons_group_raw(g, m);
        atomicAdd(&kept_count[c], 1);
    }
}

// peaks every cluster writes, and its status (the capacity bit is the emit kernel's)
__global__ void cons_out_counts_kernel(const int64_t* __restrict__ cstart, const int64_t* __restrict__ cpool,
                                       const int64_t* __restrict__ big_size, const int32_t* __restrict__ kept_count,
                                       const int32_t* __restrict__ medoids, const int64_t* __restrict__ indptr, int64_t n,
                                       int64_t n_clusters, int64_t* __restrict__ out_count, int32_t* __restrict__ status) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_clusters; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = cstart[c + 1] - cstart[c];
        int st = big_size[c] > 0 ? FAL_CONS_ST_GLOBAL : 0;
        int64_t count;
        if (m == 1) {
            count = cpool[c + 1] - cpool[c];
        } else if (m > 1 && kept_count[c] > 0) {
            count = kept_count[c];
        } else {
            const int64_t med = medoids[c];
            count = (med >= 0 && med < n) ? std::max<int64_t>(indptr[med + 1] - indptr[med], 0) : 0;
            st |= FAL_CONS_ST_FALLBACK;
        }
        out_count[c] = count;
        status[c] = st;
    }
}

// one wave per cluster: a single member's / the medoid's peaks copied, else the kept groups compacted in pooled (= m/z) order,
// the norm summed over them in that order first
__global__ __launch_bounds__(kConsBlock) void cons_emit_kernel(const int64_t* __restrict__ cstart, const int64_t* __restrict__ cpool,
                                                               int64_t n_clusters, const int32_t* __restrict__ pool_peak,
                                                               const int32_t* __restrict__ medoids, const int64_t* __restrict__ indptr,
                                                               const float* __restrict__ mz, const float* __restrict__ intensity,
                                                               const uint8_t* __restrict__ kept, const float* __restrict__ gmz,
                                                               const double* __restrict__ graw, const int64_t* __restrict__ out_indptr,
                                                               int64_t nnz_cap, float* __restrict__ out_mz,
                                                               float* __restrict__ out_intensity, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)kConsBlock + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * kConsBlock) >> 6;
    for (int64_t c = wave; c < n_clusters; c += n_waves) {
        const int64_t o = out_indptr[c], oe = out_indptr[c + 1];
        const int st = status[c];
        if (oe > nnz_cap) {
            if (lane == 0) status[c] = st | FAL_CONS_ST_CAPACITY;
            continue;
        }
        const int64_t m = cstart[c + 1] - cstart[c], p = cpool[c], end = cpool[c + 1];
        if (st & FAL_CONS_ST_FALLBACK) {
            const int64_t src = oe > o ? indptr[medoids[c]] : 0;      // (oe > o: the medoid is a row of the dataset)
            for (int64_t j = lane; j < oe - o; j += 64) {
                out_mz[o + j] = mz[src + j];
                out_intensity[o + j] = intensity[src + j];
            }
            continue;
        }
        if (m == 1) {
            for (int64_t j = lane; j < oe - o; j += 64) {
                const int32_t g = pool_peak[p + j];
                out_mz[o + j] = mz[g];
                out_intensity[o + j] = intensity[g];
            }
            continue;
        }
        double norm2 = 0.0;
        for (int64_t base = p; base < end; base += 64) {
            const int64_t k = base + lane;
            const bool on = k < end && kept[k];
            const double raw = on ? graw[k] : 0.0;
            unsigned long long b = __ballot(on);
            while (b) {
                cons_norm_add(norm2, __shfl(raw, __builtin_ctzll(b), 64));
                b &= b - 1;
            }
        }
        int64_t w = o;
        for (int64_t base = p; base < end; base += 64) {
            const int64_t k = base + lane;
            const bool on = k < end && kept[k];
            const unsigned long long b = __ballot(on);
            if (on) {
                const int64_t dst = w + __builtin_popcountll(b & ((1ull << lane) - 1ull));
                if (dst < oe) {                                            // (holds: oe - o = the cluster's kept groups)
                    out_mz[dst] = gmz[k];
                    out_intensity[dst] = cons_intensity(graw[k], norm2);
                }
            }
            w += __builtin_popcountll(b);
        }
    }
}

int bits_for(int64_t values) {       // radix bits that tell `values` keys 0 .. values - 1 apart
    int b = 1;
    while (b < 32 && (1ll << b) < values) ++b;
    return b;
}

}  // namespace
}  // namespace fal
FAL_WARM_KERNEL(fal::cons_label_keys_kernel);

using namespace fal;

extern "C" int fal_consensus_spectra(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n,
                                     const int32_t* labels, const int32_t* medoids, int64_t n_clusters, double fragment_tol,
                                     double min_fraction, int64_t nnz_cap, int64_t* out_indptr, float* out_mz, float* out_intensity,
                                     int32_t* status_out) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && n_clusters >= 0 && nnz_cap >= 0 && n < (1ll << 31) && n_clusters < (1ll << 31), FAL_EINVAL,
                "fal_consensus_spectra: bad argument");
    FAL_REQUIRE(fragment_tol >= 0.0 && min_fraction > 0.0 && min_fraction <= 1.0, FAL_EINVAL,
                "fal_consensus_spectra: fragment_tol must be >= 0 and min_fraction in (0, 1]");
    FAL_REQUIRE(out_indptr, FAL_EINVAL, "fal_consensus_spectra: NULL out_indptr");
    if (n_clusters == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int64_t), ctx->stream));
        return FAL_OK;
    }
    FAL_REQUIRE(indptr && medoids && status_out && (n == 0 || labels), FAL_EINVAL, "fal_consensus_spectra: NULL table");
    FAL_REQUIRE(nnz_cap == 0 || (out_mz && out_intensity), FAL_EINVAL, "fal_consensus_spectra: NULL peaks");
    hipStream_t s = ctx->stream;
    const auto grid_for = [&](int64_t items) {
        return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, kConsBlock), (int64_t)ctx->num_cus * 16)));
    };
    const int64_t n1 = std::max<int64_t>(n, 1), nc = n_clusters;

    // ---- rows by (label, row); the pool offset of every member and cluster ---------------------------------------------------
    ScratchLayout LA, LB, LP;
    const auto key_in = LA.array<uint32_t>(n1), key = LA.array<uint32_t>(n1);
    const auto row_in = LA.array<int32_t>(n1), row = LA.array<int32_t>(n1), mcount = LA.array<int32_t>(n1);
    LA.pad(64);
    FAL_TRY(LA.reserve(ctx, SLOT_TAIL));
    int64_t* pool_off = nullptr;
    FAL_TRY(ctx->reserve(SLOT_TAIL2, sizeof(int64_t) * (size_t)(n + 2), (void**)&pool_off));
    const auto cstart = LB.array<int64_t>(nc + 1), cpool = LB.array<int64_t>(nc + 1), big_size = LB.array<int64_t>(nc + 1);
    const auto big_off = LB.array<int64_t>(nc + 1), out_count = LB.array<int64_t>(nc + 1);
    const auto kept_count = LB.array<int32_t>(nc);
    FAL_TRY(LB.reserve(ctx, SLOT_TAIL3));
    if (n > 0) {
        hipLaunchKernelGGL(cons_label_keys_kernel, grid_for(n), dim3(kConsBlock), 0, s, labels, n, key_in, row_in);
        FAL_CHECK_HIP(hipGetLastError());
        FAL_TRY(sort_pairs_u32_i32(ctx, key_in, key, row_in, row, n, 32, SLOT_SORT));
        hipLaunchKernelGGL(cons_member_counts_kernel, grid_for(n), dim3(kConsBlock), 0, s, key, row, n, nc, indptr, mcount);
        FAL_CHECK_HIP(hipGetLastError());
    }
    FAL_TRY(device_scan_i32(ctx, mcount, n, pool_off, SLOT_SORT2));
    hipLaunchKernelGGL(cons_cluster_start_kernel, grid_for(nc + 1), dim3(kConsBlock), 0, s, key, n, nc, cstart);
    FAL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cons_cluster_sizes_kernel, grid_for(nc + 1), dim3(kConsBlock), 0, s, cstart, pool_off, nc, cpool, big_size,
                       kept_count);
    FAL_CHECK_HIP(hipGetLastError());
    ctx->release(SLOT_SORT2);
    FAL_TRY(device_scan_i64(ctx, big_size, nc, big_off, SLOT_SORT2));

    // ---- the one synchronisation: pooled peaks, and how many of them the device-wide sort takes --------------------------------
    int64_t* h = nullptr;
    FAL_TRY(ctx->pinned_reserve(3 * sizeof(int64_t), (void**)&h));
    FAL_CHECK_HIP(hipMemcpyAsync(h, pool_off + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    FAL_CHECK_HIP(hipMemcpyAsync(h + 1, big_off + nc, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    FAL_CHECK_HIP(hipMemcpyAsync(h + 2, indptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    FAL_CHECK_HIP(hipStreamSynchronize(s));
    const int64_t pooled = h[0], n_big = h[1], nnz = h[2];
    FAL_REQUIRE(nnz >= 0 && nnz < (1ll << 31) && pooled >= 0 && pooled <= nnz && n_big >= 0 && n_big <= pooled, FAL_EUNSUPPORTED,
                "fal_consensus_spectra: %lld peaks (the pooled order is indexed with 31 bits, and indptr must not decrease)",
                (long long)nnz);

    // ---- pool, sort every cluster's pool, groups --------------------------------------------------------------------------------
    const auto graw = LP.array<double>(pooled);
    const auto pool_peak = LP.array<int32_t>(pooled), pool_cluster = LP.array<int32_t>(pooled);
    const auto smz = LP.array<float>(pooled), sint = LP.array<float>(pooled), gmz = LP.array<float>(pooled);
    const auto kept = LP.array<uint8_t>(pooled);
    LP.pad(64);
    if (pooled > 0) {
        FAL_TRY(LP.reserve(ctx, SLOT_DB));
        hipLaunchKernelGGL(cons_pool_kernel, grid_for(pooled), dim3(kConsBlock), 0, s, pool_off, key, row, n, pooled, indptr, pool_peak,
                           pool_cluster);
        FAL_CHECK_HIP(hipGetLastError());
        const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nc, (int64_t)ctx->num_cus * 40));
        hipLaunchKernelGGL(cons_sort_lds_kernel, dim3(wgs), dim3(kConsBlock), 0, s, cstart, cpool, nc, pool_peak, mz, intensity, smz, sint);
        FAL_CHECK_HIP(hipGetLastError());
        if (n_big > 0) {
            ScratchLayout LK;
            const auto k0 = LK.array<uint32_t>(n_big), k1 = LK.array<uint32_t>(n_big);
            const auto v0 = LK.array<int32_t>(n_big), v1 = LK.array<int32_t>(n_big);
            FAL_TRY(LK.reserve(ctx, SLOT_DB2));
            hipLaunchKernelGGL(cons_big_keys_kernel, grid_for(n_big), dim3(kConsBlock), 0, s, big_off, cpool, nc, n_big, pool_peak, mz, k0, v0);
            FAL_CHECK_HIP(hipGetLastError());
            ctx->release(SLOT_SORT);
            FAL_TRY(sort_pairs_u32_i32(ctx, k0, k1, v0, v1, n_big, 32, SLOT_SORT));          // by m/z, ties in pooled order
            hipLaunchKernelGGL(cons_big_cluster_keys_kernel, grid_for(n_big), dim3(kConsBlock), 0, s, v1, n_big, pool_cluster, k1);
            FAL_CHECK_HIP(hipGetLastError());
            ctx->release(SLOT_SORT);
            FAL_TRY(sort_pairs_u32_i32(ctx, k1, k0, v1, v0, n_big, bits_for(nc), SLOT_SORT));  // then by cluster: stable
            hipLaunchKernelGGL(cons_big_scatter_kernel, grid_for(n_big), dim3(kConsBlock), 0, s, k0, v0, n_big, big_off, cpool, pool_peak, mz,
                               intensity, smz, sint);
            FAL_CHECK_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(cons_groups_kernel, grid_for(pooled), dim3(kConsBlock), 0, s, pool_cluster, pooled, cstart, cpool, smz, sint,
                           fragment_tol, min_fraction, kept, gmz, graw, kept_count);
        FAL_CHECK_HIP(hipGetLastError());
    }

    // ---- count, scan, emit --------------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(cons_out_counts_kernel, grid_for(nc), dim3(kConsBlock), 0, s, cstart, cpool, big_size, kept_count, medoids, indptr,
                       n, nc, out_count, status_out);
    FAL_CHECK_HIP(hipGetLastError());
    ctx->release(SLOT_SORT2);
    FAL_TRY(device_scan_i64(ctx, out_count, nc, out_indptr, SLOT_SORT2));
    hipLaunchKernelGGL(cons_emit_kernel, grid_for(nc * 64), dim3(kConsBlock), 0, s, cstart, cpool, nc, pool_peak, medoids, indptr, mz,
                       intensity, kept, gmz, graw, out_indptr, nnz_cap, out_mz, out_intensity, status_out);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
