// f4: hierarchical clustering of the (re-scored) neighbour graph -- the clustering the reference snapshot ships:
// `fcluster(fastcluster.linkage(pdist, linkage), distance_threshold, "distance")` on the exact cosine distances of a
// block (reference cluster.py:283-290), here on the sparse neighbour graph with "missing pair = distance 1"
// (the reference's own convention for pairs below min_matched_peaks, cluster.py:621-626).
//
// Cut at a threshold t < 1 a flat cluster can only join spectra of one connected component of the graph of edges with
// d <= t (single: the components themselves; complete / average: a merge across two components has height 1).  So:
//   1. lock-free union-find (unionfind.h) over the stored edges with d <= t (both directions) -> components, root = lowest row;
//   2. single linkage: done.  complete / average: one wave per component of >= 2 rows -- dense matrix of the component
//      (d(i, j) = the smaller of the stored directions, 1 where neither is stored), naive agglomeration with the
//      Lance-Williams update in float64 (scipy's formulas), always merging the pair with the smallest height (ties:
//      lowest (a, b)), until the smallest height exceeds t;
//   3. clusters of one row become noise (-1: the reference's _postprocess_cluster drops groups < 2, cluster.py:441-454),
//      the others are numbered by their lowest row -- the interface of the DBSCAN stage (a9), so a10..a12 follow
//      unchanged.
// fastcluster is not available and scipy's tie order is not specified: PARITY with them stays UNPINNED for exact ties (the
// partition is identical whenever merge heights are distinct; tests/test_gpu_linkage.py against scipy.cluster.hierarchy).
// The order this file states for itself -- smallest height, ties -> lowest (a, b) in the group's ascending-row numbering,
// float64 updates -- IS pinned: tests/linkage_cases.py restates it in numpy, tests/test_gpu_linkage_ties.py holds both
// agglomeration kernels to it on inputs made of ties, label for label.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "ivf.h"
#include "util.h"
#include "peakmatch.h"
#include "unionfind.h"

namespace fal {

// Connected groups of up to kLinkageWaveMax rows are agglomerated one wave per group (O(m^3 / 64): the whole matrix is
// searched for every merge); larger ones by a 1,024-thread workgroup that keeps every row's nearest partner cached
// (`lk_agglomerate_big_kernel`: O(m^2)-ish, the same merges in the same order).  There is no size cap (round 3 refused groups of
// more than 2,048 rows; the reference runs fastcluster on whole blocks of up to batch_size rows, cluster.py:277-290): a group is
// bounded by its bucket, a bucket by batch_size, and the m x m float64 matrix (8.6 GB at 32,768 rows) is the memory the
// reference's own condensed matrix takes twice over.
constexpr int kLinkageWaveMax = 256;

__global__ void lk_init_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ count, int32_t* __restrict__ rep, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        parent[i] = (int32_t)i;
        count[i] = 0;
        rep[i] = -1;
    }
}

__global__ void lk_edges_kernel(const int32_t* __restrict__ nb_idx, const float* __restrict__ nb_dist, int64_t n, int k,
                                float t, int32_t* __restrict__ parent) {
    const int64_t total = n * k;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / k;
        const int32_t j = nb_idx[e];
        if (j >= 0 && (int64_t)j < n && (int64_t)j != i && nb_dist[e] <= t) uf_union<kUfAgent>(parent, (int32_t)i, j);
    }
}

// the same over a symmetric CSR of float64 distances (exact mode: ids in sorted-row space, rows of the CSR = rows here)
__global__ void lk_edges_csr_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const double* __restrict__ dist,
                                    int64_t n, double t, int32_t* __restrict__ parent) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int32_t j = idx[e];
            if (j >= 0 && (int64_t)j < n && (int64_t)j != i && dist[e] <= t) uf_union<kUfAgent>(parent, (int32_t)i, j);
        }
}

__global__ void lk_roots_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ count, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t root = uf_find_final<kUfAgent>(parent, (int32_t)i);
        uf_store<kUfAgent>(&parent[i], root);
        atomicAdd(&count[root], 1);
    }
}

// per row: 1 where the row is the root of a component of >= 2 rows; sizes / squared sizes for the member and matrix offsets
// (+ the list of the components beyond the one-wave form: big[0] = how many, big[1..] = their roots, any order)
__global__ void lk_comp_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ count, int64_t n,
                               int32_t* __restrict__ is_comp, int64_t* __restrict__ msz, int64_t* __restrict__ msq,
                               int32_t* __restrict__ big) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool c = parent[i] == (int32_t)i && count[i] >= 2;
        is_comp[i] = c;
        msz[i] = c ? count[i] : 0;
        msq[i] = c ? (int64_t)count[i] * count[i] : 0;
        if (c && count[i] > kLinkageWaveMax) big[1 + atomicAdd(&big[0], 1)] = (int32_t)i;
    }
}

__global__ void lk_fill_kernel(double* __restrict__ D, int64_t cells) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) D[c] = 1.0;
}

__global__ void lk_scatter_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ count, int64_t n,
                                  const int64_t* __restrict__ moff, int32_t* __restrict__ cursor, int32_t* __restrict__ mem,
                                  const int64_t* __restrict__ comp_rank, int32_t* __restrict__ comp_root) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t root = parent[i];
        if (count[root] < 2) continue;
        mem[moff[root] + atomicAdd(&cursor[root], 1)] = (int32_t)i;
        if (root == (int32_t)i) comp_root[comp_rank[i]] = root;
    }
}

// single linkage: the component is the cluster
__global__ void lk_single_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ count, int64_t n,
                                 int32_t* __restrict__ rep) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        rep[i] = count[parent[i]] >= 2 ? parent[i] : -1;
}

// one wave per component: method 1 = complete, 2 = average
__global__ __launch_bounds__(64) void lk_agglomerate_kernel(const int32_t* __restrict__ nb_idx, const float* __restrict__ nb_dist,
                                                            int64_t n, int k, const int64_t* __restrict__ csr_ptr,
                                                            const int32_t* __restrict__ csr_idx, const double* __restrict__ csr_dist,
                                                            double t, int method, const int32_t* __restrict__ parent,
                                                            const int32_t* __restrict__ count, const int32_t* __restrict__ comp_root,
                                                            const int64_t* __restrict__ moff, const int64_t* __restrict__ qoff,
                                                            const int32_t* __restrict__ mem, int32_t* __restrict__ mem_sorted,
                                                            int32_t* __restrict__ lidx, int32_t* __restrict__ act,
                                                            int32_t* __restrict__ sz, int32_t* __restrict__ cl,
                                                            double* __restrict__ Dall, int32_t* __restrict__ rep) {
    const int lane = threadIdx.x;
    const int32_t root = comp_root[blockIdx.x];
    const int m = count[root];
    if (m > kLinkageWaveMax) return;                        // lk_agglomerate_big_kernel's
    const int64_t mo = moff[root];
    const int32_t* mu = mem + mo;
    int32_t* ms = mem_sorted + mo;
    int32_t* a_act = act + mo;
    int32_t* a_sz = sz + mo;
    int32_t* a_cl = cl + mo;
    double* D = Dall + qoff[root];
    // members in ascending row order (rank by counting); local index of every member row
    for (int x = lane; x < m; x += 64) {
        const int32_t rx = mu[x];
        int rank = 0;
        for (int y = 0; y < m; ++y) rank += mu[y] < rx;
        ms[rank] = rx;
        lidx[rx] = rank;
        a_act[x] = 1;
        a_sz[x] = 1;
        a_cl[x] = x;
    }
    // (D arrives filled with 1.0: missing pair = distance 1, lk_fill_kernel -- or with every exact distance, lk_exact_fill_kernel:
    // then there is no edge source to read)
    __threadfence_block();
    __syncthreads();
    for (int a = 0; a < m; ++a) {
        const int64_t row = ms[a];
        if (csr_ptr) {
            for (int64_t e = csr_ptr[row] + lane; e < csr_ptr[row + 1]; e += 64) {
                const int32_t j = csr_idx[e];
                if (j >= 0 && (int64_t)j < n && (int64_t)j != row && parent[j] == root) D[(int64_t)a * m + lidx[j]] = csr_dist[e];
            }
            continue;
        }
        for (int s = lane; s < k; s += 64) {
            const int32_t j = nb_idx[row * k + s];
            if (j >= 0 && (int64_t)j < n && (int64_t)j != row && parent[j] == root) D[(int64_t)a * m + lidx[j]] = (double)nb_dist[row * k + s];
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int64_t c = lane; c < (int64_t)m * m; c += 64) {                          // d(i, j) = the smaller stored direction
        const int a = (int)(c / m), b = (int)(c % m);
        if (a < b) {
            const double v = fmin(D[c], D[(int64_t)b * m + a]);
            D[c] = v;
            D[(int64_t)b * m + a] = v;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int step = 0; step < m - 1; ++step) {
        double bv = INFINITY;
        int ba = 0x7fffffff, bb = 0x7fffffff;
        for (int a = lane; a < m; a += 64) {
            if (!a_act[a]) continue;
            for (int b = a + 1; b < m; ++b) {
                if (!a_act[b]) continue;
                const double v = D[(int64_t)a * m + b];
                if (v < bv || (v == bv && (a < ba || (a == ba && b < bb)))) {
                    bv = v;
                    ba = a;
                    bb = b;
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oa = __shfl_xor(ba, off, 64), ob = __shfl_xor(bb, off, 64);
            if (ov < bv || (ov == bv && (oa < ba || (oa == ba && ob < bb)))) {
                bv = ov;
                ba = oa;
                bb = ob;
            }
        }
        if (!(bv <= t)) break;                                                      // fcluster(Z, t, "distance")
        const double sa = (double)a_sz[ba], sb = (double)a_sz[bb];
        for (int c = lane; c < m; c += 64) {
            if (!a_act[c] || c == ba || c == bb) continue;
            const double dac = D[(int64_t)ba * m + c], dbc = D[(int64_t)bb * m + c];
            const double nv = method == 1 ? fmax(dac, dbc) : (sa * dac + sb * dbc) / (sa + sb);   // scipy's Lance-Williams forms
            D[(int64_t)ba * m + c] = nv;
            D[(int64_t)c * m + ba] = nv;
        }
        for (int x = lane; x < m; x += 64)
            if (a_cl[x] == bb) a_cl[x] = ba;
        __threadfence_block();
        __syncthreads();
        if (lane == 0) {
            a_act[bb] = 0;
            a_sz[ba] += a_sz[bb];
        }
        __threadfence_block();
        __syncthreads();
    }
    for (int x = lane; x < m; x += 64) {
        const int c = a_cl[x];                              // representative = the cluster's lowest member (a < b in every merge)
        rep[ms[x]] = a_sz[c] >= 2 ? ms[c] : -1;
    }
}


// Groups beyond the one-wave form: one workgroup of 16 waves per group.  The same agglomeration -- always the pair with the
// smallest height, ties -> lowest (a, b), Lance-Williams updates in float64 -- with the search made incremental: every active
// row a keeps its nearest partner among the active b > a (`nnv`, `nni`: smallest value, ties -> lowest b), so the global
// minimum with the (value, a, b) tie order is a reduction over m cached entries; after a merge only the rows whose cached
// partner was one of the merged pair are searched again (a wave per row), the others are updated in place (a new value can
// only tie the cached one: complete and average linkage are reducible, d(a + b, c) >= min(d(a, c), d(b, c))).
// In exact arithmetic the in-place branch below replaces nothing: before the merge D[c][ba] > nnv[c] or nni[c] < ba, the
// same for bb, and a reducible update cannot go below the smaller of the two (the sequential port in tests/linkage_cases.py
// counts zero on heights that are binary fractions or few float32 values).  In float64 it is LIVE: the average of two equal
// heights, (sa * x + sb * x) / (sa + sb), rounds one ulp below x for some sizes (x = 0.04097352393619469, sa = 25, sb = 37),
// which is below the cached nnv[c] = x -- exact mode's cosines and float32 distances after a few unequal means give such
// heights (tests/test_linkage_cpu.py keeps inputs where it fires).  The cache's (value, lowest b) invariant depends on it.
__global__ __launch_bounds__(1024) void lk_agglomerate_big_kernel(const int32_t* __restrict__ nb_idx, const float* __restrict__ nb_dist,
                                                                  int64_t n, int k, const int64_t* __restrict__ csr_ptr,
                                                                  const int32_t* __restrict__ csr_idx, const double* __restrict__ csr_dist,
                                                                  double t, int method, const int32_t* __restrict__ parent,
                                                                  const int32_t* __restrict__ count, const int32_t* __restrict__ big,
                                                                  const int64_t* __restrict__ moff, const int64_t* __restrict__ qoff,
                                                                  const int32_t* __restrict__ mem, int32_t* __restrict__ mem_sorted,
                                                                  int32_t* __restrict__ lidx, int32_t* __restrict__ act,
                                                                  int32_t* __restrict__ sz, int32_t* __restrict__ cl,
                                                                  int32_t* __restrict__ nni_all, int32_t* __restrict__ todo_all,
                                                                  double* __restrict__ nnv_all, double* __restrict__ Dall,
                                                                  int32_t* __restrict__ rep) {
    constexpr int T = 1024, W = T / 64;
    __shared__ double s_v[W];
    __shared__ int32_t s_a[W];
    __shared__ double s_bv;
    __shared__ int32_t s_ba, s_bb, s_ntodo;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int32_t root = big[1 + blockIdx.x];
    const int m = count[root];
    const int64_t mo = moff[root];
    const int32_t* mu = mem + mo;
    int32_t* ms = mem_sorted + mo;
    int32_t* a_act = act + mo;
    int32_t* a_sz = sz + mo;
    int32_t* a_cl = cl + mo;
    int32_t* nni = nni_all + mo;
    int32_t* todo = todo_all + mo;
    double* nnv = nnv_all + mo;
    double* D = Dall + qoff[root];
    auto sync = [&]() {
        __threadfence_block();
        __syncthreads();
    };
    for (int x = tid; x < m; x += T) {                      // members in ascending row order (rank by counting)
        const int32_t rx = mu[x];
        int rank = 0;
        for (int y = 0; y < m; ++y) rank += mu[y] < rx;
        ms[rank] = rx;
        lidx[rx] = rank;
        a_act[x] = 1;
        a_sz[x] = 1;
        a_cl[x] = x;
    }
    sync();
    if (csr_ptr) {                                          // (CSR source: one wave per member row)
        for (int a = w; a < m; a += W) {
            const int64_t row = ms[a];
            for (int64_t e = csr_ptr[row] + lane; e < csr_ptr[row + 1]; e += 64) {
                const int32_t j = csr_idx[e];
                if (j >= 0 && (int64_t)j < n && (int64_t)j != row && parent[j] == root) D[(int64_t)a * m + lidx[j]] = csr_dist[e];
            }
        }
    }
    for (int64_t e = tid; e < (int64_t)m * k; e += T) {     // stored edges inside the group (D arrives filled with 1.0)
        const int a = (int)(e / k), s = (int)(e % k);
        const int64_t row = ms[a];
        const int32_t j = nb_idx[row * k + s];
        if (j >= 0 && (int64_t)j < n && (int64_t)j != row && parent[j] == root) D[(int64_t)a * m + lidx[j]] = (double)nb_dist[row * k + s];
    }
    sync();
    for (int64_t c = tid; c < (int64_t)m * m; c += T) {     // d(i, j) = the smaller stored direction
        const int a = (int)(c / m), b = (int)(c % m);
        if (a < b) {
            const double v = fmin(D[c], D[(int64_t)b * m + a]);
            D[c] = v;
            D[(int64_t)b * m + a] = v;
        }
    }
    sync();
    // nearest active partner b > a of row a: smallest value, ties -> lowest b (one wave per row)
    auto search_row = [&](int a) {
        double bv = INFINITY;
        int bb = 0x7fffffff;
        const double* Da = D + (int64_t)a * m;
        for (int b = a + 1 + lane; b < m; b += 64) {
            if (!a_act[b]) continue;
            const double v = Da[b];
            if (v < bv) {                                   // (b ascends inside a lane: "<" keeps the lowest b)
                bv = v;
                bb = b;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int ob = __shfl_xor(bb, off, 64);
            if (ov < bv || (ov == bv && ob < bb)) {
                bv = ov;
                bb = ob;
            }
        }
        if (lane == 0) {
            nnv[a] = bv;
            nni[a] = bb;
        }
    };
    for (int a = w; a < m; a += W) search_row(a);
    sync();
    for (int step = 0; step < m - 1; ++step) {
        double bv = INFINITY;
        int ba = 0x7fffffff;
        for (int a = tid; a < m; a += T) {
            if (!a_act[a]) continue;
            const double v = nnv[a];
            if (v < bv) {                                   // (a ascends inside a thread)
                bv = v;
                ba = a;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oa = __shfl_xor(ba, off, 64);
            if (ov < bv || (ov == bv && oa < ba)) {
                bv = ov;
                ba = oa;
            }
        }
        if (lane == 0) {
            s_v[w] = bv;
            s_a[w] = ba;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < W; ++i)
                if (s_v[i] < bv || (s_v[i] == bv && s_a[i] < ba)) {
                    bv = s_v[i];
                    ba = s_a[i];
                }
            s_bv = bv;
            s_ba = ba;
            s_bb = ba < m ? nni[ba] : 0x7fffffff;
            s_ntodo = 0;
        }
        __syncthreads();
        bv = s_bv;
        ba = s_ba;
        const int bb = s_bb;
        if (!(bv <= t)) break;                              // fcluster(Z, t, "distance")
        const double sa = (double)a_sz[ba], sb = (double)a_sz[bb];
        for (int c = tid; c < m; c += T) {
            if (a_cl[c] == bb) a_cl[c] = ba;
            if (!a_act[c] || c == ba || c == bb) continue;
            const double dac = D[(int64_t)ba * m + c], dbc = D[(int64_t)bb * m + c];
            const double nv = method == 1 ? fmax(dac, dbc) : (sa * dac + sb * dbc) / (sa + sb);   // scipy's Lance-Williams forms
            D[(int64_t)ba * m + c] = nv;
            D[(int64_t)c * m + ba] = nv;
            if (c < bb) {                                   // rows above bb never had ba or bb among their partners b > c
                const int32_t p = nni[c];
                if (p == bb || (p == ba && c < ba)) todo[atomicAdd(&s_ntodo, 1)] = c;
                else if (c < ba && (nv < nnv[c] || (nv == nnv[c] && ba < p))) {
                    nnv[c] = nv;
                    nni[c] = ba;
                }
            }
        }
        sync();
        if (tid == 0) {
            a_act[bb] = 0;
            a_sz[ba] += a_sz[bb];
            todo[s_ntodo++] = ba;
        }
        sync();
        const int nt = s_ntodo;
        for (int i = w; i < nt; i += W) search_row(todo[i]);
        sync();
    }
    for (int x = tid; x < m; x += T) {
        const int c = a_cl[x];                              // representative = the cluster's lowest member (a < b in every merge)
        rep[ms[x]] = a_sz[c] >= 2 ? ms[c] : -1;
    }
}

// exact mode, average linkage: the matrix of a component holds the exact distance of EVERY member pair (heights above t enter
// the Lance-Williams averages).  Members in ascending row order first (the agglomeration kernels rank them the same way again).
__global__ __launch_bounds__(64) void lk_rank_kernel(const int32_t* __restrict__ comp_root, const int32_t* __restrict__ count,
                                                     const int64_t* __restrict__ moff, const int32_t* __restrict__ mem,
                                                     int32_t* __restrict__ mem_sorted) {
    const int32_t root = comp_root[blockIdx.x];
    const int m = count[root];
    const int32_t* mu = mem + moff[root];
    for (int x = threadIdx.x; x < m; x += 64) {
        const int32_t rx = mu[x];
        int rank = 0;
        for (int y = 0; y < m; ++y) rank += mu[y] < rx;
        mem_sorted[moff[root] + rank] = rx;
    }
}

// one thread per matrix cell of every component (cells of component c: qoff[comp_root[c]] ..); the lower row of a pair is the
// query spectrum, as in the reference's condensed matrix (cluster.py:593-639: cosine_fast(i, j) for i < j)
__global__ __launch_bounds__(256) void lk_exact_fill_kernel(int64_t n_comp, const int32_t* __restrict__ comp_root,
                                                            const int32_t* __restrict__ count, const int64_t* __restrict__ moff,
                                                            const int64_t* __restrict__ qoff, const int32_t* __restrict__ mem_sorted,
                                                            int64_t n_sq, ExactPeaks pk, double* __restrict__ Dall) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_sq; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n_comp - 1;                    // the last component whose first cell is <= c
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (qoff[comp_root[mid]] <= c) lo = mid;
            else hi = mid - 1;
        }
        const int32_t root = comp_root[lo];
        const int m = count[root];
        const int64_t q = c - qoff[root];
        const int a = (int)(q / m), b = (int)(q % m);
        double* D = Dall + qoff[root];
        if (a == b) D[q] = 0.0;
        if (a >= b) continue;
        const int32_t* ms = mem_sorted + moff[root];
        bool ok = true;
        const double d = exact_distance(pk, ms[a], ms[b], &ok);
        if (!ok) atomicExch(pk.err, 1);
        D[(int64_t)a * m + b] = d;
        D[(int64_t)b * m + a] = d;
    }
}

__global__ void lk_isrep_kernel(const int32_t* __restrict__ rep, int64_t n, int32_t* __restrict__ is_rep) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        is_rep[i] = rep[i] == (int32_t)i;
}

__global__ void lk_label_kernel(const int32_t* __restrict__ rep, const int64_t* __restrict__ rank, int64_t n,
                                int32_t* __restrict__ labels) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        labels[i] = rep[i] >= 0 ? (int32_t)rank[rep[i]] : -1;
}

// labels + cluster count on the device (the interface of dbscan_dev); synchronises once for the scratch sizes of the
// complete / average forms
int linkage_dev_src(fal_ctx* ctx, const LinkageSource& src, int64_t n, double t, int method, int32_t* labels,
                    int64_t** d_count_out) {
    const int32_t* nb_idx = src.nb_idx;
    const float* nb_dist = src.nb_dist;
    const int k = src.csr_ptr || src.exact_fill ? 0 : src.k;
    hipStream_t st = ctx->stream;
    int64_t* rank = nullptr;
    ScratchLayout L;
    const auto parent = L.array<int32_t>(n), count = L.array<int32_t>(n), rep = L.array<int32_t>(n), flag = L.array<int32_t>(n);
    FAL_TRY(L.reserve(ctx, SLOT_DB));
    FAL_TRY(ctx->reserve(SLOT_DB2, sizeof(int64_t) * (size_t)(n + 1), (void**)&rank));
    const int grid = (int)std::min<int64_t>(ceil_div(n, 256), (int64_t)ctx->num_cus * 16);
    const int egrid = (int)std::min<int64_t>(ceil_div(n * src.k, 256), (int64_t)ctx->num_cus * 32);
    ctx->stage_reset(ST_DBSCAN);
    StageScope ts(ctx, ST_DBSCAN);
    hipLaunchKernelGGL(lk_init_kernel, dim3(grid), dim3(256), 0, st, parent, count, rep, n);
    if (src.csr_ptr)
        hipLaunchKernelGGL(lk_edges_csr_kernel, dim3(grid), dim3(256), 0, st, src.csr_ptr, src.csr_idx, src.csr_dist, n, t, parent);
    else
        hipLaunchKernelGGL(lk_edges_kernel, dim3(egrid), dim3(256), 0, st, nb_idx, nb_dist, n, src.k, (float)t, parent);
    hipLaunchKernelGGL(lk_roots_kernel, dim3(grid), dim3(256), 0, st, parent, count, n);
    if (method == 0) {
        hipLaunchKernelGGL(lk_single_kernel, dim3(grid), dim3(256), 0, st, parent, count, n, rep);
    } else {
        ScratchLayout LT, LT2;
        const auto msz = LT.array<int64_t>(n + 1), msq = LT.array<int64_t>(n + 1), moff = LT.array<int64_t>(n + 1), qoff = LT.array<int64_t>(n + 1);
        FAL_TRY(LT.reserve(ctx, SLOT_TAIL));
        const int64_t big_cap = n / kLinkageWaveMax + 2;    // components of more than kLinkageWaveMax rows: at most n / that many
        const auto crank = LT2.array<int64_t>(n + 1);       // (the n + 1 words of the scan)
        const auto big = LT2.array<int32_t>(big_cap + 2);
        FAL_TRY(LT2.reserve(ctx, SLOT_TAIL2));
        FAL_CHECK_HIP(hipMemsetAsync(big, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(lk_comp_kernel, dim3(grid), dim3(256), 0, st, parent, count, n, flag, msz, msq, big);
        FAL_TRY(device_scan_i32(ctx, flag, n, crank, SLOT_DB3));
        FAL_TRY(device_scan_i64(ctx, msz, n, moff, SLOT_DB3));
        FAL_TRY(device_scan_i64(ctx, msq, n, qoff, SLOT_DB3));
        int64_t tot[3] = {0, 0, 0};
        int32_t n_big = 0;
        FAL_CHECK_HIP(hipMemcpyAsync(&n_big, big, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipMemcpyAsync(&tot[0], crank + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipMemcpyAsync(&tot[1], moff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipMemcpyAsync(&tot[2], qoff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        const int64_t n_comp = tot[0], n_mem = tot[1], n_sq = tot[2];
        if (n_comp > 0) {
            ScratchLayout LT3, LT4;
            const auto mem = LT3.array<int32_t>(n_mem), mem_sorted = LT3.array<int32_t>(n_mem), act = LT3.array<int32_t>(n_mem);
            const auto sz = LT3.array<int32_t>(n_mem), cl = LT3.array<int32_t>(n_mem), nni = LT3.array<int32_t>(n_mem), todo = LT3.array<int32_t>(n_mem);
            const auto lidx = LT3.array<int32_t>(n), cursor = LT3.array<int32_t>(n), comp_root = LT3.array<int32_t>(n_comp);
            LT3.pad(64);
            FAL_TRY(LT3.reserve(ctx, SLOT_TAIL3));
            const auto D = LT4.array<double>(n_sq), nnv = LT4.array<double>(n_mem);
            LT4.pad(128);
            const int rc = LT4.reserve(ctx, SLOT_TAIL4);
            if (rc != FAL_OK) {
                set_error("hierarchical clustering (complete / average): the connected groups within the distance threshold need "
                          "%.1f GB of pair distances (sum of squared group sizes %lld); single linkage or DBSCAN take the same graph",
                          8e-9 * (double)n_sq, (long long)n_sq);
                return rc;
            }
            FAL_CHECK_HIP(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)n, st));
            const unsigned qgrid = (unsigned)std::min<int64_t>(ceil_div(n_sq, 256), (int64_t)ctx->num_cus * 32);
            hipLaunchKernelGGL(lk_scatter_kernel, dim3(grid), dim3(256), 0, st, parent, count, n, moff, cursor, mem, crank, comp_root);
            const int64_t* cp = src.csr_ptr;
            if (src.exact_fill) {                           // every member pair scored again (average linkage of exact mode)
                hipLaunchKernelGGL(lk_rank_kernel, dim3((unsigned)n_comp), dim3(64), 0, st, comp_root, count, moff, mem, mem_sorted);
                hipLaunchKernelGGL(lk_exact_fill_kernel, dim3(qgrid), dim3(256), 0, st, n_comp, comp_root, count, moff, qoff, mem_sorted,
                                   n_sq, src.peaks, D);
                cp = nullptr;
            } else {
                hipLaunchKernelGGL(lk_fill_kernel, dim3(qgrid), dim3(256), 0, st, D, n_sq);
            }
            hipLaunchKernelGGL(lk_agglomerate_kernel, dim3((unsigned)n_comp), dim3(64), 0, st, nb_idx, nb_dist, n, k, cp, src.csr_idx,
                               src.csr_dist, t, method, parent, count, comp_root, moff, qoff, mem, mem_sorted, lidx, act, sz, cl, D, rep);
            if (n_big > 0)
                hipLaunchKernelGGL(lk_agglomerate_big_kernel, dim3((unsigned)n_big), dim3(1024), 0, st, nb_idx, nb_dist, n, k, cp,
                                   src.csr_idx, src.csr_dist, t, method, parent, count, big, moff, qoff, mem, mem_sorted, lidx, act, sz,
                                   cl, nni, todo, nnv, D, rep);
        }
    }
    hipLaunchKernelGGL(lk_isrep_kernel, dim3(grid), dim3(256), 0, st, rep, n, flag);
    FAL_TRY(device_scan_i32(ctx, flag, n, rank, SLOT_DB3));
    hipLaunchKernelGGL(lk_label_kernel, dim3(grid), dim3(256), 0, st, rep, rank, n, labels);
    FAL_CHECK_HIP(hipGetLastError());
    *d_count_out = rank + n;
    // the agglomeration's work arrays are dead on the host side (their kernels are enqueued): the tail stage reuses the slots
    for (int slot : {SLOT_TAIL, SLOT_TAIL2, SLOT_TAIL3, SLOT_TAIL4, SLOT_DB3}) ctx->release(slot);
    return FAL_OK;
}

int linkage_dev(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k, float t, int method,
                int32_t* labels, int64_t** d_count_out) {
    LinkageSource src;
    src.nb_idx = nb_idx;
    src.nb_dist = nb_dist;
    src.k = k;
    return linkage_dev_src(ctx, src, n, (double)t, method, labels, d_count_out);
}

}  // namespace fal
FAL_WARM_KERNEL(fal::lk_init_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_linkage_cluster(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k, float threshold,
                                   int method, int32_t* labels, int64_t* n_clusters) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n >= 0 && k >= 1 && n < (int64_t)INT32_MAX, FAL_EINVAL, "fal_linkage_cluster: bad argument");
    FAL_REQUIRE(method >= 0 && method <= 2, FAL_EINVAL, "fal_linkage_cluster: method must be 0 (single), 1 (complete) or 2 (average)");
    FAL_REQUIRE(threshold < 1.0f, FAL_EUNSUPPORTED, "fal_linkage_cluster: the threshold must be below 1 (the distance of a missing pair)");
    if (n_clusters) *n_clusters = 0;
    if (n == 0) return FAL_OK;
    FAL_REQUIRE(nb_idx && nb_dist && labels, FAL_EINVAL, "fal_linkage_cluster: NULL array");
    int64_t* d_count = nullptr;
    FAL_TRY(linkage_dev(ctx, nb_idx, nb_dist, n, k, threshold, method, labels, &d_count));
    if (n_clusters) {
        FAL_CHECK_HIP(hipMemcpyAsync(n_clusters, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return FAL_OK;
}
