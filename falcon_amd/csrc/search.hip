// a7: n_probe search of every row against its bucket's index, top-k_ann by (sim desc, id asc).
//
// Flat buckets (one list): dense tile scan of the bucket against itself + wavefront select.
// IVF buckets: coarse quantiser (dense scan vs the bucket's centroids + select k = n_probe),
// candidate-count prefix, fine scan over the union of probed lists, select.
// The sims of a batch of buckets live in one scratch buffer (default 2 GiB, FALCON_SIMS_MB): big
// enough that a launch holds many tiles per wave slot (short launches lose more to their tail than
// the buffer's HBM round trip costs; measured 160 MiB: 4.5 ms, 1 GiB: 3.5 ms of scan at 1 M spectra).
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "common.h"
#include "scan.h"
#include "ivf.h"
#include "util.h"
#include "fused.h"
#include "ivf16.h"
#include "coarse16.h"

namespace fal {

// total candidates of each query = sum of the sizes of its probed lists (0 where probes are -1),
// stored at the query's TILE-ORDER slot 32 * tile + lane (unused lanes of a last tile stay 0)
template <int NPV>      // probes per query / 4 loaded as 16-byte pieces in front of the list-size gathers (0: any n_probe)
__global__ void probe_totals_kernel(const int32_t* __restrict__ probes, int np, const DenseJob* __restrict__ jobs,
                                    int n_jobs, int64_t n_tiles, const int64_t* __restrict__ list_off,
                                    int64_t* __restrict__ totals) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t t = g >> 5;
    int64_t tot = 0;
    if (t < n_tiles) {
        const DenseJob job = jobs[find_job(jobs, n_jobs, t)];
        const int lt = (int)(t - job.tile0), ql = (int)(g & 31);
        if (32 * lt + ql < job.nq) {
            const int64_t p = job.q_row0 + 32 * (int64_t)lt + ql;
            const int64_t* lo = list_off + job.c_row0;
            if (NPV > 0) {
                int4 pr[NPV > 0 ? NPV : 1];
                const int4* src = reinterpret_cast<const int4*>(probes + p * np);
#pragma unroll
                for (int v = 0; v < NPV; ++v) pr[v] = src[v];
                int64_t part[NPV > 0 ? 4 * NPV : 1];
#pragma unroll
                for (int v = 0; v < NPV; ++v) {
                    const int l[4] = {pr[v].x, pr[v].y, pr[v].z, pr[v].w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) part[4 * v + c] = l[c] >= 0 ? lo[l[c] + 1] - lo[l[c]] : 0;
                }
#pragma unroll
                for (int j = 0; j < 4 * NPV; ++j) tot += part[j];
            } else {
                for (int j = 0; j < np; ++j) {
                    const int l = probes[p * np + j];
                    if (l >= 0) tot += lo[l + 1] - lo[l];
                }
            }
            totals[g] = tot;      // slot g = 32 * tile + lane (tile order, padded)
        }
    }
    // the largest candidate count of the launch, behind the padded slots (one atomic per wave)
    int64_t m = tot;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (int64_t)__shfl_xor((long long)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(reinterpret_cast<unsigned long long*>(totals + 32 * n_tiles + 1), (unsigned long long)m);
}

// ---- inverted probe table: for every list, the queries that probe it ---------------------------
__global__ void probe_hist_kernel(const int32_t* __restrict__ probes, int np, const DenseJob* __restrict__ jobs,
                                  int n_jobs, int64_t n_tiles, int32_t* __restrict__ cnt) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t t = g >> 5;
    if (t >= n_tiles) return;
    const DenseJob job = jobs[find_job(jobs, n_jobs, t)];
    const int lt = (int)(t - job.tile0), ql = (int)(g & 31);
    if (32 * lt + ql >= job.nq) return;
    const int64_t p = job.q_row0 + 32 * (int64_t)lt + ql;
    for (int j = 0; j < np; ++j) {
        const int l = probes[p * np + j];
        if (l >= 0) atomicAdd(&cnt[job.c_row0 + l], 1);
    }
}

// tiles of a list = groups of 2^shift rows of the LIST (each streams all queries probing the list); a list
// nobody probes needs none
__global__ void list_tiles_kernel(const int32_t* __restrict__ cnt, const int64_t* __restrict__ list_off, int64_t n,
                                  int shift, int32_t* __restrict__ tiles) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rows = list_off[i + 1] - list_off[i];
        tiles[i] = (cnt[i] > 0 && rows > 0) ? (int32_t)((rows + (1 << shift) - 1) >> shift) : 0;
    }
}

// inv_q[e] = query position, inv_dest[e] = where that query's sims for this list start
// (= its sims offset + the sizes of the lists it probes before this one)
__global__ void probe_scatter_kernel(const int32_t* __restrict__ probes, int np, const DenseJob* __restrict__ jobs,
                                     int n_jobs, int64_t n_tiles, const int64_t* __restrict__ list_off,
                                     const int64_t* __restrict__ q_sim_off, const int64_t* __restrict__ inv_off,
                                     int32_t* __restrict__ cursor, int32_t* __restrict__ inv_q,
                                     int64_t* __restrict__ inv_dest) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t t = g >> 5;
    if (t >= n_tiles) return;
    const DenseJob job = jobs[find_job(jobs, n_jobs, t)];
    const int lt = (int)(t - job.tile0), ql = (int)(g & 31);
    if (32 * lt + ql >= job.nq) return;
    const int64_t p = job.q_row0 + 32 * (int64_t)lt + ql;
    int64_t dest = q_sim_off[g];
    for (int j = 0; j < np; ++j) {
        const int l = probes[p * np + j];
        if (l < 0) continue;
        const int64_t G = job.c_row0 + l;
        const int64_t e = inv_off[G] + atomicAdd(&cursor[G], 1);
        inv_q[e] = (int32_t)p;
        inv_dest[e] = dest;
        dest += list_off[G + 1] - list_off[G];
    }
}

// entries per list (the histogram of the probe table), one workgroup per bucket with the counters in LDS
__global__ __launch_bounds__(1024) void probe_hist_bucket_kernel(const int32_t* __restrict__ probes, int np,
                                                                 const DenseJob* __restrict__ jobs, int32_t* __restrict__ cnt) {
    extern __shared__ int32_t hist[];
    const DenseJob job = jobs[blockIdx.x];
    const int nl = job.nc;
    for (int i = threadIdx.x; i < nl; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t e = threadIdx.x; e < (int64_t)job.nq * np; e += blockDim.x) {
        const int l = probes[job.q_row0 * np + e];
        if (l >= 0) atomicAdd(&hist[l], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nl; i += blockDim.x) cnt[job.c_row0 + i] = hist[i];
}

// probe_hist_bucket_kernel + probe_totals_kernel in one pass over the probes (round 5; buckets of up to 4,096 lists): a thread per
// query, the bucket's list sizes and the histogram in LDS -- a query's candidate total is the sum of its probed lists' sizes
// (16 LDS reads instead of 32 dependent 8-byte gathers from global memory), stored at its tile-order slot; the launch's largest
// total behind the padded slots as probe_totals_kernel leaves it.
template <int NPV>
__global__ __launch_bounds__(1024) void probe_hist_totals_bucket_kernel(const int32_t* __restrict__ probes, int np,
                                                                        const DenseJob* __restrict__ jobs,
                                                                        const int64_t* __restrict__ list_off, int64_t n_tiles,
                                                                        int32_t* __restrict__ cnt, int64_t* __restrict__ totals) {
    extern __shared__ int32_t lds32[];
    const DenseJob job = jobs[blockIdx.x];
    const int nl = job.nc;
    int32_t* hist = lds32;                // [nl]
    int32_t* len = lds32 + nl;            // [nl] rows of every list
    for (int i = threadIdx.x; i < nl; i += blockDim.x) {
        hist[i] = 0;
        len[i] = (int32_t)(list_off[job.c_row0 + i + 1] - list_off[job.c_row0 + i]);
    }
    __syncthreads();
    int64_t mx = 0;
    for (int ql = threadIdx.x; ql < job.nq; ql += blockDim.x) {
        const int64_t p = job.q_row0 + ql;
        int64_t tot = 0;
        auto take = [&](int l) {
            if (l < 0) return;
            atomicAdd(&hist[l], 1);
            tot += len[l];
        };
        if (NPV > 0) {
            int4 pr[NPV > 0 ? NPV : 1];
            const int4* src = reinterpret_cast<const int4*>(probes + p * np);
#pragma unroll
            for (int v = 0; v < NPV; ++v) pr[v] = src[v];
#pragma unroll
            for (int v = 0; v < NPV; ++v) { take(pr[v].x); take(pr[v].y); take(pr[v].z); take(pr[v].w); }
        } else {
            for (int j = 0; j < np; ++j) take(probes[p * np + j]);
        }
        totals[32 * (job.tile0 + (ql >> 5)) + (ql & 31)] = tot;
        mx = max(mx, tot);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (int64_t)__shfl_xor((long long)mx, off, 64));
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(reinterpret_cast<unsigned long long*>(totals + 32 * n_tiles + 1), (unsigned long long)mx);
    __syncthreads();
    for (int i = threadIdx.x; i < nl; i += blockDim.x) cnt[job.c_row0 + i] = hist[i];
}

// The same table with every list's entries in ASCENDING QUERY ORDER (to within one chunk of 1,024 queries): one workgroup per
// bucket walks the bucket's queries chunk by chunk, cursors in LDS.  The fine-scan kernels stream a list's queries in table
// order; the ~64 lists of a bucket that run concurrently on an XCD then sweep the bucket's rows together and share them in L2
// (with the arrival order of global atomics the gathers came from HBM: 4.2 TB/s for 128 GB at 10 M spectra).
// Nothing the scatter of a query needs is loaded inside its probe loop: the bucket's list sizes and table offsets sit in LDS,
// the query's probes arrive as 16-byte pieces before the first of them is used (the first version paid three dependent global
// round trips per probe: probe -> list_off pair / inv_off, 32 times per query and chunk).
template <int NPV>      // probes per query / 4 held in registers (0: any n_probe, the plain loop)
__global__ __launch_bounds__(1024) void probe_scatter_bucket_kernel(const int32_t* __restrict__ probes, int np,
                                                                    const DenseJob* __restrict__ jobs,
                                                                    const int64_t* __restrict__ list_off,
                                                                    const int64_t* __restrict__ q_sim_off,
                                                                    const int64_t* __restrict__ inv_off, int32_t* __restrict__ inv_q,
                                                                    int64_t* __restrict__ inv_dest, const int32_t* __restrict__ perm,
                                                                    int32_t* __restrict__ inv_row, int lds_lists) {
    extern __shared__ int64_t lds64[];
    const DenseJob job = jobs[blockIdx.x];
    const int nl = job.nc;
    // lds_lists >= the launch's largest list count: 12 bytes of LDS per list (table position + size); otherwise (buckets with
    // thousands of lists: 12 bytes each would not fit) only a 4-byte cursor per list, offsets and sizes from global memory
    const bool full = nl <= lds_lists;
    int64_t* at = lds64;                                     // [nl] where the list's next table entry goes
    int32_t* len = reinterpret_cast<int32_t*>(lds64 + (full ? nl : 0));   // [nl] rows of the list | (else) entries written so far
    for (int i = threadIdx.x; i < nl; i += blockDim.x) {
        if (full) {
            const int64_t b = list_off[job.c_row0 + i], e = list_off[job.c_row0 + i + 1];
            len[i] = (int32_t)(e - b);
            at[i] = inv_off[job.c_row0 + i];
        } else {
            len[i] = 0;
        }
    }
    __syncthreads();
    for (int q0 = 0; q0 < job.nq; q0 += blockDim.x) {
        const int ql = q0 + threadIdx.x;
        if (ql < job.nq) {
            const int64_t p = job.q_row0 + ql;
            int64_t dest = q_sim_off[32 * (job.tile0 + (ql >> 5)) + (ql & 31)];
            const int32_t row = inv_row ? perm[p] : 0;       // (the f16 list scan gathers its queries by sorted row)
            auto put = [&](int l) {
                if (l < 0) return;
                int64_t e;
                int32_t rows;
                if (full) {
                    e = (int64_t)atomicAdd(reinterpret_cast<unsigned long long*>(&at[l]), 1ull);
                    rows = len[l];
                } else {
                    const int64_t G = job.c_row0 + l;
                    e = inv_off[G] + atomicAdd(&len[l], 1);
                    rows = (int32_t)(list_off[G + 1] - list_off[G]);
                }
                inv_q[e] = (int32_t)p;
                inv_dest[e] = dest;
                if (inv_row) inv_row[e] = row;
                dest += rows;
            };
            if (NPV > 0) {
                int4 pr[NPV > 0 ? NPV : 1];
                const int4* src = reinterpret_cast<const int4*>(probes + p * np);
#pragma unroll
                for (int v = 0; v < NPV; ++v) pr[v] = src[v];
#pragma unroll
                for (int v = 0; v < NPV; ++v) { put(pr[v].x); put(pr[v].y); put(pr[v].z); put(pr[v].w); }
            } else {
                for (int j = 0; j < np; ++j) put(probes[p * np + j]);
            }
        }
        __syncthreads();                                     // chunk after chunk: the order inside a list follows the queries
    }
}

// lists per bucket up to which the probe table kernel keeps 12 bytes per list in LDS (48 KB)
static int probe_lds_lists() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("FALCON_PROBE_LDS_LISTS");
        v = e ? std::max(0, std::min(4096, atoi(e))) : 4096;
    }
    return v;
}

size_t sims_mb_env() {
    const char* e = getenv("FALCON_SIMS_MB");
    return e ? (size_t)atoll(e) : 2048;
}

size_t ckeys_mb_env() {
    const char* e = getenv("FALCON_CKEYS_MB");
    return e ? (size_t)atoll(e) : 32768;
}

static size_t sims_capacity_floats() {
    static const size_t cap = sims_cap_floats(sims_mb_env());      // (read once per process)
    return cap;
}

static int dense1_max_env() {
    static const int v = [] {
        const char* e = getenv("FALCON_DENSE1_MAX");
        return e ? atoi(e) : 0;
    }();
    return v;
}

// fine-scan tiles: groups of four 32-row list slices for the 4-wave shared-stream kernels (ivf_fine.hip, ivf16.hip)
constexpr int kGroupShift = 7;

}  // namespace fal
FAL_WARM_KERNEL(fal::probe_totals_kernel<4>);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

namespace {
struct NeighborFilter {          // a8 fused into the final selection (scan.h SelectArgs::nb_idx)
    const float* pmz;
    const float* rt;
    double tol, rt_tol;
    int is_da, keep;
    int32_t* nb_idx;
    float* nb_dist;
    int32_t* nb_count;
};

void set_filter(SelectArgs& sa, const NeighborFilter* nf) {
    if (!nf) return;
    sa.f_pmz = nf->pmz; sa.f_rt = nf->rt; sa.f_tol = nf->tol; sa.f_rt_tol = nf->rt_tol;
    sa.f_is_da = nf->is_da; sa.f_keep = nf->keep; sa.nb_idx = nf->nb_idx; sa.nb_dist = nf->nb_dist;
    sa.nb_count = nf->nb_count;
}
void set_filter(FusedArgs& fa, const NeighborFilter* nf) {
    fa.pmz = nf->pmz; fa.rt = nf->rt; fa.tol = nf->tol; fa.rt_tol = nf->rt_tol; fa.is_da = nf->is_da;
    fa.keep = nf->keep; fa.nb_idx = nf->nb_idx; fa.nb_dist = nf->nb_dist; fa.nb_count = nf->nb_count;
}

// f(std::integral_constant<int, NPV>): the probe kernels' template pick -- 16 / 32 probes per query arrive as 4 / 8 16-byte
// pieces, any other count takes the plain loop (NPV 0)
template <class F>
void with_np_vec(int np, F&& f) {
    if (np == 16) f(std::integral_constant<int, 4>());
    else if (np == 32) f(std::integral_constant<int, 8>());
    else f(std::integral_constant<int, 0>());
}

struct Search {                  // one call: what every step reads
    fal_ctx* ctx;
    const fal_ivf* ivf;
    int k_ann;
    float* sim;                  // [n, k_ann] top-k, or ...
    int32_t* idx;
    const NeighborFilter* nf;    // ... the neighbour lists
    size_t cap;                  // floats of the hand-off buffer a batch may fill
};
struct Probes {                  // run_coarse -> build_probe_table, the fine scans
    int np;                      // probes per query
    int32_t* probes;             // [n, np] bucket-local list ids by list-order position (-1 = none)
    int64_t n_slots;             // tile-order query slots: 32 per IVF tile
    int64_t* totals;             // [n_slots + 2] zeroed: candidates of every slot, the largest of them in the last word
    int64_t* q_sim_off;          // [n_slots + 1] their prefix (build_probe_table fills it)
};
struct ProbeTable {              // build_probe_table -> the fine scans
    int64_t *inv_off, *ltile_off;        // [total_lists + 1] entries / tiles of every list, prefix
    int32_t* inv_q;                      // [pairs] query position
    int64_t* inv_dest;                   // [pairs] where that query's sims for this list start
    int32_t* inv_row;                    // [pairs] the query's sorted row, or nullptr (no f16 list scan can follow)
    int64_t* q_sim_off;
    std::vector<int64_t> qoff, lt_host;  // host: q_sim_off of every tile's first slot (+ the end), ltile_off
    int64_t max_total;                   // the most candidates any query has
};
}  // namespace

// Flat buckets with the top-k kept on chip (fused.hip)
static int run_fused_flat(const Search& s, const std::vector<int64_t>& order) {
    fal_ctx* ctx = s.ctx;
    const fal_ivf* ivf = s.ivf;
    const FusedFlatPlan p = plan_fused_flat(order, ivf->bucket_off.data(), s.k_ann);
    DenseJob* jd = nullptr;
    FAL_TRY(ctx->reserve(SLOT_JOBS, sizeof(DenseJob) * (p.j32.size() + p.j128.size() + 1), (void**)&jd));
    FAL_TRY(ctx->upload(jd, p.j32.data(), sizeof(DenseJob) * p.j32.size()));
    if (!p.j128.empty()) FAL_TRY(ctx->upload(jd + p.j32.size(), p.j128.data(), sizeof(DenseJob) * p.j128.size()));
    FusedArgs fa{};
    fa.X = ivf->X; fa.X16 = reinterpret_cast<const __half*>(ivf->Xpre);
    fa.jobs32 = jd; fa.n_jobs32 = (int)p.j32.size(); fa.jobs128 = jd + p.j32.size(); fa.n_jobs128 = (int)p.j128.size();
    fa.k = s.k_ann;
    set_filter(fa, s.nf);
    FAL_TRY(launch_fused(ctx, fa, ivf->d, ivf->n, p.list_tiles128, p.list_tiles32, p.j32[0].nc));
    ctx->counters[0] = p.pairs;
    ctx->counters[4] = 0;
    ctx->counters[2] = 1;
    ctx->counters[3] = 0;
    return FAL_OK;
}

// A. flat buckets through the hand-off buffer: per batch the scans of its four kernel classes, then the select
static int run_flat_batches(const Search& s, const FlatPlan& flat, const FlatRule& rule, const DenseJob* flat_dev, float* sims,
                            size_t sims_floats) {
    fal_ctx* ctx = s.ctx;
    const fal_ivf* ivf = s.ivf;
    const int d = ivf->d;
    for (const FlatBatch& fb : flat.batches) {
        if (fb.jm > fb.j0)
            FAL_TRY(launch_scan16(ctx, ivf->x16_planes, ivf->X16, d, flat_dev + fb.j0, (int)(fb.jm - fb.j0), fb.list_tiles16, sims, 0,
                                  sims + sims_floats));
        // (flat buckets keep their rows' positions in list order: the sorted rows serve)
        if (fb.js > fb.jm)
            FAL_TRY(launch_dense4(ctx, ivf->X, d, flat_dev + fb.jm, flat.jobs.data() + fb.jm, (int)(fb.js - fb.jm), sims, 0));
        if (fb.jk > fb.js)
            FAL_TRY(launch_dense(ctx, ST_SCAN, EPI_STORE, ivf->X, ivf->X, d, flat_dev + fb.js, (int)(fb.jk - fb.js), 0, fb.tiles, sims, 0,
                                 nullptr, fb.list_tiles1));
        const int n_one = (int)(fb.j1 - fb.jk);
        const FlatKernel one = flat_one_block_kernel(rule);
        if (n_one > 0 && one == FLAT_EXACT_SMALL)
            FAL_TRY(launch_flat_exact_small(ctx, ivf->X, d, flat_dev + fb.jk, n_one, sims, 0));
        else if (n_one > 0 && one == FLAT_TINY4)
            FAL_TRY(launch_dense_tiny4(ctx, ivf->X, d, flat_dev + fb.jk, n_one, sims, 0));
        else if (n_one > 0)
            FAL_TRY(launch_dense(ctx, ST_SCAN, EPI_STORE, ivf->X, ivf->X, d, flat_dev + fb.jk, n_one, 0, fb.tiles, sims, 0, nullptr,
                                 fb.list_tiles32));
        SelectArgs sa{};
        sa.sims = sims; sa.sims_base = 0; sa.k = s.k_ann; sa.out_sim = s.sim; sa.out_idx = s.idx;
        sa.jobs = flat_dev + fb.j0; sa.n_jobs = (int)(fb.j1 - fb.j0); sa.tile_begin = 0; sa.ids_are_rows = 1;
        set_filter(sa, s.nf);
        FAL_TRY(launch_select(ctx, ST_SELECT, MODE_DENSE, sa, fb.tiles * 32));
    }
    return FAL_OK;
}

// B. indexed buckets, the coarse quantiser: every query's n_probe lists, from the build's keys or from a scan of the centroids
static int run_coarse(const Search& s, const CoarsePlan& coarse, const TileCuts& cuts, const DenseJob* coarse_dev, float* sims,
                      int n_probe, Probes* out) {
    fal_ctx* ctx = s.ctx;
    const fal_ivf* ivf = s.ivf;
    const int d = ivf->d, n_jobs = (int)coarse.jobs.size();
    const int np = std::min(n_probe, coarse.max_n_list);
    int32_t* probes = nullptr;
    float* probe_sim = nullptr;
    int64_t *totals = nullptr, *q_sim_off = nullptr;
    FAL_TRY(ctx->reserve(SLOT_PROBES, sizeof(int32_t) * (size_t)ivf->n * np, (void**)&probes));
    FAL_TRY(ctx->reserve(SLOT_PROBE_SIM, sizeof(float) * (size_t)ivf->n * np, (void**)&probe_sim));
    const int64_t n_slots = coarse.tiles * 32;
    FAL_TRY(ctx->reserve(SLOT_QOFF, sizeof(int64_t) * (size_t)(n_slots + 1), (void**)&q_sim_off));
    FAL_TRY(ctx->reserve(SLOT_MISC, sizeof(int64_t) * (size_t)(n_slots + 2), (void**)&totals));
    FAL_CHECK_HIP(hipMemsetAsync(totals, 0, sizeof(int64_t) * (size_t)(n_slots + 2), ctx->stream));
    *out = Probes{np, probes, n_slots, totals, q_sim_off};
    // the final k-means pass left the (row, centroid) similarities behind as 16-bit keys: no second scan (coarse16.hip)
    const bool from_keys = ivf->ckeys != nullptr && ivf->X != nullptr &&
                           (ivf->ckeys_stride <= 512 || (ivf->ckeys_stride <= 2048 && ivf->sp_cols != nullptr));
    if (from_keys) {
        Coarse16Args ca{ivf->ckeys, ivf->ckeys_stride, ivf->X, ivf->centroids, d, coarse_dev, n_jobs, coarse.tiles, nullptr,
                        ivf->perm, np, probes};
        ca.sp_cols = ivf->sp_cols;
        ca.sp_vals = ivf->sp_vals;
        return launch_coarse16(ctx, ca);
    }
    FAL_TRY(ivf_ensure_xl(ctx, ivf));
    for (size_t bi = 0; bi + 1 < cuts.cuts.size(); ++bi) {
        const int64_t t0 = cuts.cuts[bi], t1 = cuts.cuts[bi + 1];
        const int64_t base = obase_of_tile(coarse.jobs, t0);
        FAL_TRY(launch_dense(ctx, ST_COARSE, EPI_STORE, ivf->Xl, ivf->centroids, d, coarse_dev, n_jobs, t0, t1 - t0, sims, base, nullptr));
        SelectArgs sa{};
        sa.sims = sims; sa.sims_base = base; sa.k = np; sa.out_sim = probe_sim; sa.out_idx = probes;
        sa.jobs = coarse_dev; sa.n_jobs = n_jobs; sa.tile_begin = t0; sa.ids_are_rows = 0;
        FAL_TRY(launch_select(ctx, ST_COARSE, MODE_DENSE, sa, (t1 - t0) * 32));
    }
    return FAL_OK;
}

// The candidate totals of every query, their prefix, and the inverted probe table (list -> the queries probing it); the
// per-tile prefix, the per-list tile prefix and the largest total come back to the host (the call's one wait in mid-stream)
static int build_probe_table(const Search& s, const CoarsePlan& coarse, const DenseJob* coarse_dev, const Probes& pr, ProbeTable* out) {
    fal_ctx* ctx = s.ctx;
    const fal_ivf* ivf = s.ivf;
    hipStream_t st = ctx->stream;
    const int np = pr.np, n_jobs = (int)coarse.jobs.size(), max_n_list = coarse.max_n_list;
    const int32_t* probes = pr.probes;
    int64_t *totals = pr.totals, *q_sim_off = pr.q_sim_off;
    const int64_t n_slots = pr.n_slots, ivf_tiles = coarse.tiles;
    const unsigned pg = (unsigned)ceil_div(n_slots, 256);
    // (buckets of up to 4,096 lists: the candidate totals come out of the probe histogram's pass below, one kernel for both)
    const bool fused_totals = max_n_list <= 4096;
    if (!fused_totals) {
        StageScope ts(ctx, ST_COARSE);
        with_np_vec(np, [&](auto v) {
            hipLaunchKernelGGL((probe_totals_kernel<decltype(v)::value>), dim3(pg), dim3(256), 0, st, probes, np, coarse_dev, n_jobs,
                               ivf_tiles, ivf->list_off, totals);
        });
        FAL_TRY(device_scan_i64(ctx, totals, n_slots, q_sim_off, SLOT_MISC2));      // (millions of slots: multi-block)
    }
    const int64_t TL = ivf->total_lists;
    const int64_t n_pairs_max = ivf->n * (int64_t)np;
    ScratchLayout LC, LI;
    const auto inv_off = LC.array<int64_t>(TL + 2), ltile_off = LC.array<int64_t>(TL + 2);
    const auto cnt = LC.array<int32_t>(TL + 1), cursor = LC.array<int32_t>(TL + 1), ltiles = LC.array<int32_t>(TL + 1);
    FAL_TRY(LC.reserve(ctx, SLOT_INVCNT));
    // (the probe table by sorted row as well when the f16 list scan may follow: ordered table + float16 rows attached)
    const bool want_rows = s.nf && ivf->X16pre && ivf->pos_of_row && max_n_list <= 16384;
    const auto inv_dest = LI.array<int64_t>(n_pairs_max);
    const auto inv_q = LI.array<int32_t>(n_pairs_max);
    LI.pad(want_rows ? 256 : 0);                            // inv_row begins 64 words behind inv_q
    const auto own_inv_row = LI.array<int32_t>(want_rows ? n_pairs_max : 0);
    LI.pad(want_rows ? 768 : 1024);                         // (slack, 1024 bytes in all: list16_kernel reads whole chunks of row ids)
    FAL_TRY(LI.reserve(ctx, SLOT_INV));
    int32_t* inv_row = want_rows ? own_inv_row.get() : nullptr;
    FAL_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(2 * TL + 2), st));     // cnt, cursor
    {
        StageScope ts(ctx, ST_COARSE);
        const dim3 bg((unsigned)n_jobs);                     // a workgroup per bucket
        if (fused_totals) {
            const size_t hl = 2 * sizeof(int32_t) * (size_t)max_n_list;
            with_np_vec(np, [&](auto v) {
                hipLaunchKernelGGL((probe_hist_totals_bucket_kernel<decltype(v)::value>), bg, dim3(1024), hl, st, probes, np, coarse_dev,
                                   ivf->list_off, ivf_tiles, cnt, totals);
            });
            FAL_TRY(device_scan_i64(ctx, totals, n_slots, q_sim_off, SLOT_MISC2));
        } else if (max_n_list <= 16384)
            hipLaunchKernelGGL(probe_hist_bucket_kernel, bg, dim3(1024), sizeof(int32_t) * (size_t)max_n_list, st, probes, np, coarse_dev,
                               cnt);
        else
            hipLaunchKernelGGL(probe_hist_kernel, dim3(pg), dim3(256), 0, st, probes, np, coarse_dev, n_jobs, ivf_tiles, cnt);
        FAL_TRY(device_scan_i32(ctx, cnt, TL, inv_off, SLOT_MISC2));
        const dim3 tg((unsigned)std::min<int64_t>(ceil_div(TL, 256), 1024));
        hipLaunchKernelGGL(list_tiles_kernel, tg, dim3(256), 0, st, cnt, ivf->list_off, TL, kGroupShift, ltiles);
        FAL_TRY(device_scan_i32(ctx, ltiles, TL, ltile_off, SLOT_MISC2));
        if (max_n_list <= 16384) {
            // (dynamic LDS stays at or below 64 KB: 12 bytes per list up to 4,096 lists, else 4)
            const int lds_lists = max_n_list <= probe_lds_lists() ? max_n_list : 0;
            const size_t lds = lds_lists ? (sizeof(int64_t) + sizeof(int32_t)) * (size_t)max_n_list : sizeof(int32_t) * (size_t)max_n_list;
            with_np_vec(np, [&](auto v) {
                hipLaunchKernelGGL((probe_scatter_bucket_kernel<decltype(v)::value>), bg, dim3(1024), lds, st, probes, np, coarse_dev,
                                   ivf->list_off, q_sim_off, inv_off, inv_q, inv_dest, ivf->perm, inv_row, lds_lists);
            });
        } else
            hipLaunchKernelGGL(probe_scatter_kernel, dim3(pg), dim3(256), 0, st, probes, np, coarse_dev, n_jobs, ivf_tiles, ivf->list_off,
                               q_sim_off, inv_off, cursor, inv_q, inv_dest);
    }
    FAL_CHECK_HIP(hipGetLastError());
    *out = ProbeTable{inv_off, ltile_off, inv_q, inv_dest, inv_row, q_sim_off, {}, {}, 0};
    // per-tile sims prefix and per-list tile prefix back to the host to cut bucket-sized batches
    out->qoff.resize((size_t)ivf_tiles + 1);
    out->lt_host.resize((size_t)TL + 1);
    FAL_CHECK_HIP(hipMemcpy2DAsync(out->qoff.data(), sizeof(int64_t), q_sim_off, 32 * sizeof(int64_t), sizeof(int64_t),
                                   (size_t)ivf_tiles + 1, hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipMemcpyAsync(out->lt_host.data(), ltile_off, sizeof(int64_t) * (size_t)(TL + 1), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipMemcpyAsync(&out->max_total, totals + n_slots + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipStreamSynchronize(st));
    return FAL_OK;
}

// the tiles [t0, t1) and lists [L0, L1) of a batch of whole indexed buckets (natural order)
struct BatchSpan { int64_t t0, t1, L0, L1; };
static BatchSpan span_of(const std::vector<DenseJob>& coarse, const BucketBatch& bt) {
    const DenseJob &first = coarse[bt.j0], &last = coarse[bt.j1 - 1];
    return {first.tile0, last.tile0 + ceil_div(last.nq, 32), first.c_row0, last.c_row0 + last.nc};
}

// C'. fine scan with the float16 prefilter (ivf16.hip): f16-MFMA scan to 16-bit keys, k-th key per query, exact tail
static int run_fine_keys(const Search& s, const CoarsePlan& coarse, const DenseJob* coarse_dev, const Probes& pr, const ProbeTable& pt,
                         const BucketCuts& cuts) {
    fal_ctx* ctx = s.ctx;
    const fal_ivf* ivf = s.ivf;
    const NeighborFilter* nf = s.nf;
    const int d = ivf->d, n_jobs = (int)coarse.jobs.size();
    // the IVF buckets in sorted-row order, 32-query tiles, sorted by decreasing size and dealt to the 8 XCD lists
    const SortedTiles32 t32 = plan_sorted_tiles32(coarse.jobs);
    ScratchLayout LJ;
    const auto jd = LJ.array<DenseJob>((int64_t)t32.j32.size());
    LJ.align(16);
    const auto tj32 = LJ.array<int32_t>(8 * t32.list_tiles32);
    FAL_TRY(LJ.reserve(ctx, SLOT_JOBS3));
    FAL_TRY(ctx->upload(jd, t32.j32.data(), sizeof(DenseJob) * t32.j32.size()));
    FAL_TRY(launch_tile_job32(ctx, jd, (int)t32.j32.size(), t32.list_tiles32, tj32));
    FusedArgs fa{};
    fa.X = ivf->X; fa.jobs32 = jd; fa.n_jobs32 = (int)t32.j32.size(); fa.tile_job32 = tj32;
    fa.k = s.k_ann;
    set_filter(fa, nf);
    fa.ivf = 1; fa.assign = ivf->assign; fa.pos_of_row = ivf->pos_of_row; fa.probes = pr.probes; fa.n_probe = pr.np;
    fa.mask_words = (coarse.max_n_list + 31) / 32; fa.list_off = ivf->list_off; fa.perm = ivf->perm;
    fa.sp_cols = ivf->sp_cols; fa.sp_vals = ivf->sp_vals; fa.rows_f16 = ivf->rows_f16;
    FAL_TRY(fused_prepare(ctx, &fa, ivf->n));
    // the exact part: only the (query, candidate) pairs that can matter (pairs16.hip)
    fa.ivf = 2;
    ScratchLayout LW;
    const auto gsel = LW.array<int2>(ivf->n);
    const auto pmz_l = LW.array<float>(ivf->n);
    FAL_TRY(LW.reserve(ctx, SLOT_WIN));
    FAL_TRY(launch_gather_pmz(ctx, nf->pmz, ivf->perm, ivf->n, pmz_l));
    uint16_t* keys = nullptr;
    // (list16_kernel addresses a batch's keys by 32-bit byte offsets from the buffer's base)
    FAL_REQUIRE(cuts.need + 2 * kSimsSlack < ((size_t)1 << 31), FAL_EUNSUPPORTED, "key batch too large (lower FALCON_SIMS_MB)");
    ctx->release(SLOT_SIMS);        // the flat / coarse stage's sims are dead (its launches are enqueued)
    FAL_TRY(ctx->reserve(SLOT_SIMS, sizeof(uint16_t) * (cuts.need + 2 * kSimsSlack), (void**)&keys));
    int64_t max_cand = 0;
    for (int64_t t = 0; t < coarse.tiles; ++t) max_cand = std::max(max_cand, pt.qoff[(size_t)t + 1] - pt.qoff[(size_t)t]);
    for (const BucketBatch& bt : cuts.batches) {
        const BatchSpan b = span_of(coarse.jobs, bt);
        const int64_t base = pt.qoff[(size_t)b.t0];
        List16Args la{};
        la.X16 = reinterpret_cast<const __half*>(ivf->X16pre); la.perm = ivf->perm;
        la.sq16 = ivf->rows_many ? nullptr : ivf->sq16;      // (queries as 256-byte sparse records: list16s.hip)
        la.d = d; la.list_off = ivf->list_off; la.inv_off = pt.inv_off;
        la.ltile_off = pt.ltile_off; la.inv_row = pt.inv_row; la.inv_dest = pt.inv_dest; la.list_begin = b.L0; la.list_end = b.L1;
        la.tile_begin = pt.lt_host[(size_t)b.L0]; la.n_tiles_max = pt.lt_host[(size_t)b.L1] - pt.lt_host[(size_t)b.L0];
        la.keys = keys; la.keys_base = base; la.sink = keys + cuts.need; la.n_rows = ivf->n;
        FAL_TRY(launch_list16(ctx, la));
        Kept16Args ka{};
        ka.keys = keys; ka.keys_base = base; ka.jobs = coarse_dev; ka.tile_begin = b.t0; ka.n_probe = pr.np;
        ka.probes = pr.probes; ka.list_off = ivf->list_off; ka.q_sim_off = pt.q_sim_off; ka.perm = ivf->perm; ka.pmz_l = pmz_l;
        ka.rt = nf->rt; ka.tol = nf->tol; ka.rt_tol = nf->rt_tol; ka.tol_f = fa.tol_f; ka.rt_f = fa.rt_f; ka.is_da = nf->is_da;
        ka.gsel = gsel; ka.gkept_id = fa.gkept_id; ka.gkcnt = fa.gkcnt;
        ka.n_tiles = b.t1 - b.t0;
        Select16Args sa{};
        sa.keys = keys; sa.keys_base = base; sa.k = s.k_ann; sa.jobs = coarse_dev; sa.n_jobs = n_jobs;
        sa.tile_begin = b.t0; sa.q_sim_off = pt.q_sim_off;
        sa.perm = ivf->perm; sa.thr = fa.thr; sa.gmem_v = fa.gmem_v; sa.gmem_id = fa.gmem_id;
        sa.max_keys = pt.max_total;
        sa.gsel = gsel;
        // FALCON_KEPT16=fused (A/B switch, read per launch; single-pass searches -- no query above 2,048 keys): kept16 as the
        // tail of the selection kernel, four queries per wave (select16k_kernel)
        const char* ke = getenv("FALCON_KEPT16");
        const bool fuse_kept = pt.max_total + 7 <= 2048 && ke && !strcmp(ke, "fused");
        sa.fuse_kept = fuse_kept ? 1 : 0;
        sa.kept = ka;
        FAL_TRY(launch_select16(ctx, sa, b.t1 - b.t0));
        if (!fuse_kept) FAL_TRY(launch_kept16(ctx, ka, b.t1 - b.t0));
    }
    FAL_TRY(launch_pairs16(ctx, fa, d, t32.list_tiles32));
    FAL_TRY(launch_fused_ivf_tail(ctx, fa, d, t32.list_tiles32, max_cand));
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return FAL_OK;
}

// C. the exact staged fine scan: fp32 list scan into the hand-off buffer, then the select
static int run_fine_staged(const Search& s, const CoarsePlan& coarse, const DenseJob* coarse_dev, const Probes& pr, const ProbeTable& pt,
                           const BucketCuts& cuts) {
    fal_ctx* ctx = s.ctx;
    const fal_ivf* ivf = s.ivf;
    float* sims = nullptr;
    ctx->release(SLOT_SIMS);        // the flat / coarse stage's sims are dead (its launches are enqueued)
    FAL_TRY(ctx->reserve(SLOT_SIMS, sizeof(float) * (cuts.need + kSimsSlack), (void**)&sims));
    FAL_TRY(ivf_ensure_xl(ctx, ivf));
    for (const BucketBatch& bt : cuts.batches) {
        const BatchSpan b = span_of(coarse.jobs, bt);
        const int64_t base = pt.qoff[(size_t)b.t0];
        ListScanArgs la{};
        la.Xl = ivf->Xl; la.d = ivf->d; la.list_off = ivf->list_off; la.inv_off = pt.inv_off; la.ltile_off = pt.ltile_off;
        la.inv_q = pt.inv_q; la.inv_dest = pt.inv_dest; la.list_begin = b.L0; la.list_end = b.L1; la.group_shift = kGroupShift;
        la.tile_begin = pt.lt_host[(size_t)b.L0]; la.n_tiles_max = pt.lt_host[(size_t)b.L1] - pt.lt_host[(size_t)b.L0];
        la.sims = sims; la.sims_base = base; la.sink = sims + cuts.need;
        FAL_TRY(launch_list_scan(ctx, la));
        SelectArgs sa{};
        sa.sims = sims; sa.sims_base = base; sa.k = s.k_ann; sa.out_sim = s.sim; sa.out_idx = s.idx;
        sa.jobs = coarse_dev; sa.n_jobs = (int)coarse.jobs.size(); sa.tile_begin = b.t0;
        sa.n_probe = pr.np; sa.probes = pr.probes; sa.list_off = ivf->list_off; sa.q_sim_off = pt.q_sim_off; sa.perm = ivf->perm;
        set_filter(sa, s.nf);
        FAL_TRY(launch_select(ctx, ST_SELECT, MODE_IVF, sa, (b.t1 - b.t0) * 32));
    }
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return FAL_OK;
}

static int search_impl(fal_ctx* ctx, const fal_ivf* ivf, int n_probe, int k_ann, float* sim, int32_t* idx,
                       const NeighborFilter* nf) {
    FAL_REQUIRE(ctx && ivf, FAL_EINVAL, "fal_ivf_search_topk: NULL ctx/ivf");
    FAL_REQUIRE(k_ann >= 1 && k_ann <= FAL_MAX_K_ANN, FAL_EUNSUPPORTED, "fal_ivf_search_topk: k_ann must be in [1, %d]", FAL_MAX_K_ANN);
    FAL_REQUIRE(n_probe >= 1 && n_probe <= FAL_MAX_N_PROBE, FAL_EUNSUPPORTED, "fal_ivf_search_topk: n_probe must be in [1, %d]", FAL_MAX_N_PROBE);
    if (ivf->n == 0) return FAL_OK;
    FAL_REQUIRE(nf || (sim && idx), FAL_EINVAL, "fal_ivf_search_topk: NULL output");
    hipStream_t st = ctx->stream;
    const int d = ivf->d;
    const int64_t n_buckets = (int64_t)ivf->n_list.size();
    const int64_t* bucket_off = ivf->bucket_off.data();
    ctx->stage_reset(ST_COARSE);
    ctx->stage_reset(ST_SCAN);
    ctx->stage_reset(ST_KERNEL);
    ctx->stage_reset(ST_SELECT);
    // fallback queries of this call (fal_ctx_counter 5): reset in stream order -- a previous call's asynchronous copy into
    // the same pinned words may still be in flight
    FAL_CHECK_HIP(hipMemcpyAsync(ctx->fb_host, ctx->zero_dev, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipMemcpyAsync(ctx->fb_host + 2, ctx->zero_dev, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    const Search s{ctx, ivf, k_ann, sim, idx, nf, sims_capacity_floats()};

    // ---- the plan (searchplan.h): job tables and batch cuts ------------------------------------------------------------
    std::vector<int64_t> order = flat_order(bucket_off, ivf->n_list.data(), n_buckets);
    // Flat buckets with the top-k kept on chip (fused.hip): needs the float16 prefilter rows and the fused a8 output
    const bool fused = nf && ivf->Xpre && ivf->X && fused_supports(d) && !order.empty() &&
                       (bucket_off[order[0] + 1] - bucket_off[order[0]]) < 65536;
    if (fused) {
        FAL_TRY(run_fused_flat(s, order));
        order.clear();                        // nothing left for the staged flat path
    }
    const bool have16 = ivf->X16 != nullptr;
    const bool have4 = ivf->X && dense4_supports(d);       // the shared-stream fp32 kernels (scan.hip)
    const FlatRule rule = FlatRule::make(have16, have4, ivf->X != nullptr, d, dense1_max_env());
    FAL_REQUIRE(have16 || ivf->X || order.empty(), FAL_EINVAL, "fal_ivf_search_topk: the index has no vectors to scan");
    const FlatPlan flat = plan_flat(order, bucket_off, rule, s.cap);
    const CoarsePlan coarse = plan_coarse(bucket_off, ivf->n_list.data(), ivf->list_base.data(), n_buckets);
    const TileCuts coarse_cuts = cut_tile_batches(coarse.jobs, coarse.tiles, s.cap);

    DenseJob *flat_dev = nullptr, *coarse_dev = nullptr;
    if (!flat.jobs.empty()) {
        FAL_TRY(ctx->reserve(SLOT_JOBS, sizeof(DenseJob) * flat.jobs.size(), (void**)&flat_dev));
        FAL_TRY(ctx->upload(flat_dev, flat.jobs.data(), sizeof(DenseJob) * flat.jobs.size()));
    }
    if (!coarse.jobs.empty()) {
        FAL_TRY(ctx->reserve(SLOT_JOBS2, sizeof(DenseJob) * coarse.jobs.size(), (void**)&coarse_dev));
        FAL_TRY(ctx->upload(coarse_dev, coarse.jobs.data(), sizeof(DenseJob) * coarse.jobs.size()));
    }
    float* sims = nullptr;
    const size_t sims_floats = std::max(flat.need, coarse_cuts.need);
    FAL_TRY(ctx->reserve(SLOT_SIMS, sizeof(float) * (sims_floats + kSimsSlack), (void**)&sims));   // slack: scan16 sink, select over-reads
    FAL_TRY(run_flat_batches(s, flat, rule, flat_dev, sims, sims_floats));
    const FlatCounters fc = flat_counters(flat, have4);    // (after a fused flat scan nothing is left: zeros)
    if (!fused) {
        ctx->counters[0] = fc.pairs;
        ctx->counters[4] = fc.mfma;
        ctx->counters[2] = (int64_t)flat.batches.size();
        ctx->counters[3] = (int64_t)(sizeof(float) * sims_floats);
    }
    ctx->counters[7] = fc.tiny_pairs;
    ctx->counters[8] = fc.tiny_mfma;
    ctx->counters[1] = 0;
    if (coarse.jobs.empty()) return FAL_OK;   // (job tables went through the pinned upload ring: nothing to wait for)
    for (const DenseJob& j : coarse.jobs) ctx->counters[1] += (int64_t)j.nq * j.nc;

    Probes pr;
    FAL_TRY(run_coarse(s, coarse, coarse_cuts, coarse_dev, sims, n_probe, &pr));
    ProbeTable pt;
    FAL_TRY(build_probe_table(s, coarse, coarse_dev, pr, &pt));
    // The float16 path's batches hold 2-byte keys: the same BYTES as a batch of float32 sims = twice the candidates (fewer, larger
    // launches of the three per-batch kernels: -1.3 ms per 10 M pass; smaller batches -- down to the 256 MB of the memory-side
    // cache -- only lose, NOTES r6).  select16_kernel holds at most 4,096 keys of a query in registers; coarser indexes keep the
    // exact staged scan rather than sending every query through the exact fallback
    const bool key_path = pt.inv_row && ivf->X && ivf16_supports(d) && pt.max_total <= 4096;
    const int64_t cap_fine = key_path ? (int64_t)std::min<size_t>(2 * s.cap, ((size_t)1 << 31) - 4 * kSimsSlack) : (int64_t)s.cap;
    const BucketCuts fine = cut_bucket_batches(coarse.jobs, pt.qoff, cap_fine);
    ctx->counters[0] += pt.qoff[(size_t)coarse.tiles];
    ctx->counters[2] += (int64_t)fine.batches.size();
    ctx->counters[3] = std::max<int64_t>(ctx->counters[3], (int64_t)(sizeof(float) * fine.need));
    FAL_REQUIRE(fine.need + kSimsSlack < ((size_t)1 << 32), FAL_EUNSUPPORTED, "sims batch too large (lower FALCON_SIMS_MB)");
    return key_path ? run_fine_keys(s, coarse, coarse_dev, pr, pt, fine) : run_fine_staged(s, coarse, coarse_dev, pr, pt, fine);
}

extern "C" int fal_ivf_search_topk(fal_ctx* ctx, const fal_ivf* ivf, int n_probe, int k_ann, float* sim, int32_t* idx) {
    fal::CallScope _call(ctx);
    return search_impl(ctx, ivf, n_probe, k_ann, sim, idx, nullptr);
}

extern "C" int fal_ivf_search_neighbors(fal_ctx* ctx, const fal_ivf* ivf, int n_probe, int k_ann,
                                        const float* precursor_mz_sorted, const float* rt_sorted, double tol, int tol_is_da,
                                        double rt_tol, int n_neighbors, int32_t* nb_idx, float* nb_dist,
                                        int32_t* nb_count) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && ivf, FAL_EINVAL, "fal_ivf_search_neighbors: NULL ctx/ivf");
    FAL_REQUIRE(n_neighbors >= 1 && n_neighbors <= FAL_MAX_K_ANN, FAL_EUNSUPPORTED,
                "fal_ivf_search_neighbors: n_neighbors must be in [1, %d]", FAL_MAX_K_ANN);
    if (ivf->n == 0) return FAL_OK;
    FAL_REQUIRE(precursor_mz_sorted && nb_idx && nb_dist, FAL_EINVAL, "fal_ivf_search_neighbors: NULL array");
    NeighborFilter nf{precursor_mz_sorted, rt_tol >= 0.0 ? rt_sorted : nullptr, tol, rt_tol, tol_is_da, n_neighbors, nb_idx, nb_dist,
                      nb_count};
    ctx->stage_reset(ST_FILTER);
    return search_impl(ctx, ivf, n_probe, k_ann, nullptr, nullptr, &nf);
}
