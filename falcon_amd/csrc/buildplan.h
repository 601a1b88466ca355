// The host arithmetic of an index build (ivf.hip): the list table of a bucket table, which assignment kernel a bucket's k-means
// passes take and the job tables of those kernels, and the small rules of the list sort, the sparsify launch, the coarse keys and
// the host-made tables.  Plain host C++, no HIP -- tests/test_buildplan_cpu.py compiles it on its own.  The CU count, the float16
// switch, the list limit and the key budget are arguments everywhere.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "searchplan.h"

namespace fal {

struct BucketDev {       // one per IVF (n_list > 1) bucket
    int64_t row0;        // first sorted row
    int64_t list0;       // global id of its list 0
    int32_t n;           // rows
    int32_t n_list;
    int64_t wave0;       // index of its first (bucket, list) wave in per-list launches
};

// Shared-stream list assignment (assign.hip): job = (a segment of a bucket's rows) x (up to 128 of its centroids)
constexpr int kAssignSeg = 2048;      // rows per segment
constexpr int kAssignGroup = 128;     // centroids per job: one 32-centroid tile per wave
constexpr int kAssignMaxLists = 512;  // lists per bucket up to which the exact assignment runs in the shared-stream kernel
constexpr int kAssignMergeLists = 2048;     // lists per bucket up to which the float16 assignment runs in groups of 128 + a merge
                                            // (16 groups = 64 subgroups of 32; round 4 stopped at 512 and sent a 1,024-list
                                            // bucket -- `--batch_size 65536` on 45 k-row windows -- to the exact fp32 kernels:
                                            // build 584 ms instead of 77 per 10 M spectra, profiles/NOTES.md r5)
constexpr int kBucketSortMaxLists = 2048;   // lists per bucket the one-wave list sort counts in LDS (bucket_list_sort_kernel)
struct AssignJob {
    int64_t row0;        // first row of the segment (sorted rows = rows of X)
    int64_t cent0;       // global row of the group's first centroid
    int32_t nrows;       // rows in the segment (<= kAssignSeg)
    int32_t ncent;       // centroids in the group (1..kAssignGroup)
    int32_t id_base;     // bucket-local list id of the group's first centroid
    int32_t part0;       // merge / group jobs (assign16.hip): position of the segment's first row among the rows of ALL merge
                         // buckets = the row index of the partial arrays (0 elsewhere)
};

// ---- the list table ------------------------------------------------------------------------------------------------------
inline bool all_flat(const int32_t* n_list, int64_t n_buckets) {      // (rows may be NULL only then)
    bool any_ivf = false;
    for (int64_t b = 0; b < n_buckets; ++b) any_ivf |= n_list[b] > 1;
    return !any_ivf;
}

struct ListTable {
    std::vector<int64_t> list_base;    // [n_buckets + 1] global id of every bucket's list 0, then total_lists
    std::vector<BucketDev> bk;         // the indexed buckets in bucket order
    int64_t total_lists = 0, ivf_waves = 0;
};
// -> -1, or the first bucket that is invalid: negative size, n_list outside [1, max_n_list] or above the rows of a non-empty
// bucket, more than INT32_MAX rows
inline int64_t plan_lists(const int64_t* bucket_off, const int32_t* n_list, int64_t n_buckets, int max_n_list, ListTable& t) {
    t.list_base.resize((size_t)n_buckets + 1);
    int64_t total = 0, waves = 0;
    for (int64_t b = 0; b < n_buckets; ++b) {
        const int64_t nb = bucket_off[b + 1] - bucket_off[b];
        if (nb < 0 || n_list[b] < 1 || n_list[b] > max_n_list || (nb > 0 && n_list[b] > nb) || nb > INT32_MAX) return b;
        t.list_base[(size_t)b] = total;
        if (n_list[b] > 1) {
            t.bk.push_back({bucket_off[b], total, (int32_t)nb, n_list[b], waves});
            waves += n_list[b];
        }
        total += n_list[b];
    }
    t.list_base[(size_t)n_buckets] = total;
    t.total_lists = total;
    t.ivf_waves = waves;
    return -1;
}

// ---- the assignment passes -----------------------------------------------------------------------------------------------
// Every k-means pass assigns a bucket's rows with one of five kernels, by its list count and by whether float16 rows are at hand:
//   use16, <= kAssignGroup lists       single-group jobs of assign16.hip (one job per row segment)
//   use16, <= kAssignMergeLists        merge jobs + their group jobs (groups of 128 centroids, then a merge over the groups)
//   <= 64 lists                        one-wave jobs of assign.hip (a 4-wave workgroup would idle most of its waves)
//   <= kAssignMaxLists                 4-wave jobs of assign.hip: (row segment) x (group of <= 128 centroids)
//   more                               the row-resident kernel (dense.hip), whose 32-row tile is amortised over many chunks
struct AssignPlan {
    std::vector<AssignJob> wide;       // launch_assign's table: n_wide 4-wave jobs, then n_wave one-wave jobs
    std::vector<AssignJob> half;       // launch_assign16's table: n_single, then n_merge, then n_group jobs
    std::vector<DenseJob> dense;
    int64_t n_wide = 0, n_wave = 0, n_single = 0, n_merge = 0, n_group = 0;
    int64_t dtiles = 0;                // 32-row tiles of the dense jobs
    int64_t merge_rows = 0;            // rows of the merge buckets: the partial arrays' rows (AssignJob::part0)
    int merge_max_lists = 0;
    int max_n_list = 0;                // of all indexed buckets
    int64_t seg = 0, wseg = 0;         // rows per 4-wave / one-wave job
};
// rows per job: long segments amortise the resident centroid tiles, but with only a few indexed buckets long segments leave most
// CUs idle -- aim for >= `per_cu` workgroups per CU, between 256 and kAssignSeg rows (a multiple of 32)
inline int64_t assign_seg_rows(int64_t work_rows, int num_cus, int per_cu) {
    return std::min<int64_t>(kAssignSeg, std::max<int64_t>(256, tiles_of(work_rows, (int64_t)num_cus * per_cu * 32) * 32));
}
inline AssignPlan plan_assign(const BucketDev* bk, size_t n_bk, int num_cus, bool use16) {
    AssignPlan p;
    int64_t work_rows = 0, wave_rows = 0;          // (rows x centroid groups, whichever kernel the bucket takes in the end)
    for (size_t i = 0; i < n_bk; ++i) {
        const BucketDev& b = bk[i];
        if (b.n_list <= 64) wave_rows += (int64_t)b.n * tiles_of(b.n_list, 32);
        else if (b.n_list <= kAssignMaxLists) work_rows += (int64_t)b.n * tiles_of(b.n_list, kAssignGroup);
        p.max_n_list = std::max(p.max_n_list, (int)b.n_list);
    }
    p.seg = assign_seg_rows(work_rows, num_cus, 4);
    p.wseg = assign_seg_rows(wave_rows, num_cus, 16);
    std::vector<AssignJob> wave, merge, group;
    for (size_t i = 0; i < n_bk; ++i) {
        const BucketDev& b = bk[i];
        if (use16 && b.n_list <= kAssignGroup) {
            for (int64_t s0 = 0; s0 < b.n; s0 += kAssignSeg)
                p.half.push_back({b.row0 + s0, b.list0, (int32_t)std::min<int64_t>(kAssignSeg, b.n - s0), b.n_list, 0, 0});
        } else if (use16 && b.n_list <= kAssignMergeLists) {
            p.merge_max_lists = std::max(p.merge_max_lists, (int)b.n_list);
            for (int64_t s0 = 0; s0 < b.n; s0 += kAssignSeg) {
                const int32_t nr = (int32_t)std::min<int64_t>(kAssignSeg, b.n - s0);
                merge.push_back({b.row0 + s0, b.list0, nr, b.n_list, 0, (int32_t)p.merge_rows});
                for (int t0 = 0; t0 < b.n_list; t0 += kAssignGroup)      // the groups of a segment next to each other: they
                    group.push_back({b.row0 + s0, b.list0 + t0, nr, std::min(kAssignGroup, b.n_list - t0), t0,   // share its rows in L2
                                     (int32_t)p.merge_rows});
                p.merge_rows += nr;
            }
        } else if (b.n_list <= 64) {
            for (int64_t s0 = 0; s0 < b.n; s0 += p.wseg)
                for (int t0 = 0; t0 < b.n_list; t0 += 32)
                    wave.push_back({b.row0 + s0, b.list0 + t0, (int32_t)std::min<int64_t>(p.wseg, b.n - s0), std::min(32, b.n_list - t0),
                                    t0, 0});
        } else if (b.n_list <= kAssignMaxLists) {
            for (int64_t s0 = 0; s0 < b.n; s0 += p.seg)
                for (int t0 = 0; t0 < b.n_list; t0 += kAssignGroup)
                    p.wide.push_back({b.row0 + s0, b.list0 + t0, (int32_t)std::min<int64_t>(p.seg, b.n - s0),
                                      std::min(kAssignGroup, b.n_list - t0), t0, 0});
        } else {
            p.dense.push_back({b.row0, b.list0, 0, p.dtiles, b.n, b.n_list, 0});
            p.dtiles += tiles_of(b.n, 32);
        }
    }
    p.n_wide = (int64_t)p.wide.size();
    p.n_wave = (int64_t)wave.size();
    p.wide.insert(p.wide.end(), wave.begin(), wave.end());
    p.n_single = (int64_t)p.half.size();
    p.n_merge = (int64_t)merge.size();
    p.n_group = (int64_t)group.size();
    p.half.insert(p.half.end(), merge.begin(), merge.end());
    p.half.insert(p.half.end(), group.begin(), group.end());
    return p;
}

// ---- the small rules -----------------------------------------------------------------------------------------------------
// key bits of the stable sort of the rows by global list
inline int list_sort_end_bit(int64_t total_lists) {
    int end_bit = 1;
    while (end_bit < 32 && (1ll << end_bit) < total_lists) ++end_bit;
    return end_bit;
}
// after the first (global) sort every later one only re-orders the rows inside the indexed buckets: one wave per bucket, as long
// as the bucket with the most lists fits the kernel's LDS histogram
inline bool bucket_sort_serves(int max_n_list) { return max_n_list <= kBucketSortMaxLists; }
// sparsify_rows_kernel: blocks of 256 rows, seg_off[i] = first block of indexed bucket i, seg_off[n_bk] = blocks of the launch
inline std::vector<int64_t> sparsify_segments(const BucketDev* bk, size_t n_bk) {
    std::vector<int64_t> seg_off(n_bk + 1, 0);
    for (size_t i = 0; i < n_bk; ++i) seg_off[i + 1] = seg_off[i] + tiles_of(bk[i].n, 256);
    return seg_off;
}
// columns of the coarse keys: the groups of the bucket with the most lists; n x stride 16-bit keys against a budget in bytes
inline int ckeys_stride_of(int max_n_list) { return kAssignGroup * (int)tiles_of(max_n_list, kAssignGroup); }
inline size_t ckeys_bytes(int64_t n, int stride) { return sizeof(uint16_t) * (size_t)n * stride; }
inline size_t ckeys_budget_bytes(size_t mb) { return mb << 20; }      // FALCON_CKEYS_MB as given
inline bool ckeys_fit(int64_t n, int stride, size_t budget_bytes) { return ckeys_bytes(n, stride) <= budget_bytes; }
// counts[total_lists + 1]: flat buckets hold all their rows in their single list (the lists of indexed buckets: 0)
inline std::vector<int64_t> initial_counts(const int64_t* bucket_off, const int32_t* n_list, const int64_t* list_base, int64_t n_buckets) {
    std::vector<int64_t> cnt((size_t)list_base[n_buckets] + 1, 0);
    for (int64_t b = 0; b < n_buckets; ++b)
        if (n_list[b] == 1) cnt[(size_t)list_base[b]] = bucket_off[b + 1] - bucket_off[b];
    return cnt;
}
// every bucket is flat: the list offsets ARE the bucket offsets (list_off[total_lists + 1])
inline std::vector<int64_t> flat_list_off(const int64_t* bucket_off, const int64_t* list_base, int64_t n_buckets) {
    const int64_t total = list_base[n_buckets];
    std::vector<int64_t> off((size_t)total + 1, 0);
    for (int64_t b = 0; b < n_buckets; ++b) off[(size_t)list_base[b] + 1] = bucket_off[b + 1];
    for (int64_t g = 1; g <= total; ++g) off[(size_t)g] = std::max(off[(size_t)g], off[(size_t)g - 1]);
    return off;
}

}  // namespace fal
