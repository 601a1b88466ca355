// The host arithmetic of a search (search.hip): which flat bucket goes to which kernel, how jobs are dealt to the 8 XCD lists,
// where the hand-off buffer's cap cuts the flat, coarse and fine batches, and what the roofline counters report.  Plain host
// C++, no HIP -- tests/test_searchplan_cpu.py compiles it on its own.  The cap is an argument everywhere.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace fal {

// One unit of dense work: the queries [q_row0, q_row0+nq) of array Q against the candidates
// [c_row0, c_row0+nc) of array C.  Tiles of 32 queries; tile0 = index of the job's first tile
// in the launch; obase = where the job's sims start (float index): one [32, ceil32(nc)] block per tile.
struct DenseJob {
    int64_t q_row0;
    int64_t c_row0;
    int64_t obase;
    int64_t tile0;
    int32_t nq;
    int32_t nc;
    int64_t xtile0;   // XCD-list mode: tiles of earlier jobs of the same XCD list (jobs j, j+8, j+16 ...)
};

inline int64_t tiles_of(int64_t rows, int64_t per_tile) { return (rows + per_tile - 1) / per_tile; }
// floats one 32-query tile of a job with nc candidates hands to the select: a [32, ceil32(nc)] block
inline int64_t tile_block_floats(int64_t nc) { return 32 * ((nc + 31) & ~31ll); }
inline int64_t sims_block_floats(int64_t nq, int64_t nc) { return tiles_of(nq, 32) * tile_block_floats(nc); }

// FALCON_SIMS_MB -> floats of the hand-off buffer a batch may fill (the search's floor: 16 MB)
inline size_t sims_cap_floats(size_t mb) { return std::max<size_t>(mb, 16) * 1024 * 1024 / sizeof(float); }

// XCD-list mode (simtile.h): job j of a launch belongs to list j % 8; a job's xtile0 = the tiles of the earlier jobs of its list
struct XcdDeal {
    int64_t list[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t take(size_t j, int64_t tiles) {
        const int64_t at = list[j & 7];
        list[j & 7] += tiles;
        return at;
    }
    int64_t longest() const { return *std::max_element(list, list + 8); }
};

// The non-empty flat buckets (one list) by decreasing size, ties in bucket order: the longest tiles start first, every XCD gets
// the same mix.  A counting sort, O(buckets + max size): this runs on the critical path.
inline std::vector<int64_t> flat_order(const int64_t* bucket_off, const int32_t* n_list, int64_t n_buckets) {
    auto flat_rows = [&](int64_t b) { return n_list[b] == 1 ? bucket_off[b + 1] - bucket_off[b] : 0; };
    int64_t max_sz = 0;
    for (int64_t b = 0; b < n_buckets; ++b) max_sz = std::max(max_sz, flat_rows(b));
    std::vector<int64_t> start((size_t)max_sz + 2, 0);
    for (int64_t b = 0; b < n_buckets; ++b)
        if (flat_rows(b) > 0) ++start[(size_t)(max_sz - flat_rows(b)) + 1];
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
    std::vector<int64_t> order((size_t)start.back());
    for (int64_t b = 0; b < n_buckets; ++b)
        if (flat_rows(b) > 0) order[(size_t)start[(size_t)(max_sz - flat_rows(b))]++] = b;
    return order;
}

// ---- flat buckets through the hand-off buffer ---------------------------------------------------------------------------
enum FlatKernel {
    FLAT_F16,          // f16-MFMA scan, 128-query tiles (scan16.hip)
    FLAT_DENSE4,       // shared-stream fp32 kernel, groups of four 32-query tiles
    FLAT_ONE_WAVE,     // one-wave fp32 kernel: a wave per 32-query tile, no staircase to wait in (33 .. small_max rows)
    FLAT_TINY4,        // the rest, "one-block" buckets: dense_tiny4_kernel ...
    FLAT_EXACT_SMALL,  // ... exact chains on the vector ALU beyond low_dim 512 ...
    FLAT_DENSE         // ... dense_kernel where the shared-stream kernels have no form for d
};
struct FlatRule {
    bool have16;       // f16 rows for the flat scan are attached
    bool have4;        // float32 rows and a shared-stream fp32 form for d (dense4_supports)
    bool has_f32;      // float32 rows; without them every bucket takes the f16 kernel
    int d;
    int64_t small_max; // largest bucket of the one-wave kernel (>= 32; 32: none)
    // small_max from FALCON_DENSE1_MAX (0: unset): no one-wave fp32 kernel beyond 512 columns
    static FlatRule make(bool have16, bool have4, bool has_f32, int d, int dense1_max_env) {
        return {have16, have4, has_f32, d, (have4 && d <= 512) ? std::max(32, dense1_max_env) : 32};
    }
};
inline FlatKernel flat_one_block_kernel(const FlatRule& r) { return r.d > 512 ? FLAT_EXACT_SMALL : r.have4 ? FLAT_TINY4 : FLAT_DENSE; }
inline FlatKernel flat_kernel_of(const FlatRule& r, int64_t nb) {
    if (r.have16 && nb >= (r.has_f32 ? 64 : 0)) return FLAT_F16;       // buckets below 64 rows: the fp32 kernels
    if (r.have4 && nb > r.small_max) return FLAT_DENSE4;
    if (r.have4 && nb > 32) return FLAT_ONE_WAVE;
    return flat_one_block_kernel(r);
}

// a batch = jobs [j0, j1): [j0, jm) f16 scan, [jm, js) dense4, [js, jk) one-wave, [jk, j1) one-block (sizes are non-increasing,
// so each class is a run); list_tiles* = the longest XCD list of the f16 / one-block / one-wave jobs
struct FlatBatch {
    size_t j0, jm, js, jk, j1;
    int64_t tiles, list_tiles16, list_tiles32, list_tiles1, floats;
};
struct FlatPlan {
    std::vector<DenseJob> jobs;        // obase / tile0 / xtile0 relative to the job's batch
    std::vector<FlatBatch> batches;
    size_t need = 0;                   // floats of the largest batch
};
// order = flat_order(); a batch is closed by the first bucket that would take it over the cap (a bucket larger than the cap is a
// batch of its own)
inline FlatPlan plan_flat(const std::vector<int64_t>& order, const int64_t* bucket_off, const FlatRule& rule, size_t cap) {
    FlatPlan p;
    p.jobs.reserve(order.size());
    FlatBatch cur{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    XcdDeal x16, x32, x1;
    auto close = [&]() {
        if (cur.j1 > cur.j0) {
            cur.list_tiles16 = x16.longest();
            cur.list_tiles32 = x32.longest();
            cur.list_tiles1 = x1.longest();
            p.batches.push_back(cur);
            p.need = std::max(p.need, (size_t)cur.floats);
        }
        cur = FlatBatch{cur.j1, cur.j1, cur.j1, cur.j1, cur.j1, 0, 0, 0, 0, 0};
        x16 = x32 = x1 = XcdDeal{};
    };
    for (int64_t b : order) {
        const int64_t row0 = bucket_off[b], nb = bucket_off[b + 1] - row0;
        const int64_t tiles = tiles_of(nb, 32), floats = sims_block_floats(nb, nb);
        if (cur.floats + floats > (int64_t)cap && cur.j1 > cur.j0) close();
        const size_t j = cur.j1;
        int64_t xtile0 = 0;                                  // (launch_dense4 lists the groups of its jobs itself)
        switch (flat_kernel_of(rule, nb)) {
        case FLAT_F16: xtile0 = x16.take(j - cur.j0, tiles_of(nb, 128)); cur.jm = cur.js = cur.jk = j + 1; break;
        case FLAT_DENSE4: cur.js = cur.jk = j + 1; break;
        case FLAT_ONE_WAVE: xtile0 = x1.take(j - cur.js, tiles); cur.jk = j + 1; break;
        default: xtile0 = x32.take(j - cur.jk, tiles);
        }
        p.jobs.push_back({row0, row0, cur.floats, cur.tiles, (int32_t)nb, (int32_t)nb, xtile0});
        cur.tiles += tiles;
        cur.floats += floats;
        cur.j1++;
    }
    close();
    return p;
}

// fal_ctx_counter 0 / 4 / 7 / 8 of the flat part
struct FlatCounters {
    int64_t pairs = 0;        // 0: (query, candidate) pairs
    int64_t mfma = 0;         // 4: inner products the matrix cores computed, padding included: blocks on / above the diagonal
                              //    (the f16 kernel: + up to 3 per 128-row tile)
    int64_t tiny_pairs = 0;   // 7, 8: the same two of the one-block buckets (dense_tiny4_kernel: outside stage 8)
    int64_t tiny_mfma = 0;
};
inline FlatCounters flat_counters(const FlatPlan& p, bool have4) {
    FlatCounters c;
    for (const DenseJob& j : p.jobs) {
        const int64_t ch = tiles_of(j.nc, 32);
        c.pairs += (int64_t)j.nq * j.nc;
        c.mfma += 1024 * (ch * (ch + 1) / 2);
    }
    if (have4)
        for (const FlatBatch& fb : p.batches)
            for (size_t j = fb.jk; j < fb.j1; ++j) {
                c.tiny_pairs += (int64_t)p.jobs[j].nq * p.jobs[j].nc;
                c.tiny_mfma += 1024;
            }
    return c;
}

// ---- flat buckets with the top-k kept on chip (fused.hip) ---------------------------------------------------------------
// two tables over the same buckets: 32-query tiles for the exact band / resolve kernels, 128-query tiles for the prefilter of
// the buckets with more than k_ann rows (a prefix: sizes are non-increasing)
struct FusedFlatPlan {
    std::vector<DenseJob> j32, j128;
    int64_t list_tiles32 = 0, list_tiles128 = 0, pairs = 0;
};
inline FusedFlatPlan plan_fused_flat(const std::vector<int64_t>& order, const int64_t* bucket_off, int k_ann) {
    FusedFlatPlan p;
    p.j32.reserve(order.size());
    XcdDeal x32, x128;
    for (size_t j = 0; j < order.size(); ++j) {
        const int64_t row0 = bucket_off[order[j]], nb = bucket_off[order[j] + 1] - row0;
        p.j32.push_back({row0, row0, 0, 0, (int32_t)nb, (int32_t)nb, x32.take(j, tiles_of(nb, 32))});
        if (nb > k_ann) p.j128.push_back({row0, row0, 0, 0, (int32_t)nb, (int32_t)nb, x128.take(p.j128.size(), tiles_of(nb, 128))});
        p.pairs += nb * nb;
    }
    p.list_tiles32 = x32.longest();
    p.list_tiles128 = x128.longest();
    return p;
}

// ---- indexed buckets ----------------------------------------------------------------------------------------------------
// the coarse quantiser's jobs (bucket rows x the bucket's centroids) in bucket order; they double as the IVF tile table
struct CoarsePlan {
    std::vector<DenseJob> jobs;
    int64_t tiles = 0, floats = 0;
    int max_n_list = 0;
};
inline CoarsePlan plan_coarse(const int64_t* bucket_off, const int32_t* n_list, const int64_t* list_base, int64_t n_buckets) {
    CoarsePlan p;
    for (int64_t b = 0; b < n_buckets; ++b) {
        const int64_t row0 = bucket_off[b], nb = bucket_off[b + 1] - row0;
        if (nb == 0 || n_list[b] == 1) continue;
        p.jobs.push_back({row0, list_base[b], p.floats, p.tiles, (int32_t)nb, n_list[b], 0});
        p.tiles += tiles_of(nb, 32);
        p.floats += sims_block_floats(nb, n_list[b]);
        p.max_n_list = std::max(p.max_n_list, n_list[b]);
    }
    return p;
}

// batches of whole tiles whose sims fit the buffer: [cuts[i], cuts[i + 1]); a single tile larger than the cap is a batch of its
// own (the buffer grows: need)
struct TileCuts {
    std::vector<int64_t> cuts;
    size_t need = 0;
};
inline TileCuts cut_tile_batches(const std::vector<DenseJob>& jobs, int64_t n_tiles, size_t cap) {
    TileCuts c;
    c.cuts.assign(1, 0);
    int64_t used = 0;
    for (const DenseJob& j : jobs) {
        const int64_t tiles = tiles_of(j.nq, 32), per_tile = tile_block_floats(j.nc);
        for (int64_t t = 0; t < tiles;) {
            int64_t room = ((int64_t)cap - used) / per_tile;
            if (room <= 0 && used > 0) {
                c.cuts.push_back(j.tile0 + t);
                used = 0;
                continue;
            }
            if (room <= 0) room = 1;
            const int64_t take = std::min(room, tiles - t);
            used += take * per_tile;
            c.need = std::max(c.need, (size_t)used);
            t += take;
        }
    }
    if (c.cuts.back() != n_tiles) c.cuts.push_back(n_tiles);
    return c;
}
// where tile t's block starts (jobs sorted by tile0, not empty)
inline int64_t obase_of_tile(const std::vector<DenseJob>& jobs, int64_t t) {
    size_t lo = 0, hi = jobs.size() - 1;
    while (lo < hi) {
        const size_t mid = (lo + hi + 1) / 2;
        if (jobs[mid].tile0 <= t) lo = mid; else hi = mid - 1;
    }
    return jobs[lo].obase + (t - jobs[lo].tile0) * tile_block_floats(jobs[lo].nc);
}

// batches of whole indexed buckets (every list of a bucket touches queries all over the bucket): qoff[t] = candidates of the
// tiles in front of tile t; a batch is closed by the first bucket that would take its span over cap_fine
struct BucketBatch { size_t j0, j1; };
struct BucketCuts {
    std::vector<BucketBatch> batches;
    size_t need = 0;                   // the largest batch's span
};
inline BucketCuts cut_bucket_batches(const std::vector<DenseJob>& coarse, const std::vector<int64_t>& qoff, int64_t cap_fine) {
    BucketCuts c;
    size_t j0 = 0;
    for (size_t j = 0; j < coarse.size(); ++j) {
        const int64_t end = qoff[(size_t)(coarse[j].tile0 + tiles_of(coarse[j].nq, 32))];
        if (end - qoff[(size_t)coarse[j0].tile0] > cap_fine && j > j0) {
            c.batches.push_back({j0, j});
            j0 = j;
        }
        c.need = std::max(c.need, (size_t)(end - qoff[(size_t)coarse[j0].tile0]));
    }
    c.batches.push_back({j0, coarse.size()});
    return c;
}

// the indexed buckets as 32-query tiles over sorted rows, by decreasing size (stable) and dealt to the 8 XCD lists (ivf16.hip)
struct SortedTiles32 {
    std::vector<DenseJob> j32;
    int64_t list_tiles32 = 0;
};
inline SortedTiles32 plan_sorted_tiles32(const std::vector<DenseJob>& coarse) {
    std::vector<size_t> ord(coarse.size());
    for (size_t j = 0; j < ord.size(); ++j) ord[j] = j;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return coarse[x].nq > coarse[y].nq; });
    SortedTiles32 p;
    XcdDeal x32;
    for (size_t j = 0; j < ord.size(); ++j) {
        const DenseJob& cj = coarse[ord[j]];
        p.j32.push_back({cj.q_row0, cj.c_row0, 0, 0, cj.nq, cj.nq, x32.take(j, tiles_of(cj.nq, 32))});
    }
    p.list_tiles32 = x32.longest();
    return p;
}

// the item table of dense4_kernel / dense4ab_kernel: 9 offsets (in items; words 9..15 unused), then from word 16 the
// (job, 128-row group) pairs of XCD list 0, 1, ...: job j under list j % 8 in j order, groups ascending.  table[8] = items.
inline std::vector<int32_t> dense4_items(const DenseJob* jobs_host, int n_jobs) {
    std::vector<int32_t> table(16, 0);
    for (int x = 0; x < 8; ++x) {
        for (int j = x; j < n_jobs; j += 8)
            for (int g = 0; g < (jobs_host[j].nq + 127) / 128; ++g) {
                table.push_back(j);
                table.push_back(g);
            }
        table[x + 1] = (int32_t)((table.size() - 16) / 2);
    }
    return table;
}

}  // namespace fal
