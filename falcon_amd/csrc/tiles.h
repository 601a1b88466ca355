// Tile table of the tiled graph tail (tail.hip): plain host C++, no HIP -- tests/test_tiles_cpu.py compiles it on its own.
//
// A tile is a run of consecutive whole precursor buckets, one workgroup's work.  It is closed by the first bucket that would
// take it over kTileRows rows; a bucket of more than kTileRows rows is a tile of its own, up to kTileMaxRows rows.  No
// neighbour pair crosses a bucket (the search is bucket by bucket), so none crosses a tile: DBSCAN components, refined
// clusters and medoids are tile-local, and only their numbering needs the tiles in front (a prefix over the tile table).
//
// kTileRows = 1,024: the 700 k-row charge-2 partition of the headline (4,678 buckets, mean 150 rows) gives ~800 tiles, three
//   per CU of 512 threads each, the 300 k-row charge-3 partition ~300.  Measured (profiles/NOTES.md): 512 rows give the same
//   stage times once the tile kernels keep several rows' loads in flight -- three quarters of the 700 k partition's pairs sit in
//   buckets of more than 512 rows, tiles of their own under either limit -- and 2,048 rows leave CUs without a tile.
// kTileMaxRows = 8,192: the tile kernels keep 16 B of LDS per row (tile_dbscan_kernel: parent, border vote, root rank, row
//   length; tile_medoid_kernel: label, size, 64-bit best), 128 KB of the CU's 160 KB at the limit; the member sort packs
//   (label, row) into 16 + 16 bits of one key.  Measured at 10 M spectra (profiles/NOTES.md): the charge-3 partition (buckets of
//   ~3,750 rows, largest 4,310) runs per tile at less than half the per-row kernels' dbscan stage; the charge-2 partition
//   (buckets of ~8,750 rows, largest 9,824) and the denser configurations take the per-row kernels as before.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace fal {

constexpr int kTileRows = 1024;
constexpr int kTileMaxRows = 8192;

// Dynamic LDS of tile_dbscan_kernel.  One size per launch, so EVERY workgroup of the call gets what the call's largest tile
// needs: 16 B per row of per-row state and another 16 B per row of edge list (four eps-edges a row), as far as the CU's 160 KB
// go -- 16 B per row at kTileMaxRows plus 24 KB.  Beyond 4,864 rows the list of the largest tile shrinks, to 6,144 edges at
// 8,192 rows; a smaller tile of the same launch has the rest of the block for its list.
constexpr int64_t kTileLdsMost = 16 * (int64_t)kTileMaxRows + 24 * 1024;
// -> bytes of dynamic LDS of a call whose largest tile has max_rows rows
constexpr int64_t tile_dbscan_lds_bytes(int64_t max_rows) {
    return 32 * max_rows < kTileLdsMost ? (max_rows > 0 ? 32 * max_rows : 0) : kTileLdsMost;
}
// -> eps-edges the list of a tile of m rows holds in a block of lds_bytes (what its 16 B per row leave, in 4-byte words); a
//    tile with more eps-edges than that reads its core rows a second time.  Never negative.
constexpr int64_t tile_edge_capacity(int64_t lds_bytes, int64_t m) {
    return lds_bytes / 4 > 4 * m ? lds_bytes / 4 - 4 * m : 0;
}

// bucket_off[0 .. n_buckets]: ascending row offsets of the buckets, bucket_off[0] = 0, bucket_off[n_buckets] = n.
// -> 0: tile_row = row offsets of the tiles (n_tiles + 1 entries, whole buckets, in order, covering [0, n); empty buckets
//       belong to no tile), *max_rows = the largest tile
//    1: some bucket has more than max_tile rows (the caller takes the per-row path), tile_row is unspecified
//   -1: the table is no bucket table of n rows
static inline int build_tile_table(const int64_t* bucket_off, int64_t n_buckets, int64_t n, int64_t tile_rows, int64_t max_tile,
                                   std::vector<int32_t>& tile_row, int64_t* max_rows) {
    tile_row.clear();
    *max_rows = 0;
    if (!bucket_off || n_buckets < 0 || n < 0 || n > (int64_t)INT32_MAX || bucket_off[0] != 0 || bucket_off[n_buckets] != n) return -1;
    if (tile_rows < 1 || max_tile < tile_rows) return -1;
    tile_row.push_back(0);
    int64_t start = 0;                                    // first row of the open tile
    for (int64_t b = 0; b < n_buckets; ++b) {
        const int64_t lo = bucket_off[b], hi = bucket_off[b + 1];
        if (hi < lo) return -1;
        if (hi - lo > max_tile) return 1;
        if (hi - start > tile_rows && lo > start) {       // this bucket would take the open tile over the limit: close it
            tile_row.push_back((int32_t)lo);
            start = lo;
        }
    }
    if (n > start) tile_row.push_back((int32_t)n);
    for (size_t t = 0; t + 1 < tile_row.size(); ++t) {
        const int64_t r = (int64_t)tile_row[t + 1] - tile_row[t];
        if (r > *max_rows) *max_rows = r;
    }
    return 0;
}

}  // namespace fal
