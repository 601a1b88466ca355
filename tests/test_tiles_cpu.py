"""The host tile-table builder of the tiled graph tail (`csrc/tiles.h`, plain C++) compiled on its own (tests/hostbuild.py):
whole buckets, in order, covering [0, n), every tile within the limits, closed by the first bucket that would take it over.
And the capacity rule of the DBSCAN tile kernel's edge list (`tile_dbscan_lds_bytes`, `tile_edge_capacity`): the figures its
comments state."""
import ctypes as C

import numpy as np
import pytest

from tests import hostbuild
from tests import tail_cases as tc

pytestmark = pytest.mark.skipif(not hostbuild.have_compiler(), reason="no host C++ compiler and no hipcc")

SHIM = r"""
#include "tiles.h"
extern "C" {
int t_limits(int which) { return which ? fal::kTileMaxRows : fal::kTileRows; }
// -> build_tile_table's code; *n_tiles and out[0 .. *n_tiles] filled on 0
int t_tiles(const int64_t* off, int64_t nb, int64_t n, int64_t tile_rows, int64_t max_tile, int32_t* out, int64_t* n_tiles, int64_t* max_rows) {
    std::vector<int32_t> v;
    const int rc = fal::build_tile_table(off, nb, n, tile_rows, max_tile, v, max_rows);
    *n_tiles = (int64_t)v.size() - 1;
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    return rc;
}
long long t_lds(long long max_rows) { return fal::tile_dbscan_lds_bytes(max_rows); }
// out[m] = the edge capacity of a tile of m rows in a call whose largest tile has max_rows rows, m = 0 .. max_rows
void t_caps(long long max_rows, long long* out) {
    const int64_t b = fal::tile_dbscan_lds_bytes(max_rows);
    for (long long m = 0; m <= max_rows; ++m) out[m] = fal::tile_edge_capacity(b, m);
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.compile_shim(tmp_path_factory.mktemp("tiles"), "tiles_shim", SHIM)


def caps(lib, max_rows):
    lib.t_lds.restype = C.c_longlong
    out = np.zeros(max_rows + 1, np.int64)
    lib.t_caps(C.c_longlong(max_rows), out.ctypes.data_as(C.c_void_p))
    return int(lib.t_lds(C.c_longlong(max_rows))), out


def tiles(lib, sizes, T, L):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = np.zeros(len(sizes) + 2, np.int32)
    nt, mx = C.c_int64(), C.c_int64()
    rc = lib.t_tiles(off.ctypes.data_as(C.c_void_p), C.c_int64(len(sizes)), C.c_int64(int(off[-1])), C.c_int64(T), C.c_int64(L),
                     out.ctypes.data_as(C.c_void_p), C.byref(nt), C.byref(mx))
    return rc, out[:nt.value + 1].astype(np.int64), mx.value, off


def expected(sizes, T):
    """the rule, sequentially: a bucket that would take the open tile over T closes it (unless the tile is empty)"""
    rows, start, pos = [0], 0, 0
    for s in sizes:
        if pos + s - start > T and pos > start:
            rows.append(pos)
            start = pos
        pos += s
    if pos > start:
        rows.append(pos)
    return np.array(rows, np.int64)


def test_limits(lib):
    T, L = lib.t_limits(0), lib.t_limits(1)
    # tile_members_kernel's sort key is (tile label << 16 | tile row) with 0xFFFFFFFF for a noise row: a label and a row
    # below 65,535 keep every real key under it; the bound here is the power of two below
    assert 1 <= T <= L <= 32768


@pytest.mark.parametrize("sizes", [[1024], [1025], [300, 401, 323], [300, 401, 324], [1] * 3000, [1024, 10, 20, 1024],
                                   [0, 0, 5, 0, 2000, 0, 3, 0], [8192, 1, 8192], [1], [], [0, 0], [700, 700, 700, 100, 100, 900]])
def test_table_follows_the_rule(lib, sizes):
    T, L = 1024, 8192
    rc, rows, mx, off = tiles(lib, sizes, T, L)
    assert rc == 0
    assert np.array_equal(rows, expected(sizes, T))
    assert np.array_equal(rows, tc.tile_table(sizes, T))                           # (the copy the GPU tests count tiles with)
    assert rows[0] == 0 and rows[-1] == off[-1] and np.all(np.diff(rows) > 0)      # in order, covering [0, n), no empty tile
    assert np.all(np.isin(rows, off))                                              # whole buckets
    for a, b in zip(rows[:-1], rows[1:]):
        inside = np.diff(off[(off >= a) & (off <= b)])
        assert b - a <= T or (inside > 0).sum() == 1                               # over T: one bucket alone
        assert b - a <= L
    assert mx == (np.diff(rows).max() if len(rows) > 1 else 0)


def test_random_tables(lib):
    rng = np.random.default_rng(1)
    for _ in range(50):
        sizes = rng.choice([0, 1, 2, 17, 150, 400, 1023, 1024, 1025, 3000], int(rng.integers(1, 60))).tolist()
        rc, rows, _, _ = tiles(lib, sizes, 1024, 8192)
        assert rc == 0 and np.array_equal(rows, expected(sizes, 1024))


def test_bucket_over_the_limit_and_bad_tables(lib):
    assert tiles(lib, [5, 8193, 5], 1024, 8192)[0] == 1
    off = np.array([0, 7, 5, 9], np.int64)                                          # not ascending
    out = np.zeros(8, np.int32)
    nt, mx = C.c_int64(), C.c_int64()
    call = lambda o, n: lib.t_tiles(o.ctypes.data_as(C.c_void_p), C.c_int64(len(o) - 1), C.c_int64(n), C.c_int64(1024), C.c_int64(8192),
                                    out.ctypes.data_as(C.c_void_p), C.byref(nt), C.byref(mx))
    assert call(off, 9) == -1
    assert call(np.array([1, 4], np.int64), 4) == -1                                # does not start at 0
    assert call(np.array([0, 4], np.int64), 5) == -1                                # does not end at n


def test_edge_capacity_figures(lib):
    """what tiles.h and the driver say of the edge list: four eps-edges a row for the call's largest tile up to 4,864 rows,
    shrinking from there to 6,144 edges at 8,192 rows; a smaller tile of the same call has the rest of the block (four more
    edges for every row it is shorter); the block never exceeds the CU's 160 KB less the kernels' static words, always holds the
    16 B per row of the largest tile, and no capacity is negative"""
    L = lib.t_limits(1)
    assert L == 8192
    own, lds = np.zeros(L + 1, np.int64), np.zeros(L + 1, np.int64)
    for mx in range(1, L + 1):
        lds[mx], c = caps(lib, mx)
        own[mx] = c[mx]
        assert c.min() >= 0 and c[0] == lds[mx] // 4
        assert np.all(np.diff(c) == -4)                                            # the rest of the block goes to a smaller tile
        assert lds[mx] % 16 == 0 and 16 * mx <= lds[mx]
    r = np.arange(L + 1)
    assert np.array_equal(own[1:4865], 4 * r[1:4865])                              # four edges a row ...
    assert own[4865] < 4 * 4865 and np.all(np.diff(own[4864:]) == -4)              # ... up to 4,864 rows, then shrinking
    assert own[8192] == 6144 and own[4864] == own.max() == 19456
    assert np.all(np.diff(lds[1:]) >= 0) and lds[L] == lds[4864] <= 160 * 1024 - 1024
    assert caps(lib, 5000)[1][100] == lds[5000] // 4 - 400 >= 4000                 # a dense 100-row tile beside a 5,000-row one
    assert caps(lib, 64)[1][64] == 256
    assert caps(lib, 0)[0] == 0                                                    # an empty call asks for nothing
