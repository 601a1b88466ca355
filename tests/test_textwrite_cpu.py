"""What the device text writers share, on the host (no GPU needed): `csrc/textwrite.h`'s flush plan -- which bytes of a wave's tile
go out singly, which as 16-byte units and which are carried over -- through a host build of the header the kernels include,
and `device.chunk_cuts`, the cut list of `format_mgf` / `format_csv`'s chunk loop."""
import ctypes as C

import numpy as np
import pytest

from tests.hostbuild import _p, compile_shim, have_compiler

SHIM = r"""
#include <stdint.h>
#include "textwrite.h"

extern "C" void t_flush_plan(int lo, int hi, int32_t* out) {
    const fal::FlushPlan p = fal::flush_plan(lo, hi);
    out[0] = p.u0;
    out[1] = p.u1;
    out[2] = p.head_end;
    out[3] = p.rest;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not have_compiler():
        pytest.skip("no host C++ compiler")
    lib = compile_shim(tmp_path_factory.mktemp("textwriteshim"), "textwrite_shim", SHIM)
    lib.t_flush_plan.argtypes, lib.t_flush_plan.restype = [C.c_int, C.c_int, C.c_void_p], None
    out = np.zeros(4, np.int32)

    def call(lo, hi):
        lib.t_flush_plan(lo, hi, _p(out))
        return tuple(int(v) for v in out)
    return call


RANGES = [(lo, hi) for lo in range(48) for hi in range(lo, lo + 97)]


def _lane_stores(lo, hi, u0, u1, head_end, rest, final):
    """`tile_flush`'s stores over its 64 lanes -> (stores per tile byte, the unit stores' byte offsets)"""
    count = np.zeros(hi + 16, np.int32)
    units = []
    for lane in range(64):
        if lo + lane < head_end:
            count[lo + lane] += 1
        for u in range(u0 + lane, u1, 64):
            count[16 * u:16 * u + 16] += 1
            units.append(16 * u)
        if final and rest + lane < hi:
            count[rest + lane] += 1
    return count, units


def test_final_flush_stores_every_byte_once(plan):
    """every lo in 0..47 x hi in lo..lo + 96: each byte of [lo, hi) is stored exactly once and nothing outside it, the unit stores
    are 16-byte aligned, and fewer than 16 bytes go out singly in front of them and behind them"""
    for lo, hi in RANGES:
        u0, u1, head_end, rest = plan(lo, hi)
        count, units = _lane_stores(lo, hi, u0, u1, head_end, rest, final=True)
        want = np.zeros_like(count)
        want[lo:hi] = 1
        assert np.array_equal(count, want), (lo, hi)
        assert all(at % 16 == 0 and lo <= at and at + 16 <= hi for at in units), (lo, hi)
        assert 0 <= head_end - lo < 16 and 0 <= hi - rest < 16 and lo <= head_end <= rest <= hi, (lo, hi)


def test_carry_over_flush_partitions_the_range(plan):
    """the form between two rounds: with a complete unit in the range, the stored bytes and the carried remainder [rest, hi)
    partition [lo, hi), the remainder is under 16 bytes and the new base (the old one + rest) is 16-byte aligned; without one
    (`tile_flush` returns before it stores: u1 <= u0) the range stays in the tile as it is, under 31 bytes"""
    for lo, hi in RANGES:
        u0, u1, head_end, rest = plan(lo, hi)
        if u1 <= u0:
            assert hi - lo < 31, (lo, hi)
            continue
        count, units = _lane_stores(lo, hi, u0, u1, head_end, rest, final=False)
        want = np.zeros_like(count)
        want[lo:rest] = 1
        assert np.array_equal(count, want), (lo, hi)
        assert all(at % 16 == 0 for at in units) and lo <= rest <= hi and hi - rest < 16 and rest % 16 == 0, (lo, hi)


def test_chunk_cuts():
    from falcon_amd.device import chunk_cuts
    sizes = [10, 20, 5, 100, 1, 1, 30, 64, 7]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = len(sizes)
    # 40 bytes: [10, 20, 5] fit, the unit of 100 is larger and grows a chunk of its own, as does the one of 64
    assert chunk_cuts(off, 40) == [0, 3, 4, 7, 8, 9]
    assert chunk_cuts(off, 1) == list(range(n + 1)) == chunk_cuts(off, 0)            # a unit a chunk
    assert chunk_cuts(off, 35) == [0, 3, 4, 7, 8, 9] and chunk_cuts(off, 30) == [0, 2, 3, 4, 6, 7, 8, 9]
    assert chunk_cuts(off, 10 ** 9) == [0, n]
    for max_bytes in (1, 7, 30, 40, 64, 100, 238, 239):
        cuts = chunk_cuts(off, max_bytes)
        assert cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts[:-1], cuts[1:]))
        # a chunk above the target is one unit; no chunk could have taken the next unit as well
        assert all(off[b] - off[a] <= max_bytes or b == a + 1 for a, b in zip(cuts[:-1], cuts[1:]))
        assert all(b == n or off[b + 1] - off[a] > max_bytes for a, b in zip(cuts[:-1], cuts[1:]))
    zeros = np.zeros(4, np.int64)                                                      # empty units: one chunk takes them all
    assert chunk_cuts(zeros, 1) == [0, 3] and chunk_cuts(np.zeros(1, np.int64), 5) == [0]
