"""Build-time guard on network.hip (no GPU needed: hipcc cross-compiles): the unit's kernels are the named ones; none of them, the tile kernel and both forms of the greedy kernel included, builds for gfx950 with scratch memory
(the window walks and the greedy rounds keep their state in registers and LDS); the tile kernel's static LDS is what DESIGN.md
states and fits three workgroups per CU; and there is no LDS-DMA and no inline assembly in the unit."""
import os
import re

import pytest

from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")

KERNELS = ["net_prepare_kernel", "net_band_kernel", "net_tile_kernel", "net_greedy_kernelILi64E", "net_greedy_kernelILi4096E",
           "net_rank_entries_kernel", "net_rank_mark_kernel", "net_keep_kernel", "net_output_kernel"]
# two sides of 3,200 staged peaks (m/z + intensity, 4 bytes each), per side the 64 global offsets (8 bytes), 128 lengths / LDS
# offsets, the total and the 64 precursors (4 bytes)
TILE_LDS = 2 * (3200 * 8 + 64 * 8 + 128 * 4 + 4 + 64 * 4)
# per listed peak of the a side its offer's weight and partner (4 bytes each), one bit per peak of the b side
GREEDY_LDS = {64: 64 * 8 + 64 // 8, 4096: 4096 * 8 + 4096 // 8}
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return L.compile_to_asm("network.hip", tmp_path_factory.mktemp("isa"))


def _ours(asm, key):
    return {k: v for k, v in L.kernel_meta(asm, key).items() if "net_" in k and "_kernel" in k}


def test_the_units_kernels_are_the_named_ones_and_use_no_scratch(asm):
    ours = _ours(asm, "private_segment_fixed_size")
    for name in KERNELS:
        assert sum(name in k for k in ours) == 1, (name, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    # (no sort is instantiated here: the unit borrows exact.hip's 64-bit pair sort)
    assert len(L.kernel_meta(asm, "private_segment_fixed_size")) == len(KERNELS), "a kernel of another name in the unit"
    spilled = {k: v for k, v in ours.items() if v != 0}
    assert not spilled, f"network kernels with scratch memory: {spilled}"


def test_the_static_lds_is_the_stated_budget(asm):
    lds = _ours(asm, "group_segment_fixed_size")
    tile = [v for k, v in lds.items() if "net_tile_kernel" in k]
    assert tile == [TILE_LDS] and TILE_LDS == 53768 and 3 * TILE_LDS <= LDS_PER_CU
    for cap, want in GREEDY_LDS.items():
        assert [v for k, v in lds.items() if f"net_greedy_kernelILi{cap}E" in k] == [want], cap
    assert GREEDY_LDS[4096] == 33280 and GREEDY_LDS[64] == 520


def test_no_lds_dma_and_no_inline_assembly_in_the_unit(asm):
    assert "global_load_lds" not in asm
    for name, body in L.kernels(asm).items():
        assert not any(s.startswith("buffer_load") and " lds" in s for s in body), name
    src = "".join(open(os.path.join(L.CSRC, f)).read() for f in ("network.hip", "nettile.h", "netmatch.h"))
    assert "global_load_lds" not in src and "lds_dma16(" not in src
    assert not re.search(r"\b(asm|__asm__?)\b", src), "no LDS-DMA helper, no inline assembly"
