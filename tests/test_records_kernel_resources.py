"""Build-time guard on recwrite.hip (no GPU needed: hipcc cross-compiles): the unit's kernels are the named ones; neither builds
for gfx950 with scratch memory (the field table is a kernel argument read in place, a unit's digits live in registers); the write
kernel's static LDS is what DESIGN.md section 20 states -- four wave tiles and the staged literals -- and fits at least twice in
a CU; and there is no LDS-DMA and no inline assembly in the unit."""
import os
import re

import pytest

from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")

KERNELS = ["rec_write_sizes_kernel", "rec_write_kernel"]
TILE, WAVES, LITERALS = 8192, 4, 4096
WRITE_LDS = WAVES * TILE + LITERALS
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return L.compile_to_asm("recwrite.hip", tmp_path_factory.mktemp("isa"))


def _ours(asm, key):
    return {k: v for k, v in L.kernel_meta(asm, key).items() if "rec_" in k and "_kernel" in k}


def test_the_units_kernels_are_the_named_ones_and_use_no_scratch(asm):
    ours = _ours(asm, "private_segment_fixed_size")
    for name in KERNELS:
        assert sum(name in k for k in ours) == 1, (name, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    assert len(L.kernel_meta(asm, "private_segment_fixed_size")) == len(KERNELS), "a kernel of another name in the unit"
    spilled = {k: v for k, v in ours.items() if v != 0}
    assert not spilled, f"record-writer kernels with scratch memory: {spilled}"


def test_the_static_lds_is_the_stated_budget(asm):
    lds = _ours(asm, "group_segment_fixed_size")
    assert [v for k, v in lds.items() if "rec_write_kernel" in k] == [WRITE_LDS]
    assert [v for k, v in lds.items() if "rec_write_sizes_kernel" in k] == [0]
    assert WRITE_LDS == 36864 and 2 * WRITE_LDS <= LDS_PER_CU
    from falcon_amd import _lib
    assert LITERALS == _lib.REC_MAX_LITERALS


def test_no_lds_dma_and_no_inline_assembly_in_the_unit(asm):
    assert "global_load_lds" not in asm
    for name, body in L.kernels(asm).items():
        assert not any(s.startswith("buffer_load") and " lds" in s for s in body), name
    # (textwrite.h: the write kernel's round loop and the long unit's pieces)
    src = "".join(open(os.path.join(L.CSRC, f)).read() for f in ("recwrite.hip", "recwrite.h", "csvwrite.h", "numtext.h", "textwrite.h"))
    assert "global_load_lds" not in src and "lds_dma16(" not in src
    assert not re.search(r"\b(asm|__asm__?)\b", src), "no LDS-DMA helper, no inline assembly"
