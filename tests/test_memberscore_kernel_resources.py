"""Build-time guard on memberscore.hip (no GPU needed: hipcc cross-compiles): the unit's kernels are the named ones; the score
kernel and the summary's kernels build for gfx950 without scratch memory (the window walk and the cluster fold keep their state
in registers; the solver kernel holds the Hungarian algorithm's per-lane arrays and may use it); the score kernel's static LDS
is what DESIGN.md states; and there is no LDS-DMA in the unit."""
import os
import re

import pytest

from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")

KERNELS = ["ms_label_keys_kernel", "ms_cluster_start_kernel", "ms_score_kernel", "ms_fallback_kernel", "ms_summary_kernel"]
MAY_SPILL = ["ms_fallback_kernel"]
# two sides of 3,200 staged peaks (m/z + intensity, 4 bytes each), per side the 64 global offsets (8 bytes), 128 lengths / LDS
# offsets and the total (4 bytes); the tile's runs: cluster and representative row (64 x 4 bytes each)
SCORE_LDS = 2 * (3200 * 8 + 64 * 8 + 128 * 4 + 4) + 2 * 64 * 4


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return L.compile_to_asm("memberscore.hip", tmp_path_factory.mktemp("isa"))


def _ours(asm, key):
    return {k: v for k, v in L.kernel_meta(asm, key).items() if "ms_" in k and "_kernel" in k}


def test_the_units_kernels_are_the_named_ones_and_use_no_scratch(asm):
    ours = _ours(asm, "private_segment_fixed_size")
    for name in KERNELS:
        assert sum(name in k for k in ours) == 1, (name, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    assert len(L.kernel_meta(asm, "private_segment_fixed_size")) == len(KERNELS), "a kernel of another name in the unit"
    spilled = {k: v for k, v in ours.items() if v != 0 and not any(m in k for m in MAY_SPILL)}
    assert not spilled, f"member-score kernels with scratch memory: {spilled}"


def test_the_score_kernels_static_lds_is_the_stated_budget(asm):
    lds = {k: v for k, v in _ours(asm, "group_segment_fixed_size").items() if "ms_score_kernel" in k}
    assert list(lds.values()) == [SCORE_LDS] and SCORE_LDS == 53768 and SCORE_LDS <= 64 * 1024


def test_no_lds_dma_in_the_unit(asm):
    assert "global_load_lds" not in asm
    for name, body in L.kernels(asm).items():
        assert not any(s.startswith("buffer_load") and " lds" in s for s in body), name
    src = open(os.path.join(L.CSRC, "memberscore.hip")).read() + open(os.path.join(L.CSRC, "memberscore.h")).read()
    assert "lds_dma16(" not in src and not re.search(r"\b(asm|__asm__?)\b", src), "no LDS-DMA helper, no inline assembly"
