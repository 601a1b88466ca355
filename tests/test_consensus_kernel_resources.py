"""Build-time guard on consensus.hip (no GPU needed: hipcc cross-compiles): every kernel of the consensus stage builds for
gfx950 without scratch memory -- the group walk keeps its float64 sums in registers, and a spill would put a memory round
trip into every step of that sequential chain -- and without LDS-DMA."""
import os

import pytest

from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")

KERNELS = ["cons_label_keys_kernel", "cons_member_counts_kernel", "cons_cluster_start_kernel", "cons_cluster_sizes_kernel",
           "cons_pool_kernel", "cons_sort_lds_kernel", "cons_big_keys_kernel", "cons_big_cluster_keys_kernel",
           "cons_big_scatter_kernel", "cons_groups_kernel", "cons_out_counts_kernel", "cons_emit_kernel"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return L.compile_to_asm("consensus.hip", tmp_path_factory.mktemp("isa"))


def test_every_consensus_kernel_is_there_and_uses_no_scratch(asm):
    meta = L.kernel_meta(asm, "private_segment_fixed_size")
    ours = {k: v for k, v in meta.items() if "cons_" in k}
    for name in KERNELS:
        assert sum(name in k for k in ours) == 1, (name, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    spilled = {k: v for k, v in ours.items() if v != 0}
    assert not spilled, f"consensus kernels with scratch memory: {spilled}"


def test_the_lds_sort_holds_one_cluster_of_the_cut(asm):
    from falcon_amd import _lib
    lds = {k: v for k, v in L.kernel_meta(asm, "group_segment_fixed_size").items() if "cons_sort_lds_kernel" in k}
    assert list(lds.values()) == [8 * _lib.CONS_LDS_PEAKS]


def test_no_lds_dma_in_the_consensus_kernels(asm):
    for name, body in L.kernels(asm).items():
        if "cons_" in name:
            assert not any("global_load_lds" in s or (s.startswith("buffer_load") and " lds" in s) for s in body), name
