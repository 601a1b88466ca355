"""Build-time guard on families.hip (no GPU needed: hipcc cross-compiles): the unit's kernels are the named ones and no other (no
rocPRIM algorithm is instantiated here: the numbering borrows the library's scan); none builds for gfx950 with scratch memory;
none has static LDS, as DESIGN.md states; there is no floating-point atomic, no LDS-DMA and no inline assembly in the unit."""
import os
import re

import pytest

from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")

KERNELS = ["fam_check_kernel", "fam_init_kernel", "fam_hook_kernel", "fam_find_kernel", "fam_lo_kernel", "fam_cut_kernel",
           "fam_flag_kernel", "fam_number_kernel", "fam_rounds_kernel"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return L.compile_to_asm("families.hip", tmp_path_factory.mktemp("isa"))


def _ours(asm, key):
    return {k: v for k, v in L.kernel_meta(asm, key).items() if "fam_" in k and "_kernel" in k}


def test_the_units_kernels_are_the_named_ones_and_use_no_scratch(asm):
    ours = _ours(asm, "private_segment_fixed_size")
    for name in KERNELS:
        assert sum(name in k for k in ours) == 1, (name, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    assert len(L.kernel_meta(asm, "private_segment_fixed_size")) == len(KERNELS), "a kernel of another name in the unit"
    spilled = {k: v for k, v in ours.items() if v != 0}
    assert not spilled, f"family kernels with scratch memory: {spilled}"


def test_no_kernel_has_static_lds(asm):
    lds = _ours(asm, "group_segment_fixed_size")
    assert len(lds) == len(KERNELS) and all(v == 0 for v in lds.values()), lds


def test_integer_atomics_only_no_lds_dma_and_no_inline_assembly(asm):
    bodies = L.kernels(asm)
    atomics = {name: [s.split()[0] for s in body if "atomic" in s.split()[0]] for name, body in bodies.items()}
    used = {op for ops in atomics.values() for op in ops}
    assert used and all(re.fullmatch(r"(global|flat)_atomic_(cmpswap|add|umin|add_x2)(_u32|_u64|_b32)?", op) for op in used), used
    # the hook kernel's compare-and-swap, the find's count, the lo kernel's minimum, the cut count
    for kernel, op in (("fam_hook_kernel", "cmpswap"), ("fam_find_kernel", "add"), ("fam_lo_kernel", "umin"), ("fam_rounds_kernel", "add")):
        assert any(op in o for name, ops in atomics.items() if kernel in name for o in ops), (kernel, atomics)
    assert "global_load_lds" not in asm
    for name, body in bodies.items():
        assert not any(s.startswith("buffer_load") and " lds" in s for s in body), name
    src = "".join(open(os.path.join(L.CSRC, f)).read() for f in ("families.hip", "netfamily.h", "unionfind.h"))
    assert "global_load_lds" not in src and "lds_dma16(" not in src
    assert not re.search(r"\b(asm|__asm__?)\b", src), "no LDS-DMA helper, no inline assembly"
    assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", src)
