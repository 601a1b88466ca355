"""Build-time guard on propagate.hip (no GPU needed: hipcc cross-compiles): the unit's kernels are the named ones and no other;
none builds for gfx950 with scratch memory; none has static LDS, as DESIGN.md states; the unit's source text holds no
floating-point atomic call and no inline assembly."""
import os
import re

import pytest

from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")

KERNELS = ["prop_check_kernel", "prop_init_kernel", "prop_relax_kernel", "prop_commit_kernel", "prop_emit_kernel"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return L.compile_to_asm("propagate.hip", tmp_path_factory.mktemp("isa"))


def _ours(asm, key):
    return {k: v for k, v in L.kernel_meta(asm, key).items() if "prop_" in k and "_kernel" in k}


def test_the_units_kernels_are_the_named_ones_and_use_no_scratch(asm):
    ours = _ours(asm, "private_segment_fixed_size")
    for name in KERNELS:
        assert sum(name in k for k in ours) == 1, (name, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    assert len(L.kernel_meta(asm, "private_segment_fixed_size")) == len(KERNELS), "a kernel of another name in the unit"
    spilled = {k: v for k, v in ours.items() if v != 0}
    assert not spilled, f"propagation kernels with scratch memory: {spilled}"


def test_no_kernel_has_static_lds(asm):
    lds = _ours(asm, "group_segment_fixed_size")
    assert len(lds) == len(KERNELS) and all(v == 0 for v in lds.values()), lds


def test_no_floating_point_atomic_call_and_no_inline_assembly_in_the_source():
    src = "".join(open(os.path.join(L.CSRC, f)).read() for f in ("propagate.hip", "netpropagate.h", "netfamily.h"))
    assert not re.search(r"\b(asm|__asm__?)\b", src), "inline assembly"
    assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", src)
    # every atomic call of the unit is one of the two integer ones: the key's maximum and the reached count
    calls = re.findall(r"\batomic\w+\s*\(", open(os.path.join(L.CSRC, "propagate.hip")).read())
    assert sorted(c.rstrip("( ") for c in calls) == ["atomicAdd", "atomicMax"], calls
