"""The two agglomeration kernels of csrc/linkage.hip on inputs made of ties, against the plain reference of
tests/linkage_cases.py (pinned itself by test_linkage_cpu.py): `lk_agglomerate_kernel` (one wave a group, up to 256 rows) and
`lk_agglomerate_big_kernel` (1,024 threads, cached nearest partners) must make the same merges in the same order --
smallest height, ties -> lowest (a, b) -- on both sides of the 256-row cut, of the wave kernel's 64-lane strides and of the
big kernel's 1,024-thread stride, with several big groups in one launch and with more than 64 slots a row.  Every comparison
is `np.array_equal` on integer labels: no tolerance, no ARI."""
import numpy as np
import pytest

from tests import linkage_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _dev(ctx, name):
    import torch
    idx, dist = lc.tie_input(name)
    return torch.from_numpy(idx).to(ctx.tdev), torch.from_numpy(dist).to(ctx.tdev)


def _check(ctx, ti, td, t, method, ref, what):
    lab, n_cl = ctx.linkage_cluster(ti, td, t, method)
    lab = lab.cpu().numpy()
    assert np.array_equal(lab, ref), (what, method, int((lab != ref).sum()))
    assert n_cl == int(ref.max()) + 1, (what, method)
    return lab


@pytest.mark.parametrize("method", ["complete", "average"])
def test_both_kernels_at_every_stride_and_the_cut(ctx, method):
    """one call: groups of 2, 3, 5, 63, 64, 65, 255 and 256 rows (the wave kernel: below, at and above one and four rounds of
    its 64-lane loops) and of 257, 1,024 and 1,025 rows (three workgroups of the big kernel: just above the cut, one full
    round of its 1,024-thread loops, one row into the second), shuffled, 7 isolated rows"""
    idx, dist = lc.tie_input("composite")
    single = lc.linkage_ref(idx, dist, lc.CUT["single"], "single")
    sizes = lc.component_sizes(single)
    assert sizes == [2, 3, 5, 63, 64, 65, 255, 256, 257, 1024, 1025]
    assert sum(s > lc.WAVE_MAX for s in sizes) == 3
    ref, _, _ = lc.tie_reference("composite", method)
    _check(ctx, *_dev(ctx, "composite"), lc.CUT[method], method, ref, "composite")


@pytest.mark.parametrize("method", ["complete", "average"])
def test_wave_and_big_kernel_agree_on_the_same_matrix(ctx, method):
    """a 16 x 16 lattice (256 rows: the wave kernel) and the same rows plus one that continues the first grid row (257 rows,
    the new one the highest-numbered member: the big kernel).  Each equals its own reference; and, as the reference confirms
    for this input (test_linkage_cpu.py), the clusters without row 256 are the same under both kernels."""
    labs = {}
    for name in ("grid256", "grid257"):
        ref, _, _ = lc.tie_reference(name, method)
        labs[name] = _check(ctx, *_dev(ctx, name), lc.CUT[method], method, ref, name)
    a, b = labs["grid256"], labs["grid257"]
    keep = b[:256] != b[256]
    first_row = lambda lab: np.array([np.flatnonzero(lab == c)[0] if c >= 0 else -1 for c in lab])
    assert np.array_equal(first_row(a)[keep], first_row(b[:256])[keep])


@pytest.mark.parametrize("method", ["complete", "average"])
def test_k_above_64_and_k_of_1(ctx, method):
    """more than 64 slots a row takes the wave kernel's `s = lane; s < k; s += 64` fill loop round twice (150 rows, k = 125)
    and the big kernel's `e / k`, `e % k` over 300 x 244 slots; k = 1 is the other end"""
    import torch
    for name, m in (("few150", 150), ("few300", 300)):
        idx, _ = lc.tie_input(name)
        assert idx.shape[0] == m and idx.shape[1] > 64
        ref, _, _ = lc.tie_reference(name, method)
        assert ref.max() > 20
        _check(ctx, *_dev(ctx, name), lc.CUT[method], method, ref, name)
    idx, dist = lc.pairs_and_triples_graph()
    assert idx.shape[1] == 1
    ref = lc.linkage_ref(idx, dist, 0.5, method)
    assert ref.tolist() == [0, 0, 1, 1, 2, 2, -1, -1, -1, -1, 3, 3, -1]
    _check(ctx, torch.from_numpy(idx).to(ctx.tdev), torch.from_numpy(dist).to(ctx.tdev), 0.5, method, ref, "k = 1")


def test_in_place_replacement_of_the_big_kernel(ctx):
    """average linkage of 300 rows whose heights are two float32 values that are no binary fractions: on the way to the cut
    a mean of two equal heights rounds below them and the in-place rule of the cached-partner bookkeeping fires (twice in
    the sequential port, test_linkage_cpu.py) -- `nnv[c]` / `nni[c]` written by the thread that owns c, read by the next
    step's reduction.  No input was found whose LABELS change when the rule is left out (the stale entry is one ulp off), so
    this runs the branch and holds the result to the reference; it does not prove the branch necessary."""
    import torch
    idx, dist, t = lc.rounding_input()
    assert idx.shape[0] > lc.WAVE_MAX
    ref = lc.linkage_ref(idx, dist, t, "average")
    assert ref.max() + 1 == 49
    _check(ctx, torch.from_numpy(idx).to(ctx.tdev), torch.from_numpy(dist).to(ctx.tdev), t, "average", ref, "two values")


def test_single_linkage_and_noise_rows(ctx):
    """the components themselves, numbered by their lowest row; the 7 isolated rows (every stored neighbour above the cut)
    are noise under every method"""
    import torch
    idx, dist = lc.tie_input("composite")
    ref = lc.linkage_ref(idx, dist, lc.CUT["single"], "single")
    assert int((ref == -1).sum()) == lc.COMPOSITE_ISOLATED and ref.max() + 1 == 11
    lab = _check(ctx, *_dev(ctx, "composite"), lc.CUT["single"], "single", ref, "composite")
    first = [int(np.flatnonzero(lab == c)[0]) for c in range(11)]
    assert first == sorted(first)
    idx, dist = lc.pairs_and_triples_graph()
    ref = lc.linkage_ref(idx, dist, 0.5, "single")
    _check(ctx, torch.from_numpy(idx).to(ctx.tdev), torch.from_numpy(dist).to(ctx.tdev), 0.5, "single", ref, "k = 1")


@pytest.mark.parametrize("method", ["complete", "single"])
def test_csr_source_at_the_cut(ctx, method):
    """`fal_linkage_cluster_csr` (no peaks: average linkage scores the pairs again and belongs to test_gpu_exact_paths.py):
    groups of 255, 256 and 257 rows next to groups of 2, 3 and 20, as the symmetric float64 CSR exact mode hands over"""
    import torch
    idx, dist = lc.tie_input("csr")
    ptr, cidx, cdist = lc.neighbour_lists_to_csr(idx, dist)
    ref = lc.linkage_ref_csr(ptr, cidx, cdist, lc.CUT[method], method)
    assert lc.component_sizes(lc.linkage_ref_csr(ptr, cidx, cdist, lc.CUT["single"], "single")) == [2, 3, 20, 255, 256, 257]
    lab, n_cl = ctx.linkage_cluster_csr(*(torch.from_numpy(x).to(ctx.tdev) for x in (ptr, cidx, cdist)), lc.CUT[method], method)
    lab = lab.cpu().numpy()
    assert np.array_equal(lab, ref), (method, int((lab != ref).sum()))
    assert n_cl == int(ref.max()) + 1


def test_repeat_calls_give_the_same_labels(ctx):
    """the member lists and the list of big groups are filled through atomics, in another order every call: three calls per
    method, the same labels"""
    ti, td = _dev(ctx, "composite")
    for method in ("complete", "average"):
        ref, _, _ = lc.tie_reference("composite", method)
        for call in range(3):
            _check(ctx, ti, td, lc.CUT[method], method, ref, f"call {call}")
