"""The references of tests/linkage_cases.py on the committed goldens, on the scipy oracle where heights are distinct and on
hand-written values; the properties of its tie inputs that test_gpu_linkage_ties.py relies on (ties at most merges, an
answer the scipy oracle does not give, an answer the opposite tie rule does not give); and the cached-partner bookkeeping
of `lk_agglomerate_big_kernel`, ported to sequential Python, against the naive agglomeration."""
import os

import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import linkage_cases as lc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = np.inf
TIE_INPUTS = ["composite", "grid256", "grid257", "few150", "few300", "csr"]


def _lists(rows):
    """[(neighbours, distances) per row] -> padded nb_idx / nb_dist"""
    k = max(len(r[0]) for r in rows)
    idx = np.full((len(rows), k), -1, np.int32)
    dist = np.full((len(rows), k), INF, np.float32)
    for i, (j, d) in enumerate(rows):
        idx[i, :len(j)] = j
        dist[i, :len(d)] = d
    return idx, dist


# --------------------------------------------------------------------------- goldens and the oracle
@pytest.mark.parametrize("method", ["single", "complete", "average"])
def test_reference_equals_every_committed_golden(method):
    g = np.load(os.path.join(GOLDEN, "linkage.npz"))
    assert int(g["n_cases"]) == 5
    for c in range(int(g["n_cases"])):
        lab = lc.linkage_ref(g[f"c{c}_idx"], g[f"c{c}_dist"], float(g[f"c{c}_t"]), method)
        assert np.array_equal(lab, g[f"c{c}_{method}"]), (c, method)


@pytest.mark.parametrize("m", [255, 256, 257])
def test_reference_equals_the_oracle_where_heights_are_distinct(m):
    idx, dist = lc.curve_graph(m, 24)
    assert m in lc.component_sizes(lc.linkage_ref(idx, dist, 0.04, "single"))       # the curve is one group at either cut
    for method, t in (("complete", 0.05), ("average", 0.04)):
        lab = lc.linkage_ref(idx, dist, t, method)
        assert np.array_equal(lab, fo.linkage_clusters(idx, dist, t, method)), method
        assert lab.max() > 20


# --------------------------------------------------------------------------- hand-written cases
def test_tie_goes_to_the_lowest_pair():
    """A chain 0 - 1 - 2 - 3 - 4, every link 0.25, every other pair missing (1.0), complete linkage cut at 0.5.  The four
    links tie.  Lowest (a, b) first: (0, 1); row 2 is then max(0.25, 1) = 1 from it, so the next is (2, 3); row 4 is 1 from
    that: [0, 0, 1, 1, -1].  The opposite rule starts at (3, 4), then (1, 2): [-1, 0, 0, 1, 1]."""
    idx, dist = _lists([([1], [.25]), ([2], [.25]), ([3], [.25]), ([4], [.25]), ([], [])])
    for method in ("complete", "average"):                      # average: (0.25 + 1) / 2 = 0.625 > 0.5, the same partition
        assert lc.linkage_ref(idx, dist, 0.5, method).tolist() == [0, 0, 1, 1, -1]
        assert lc.linkage_ref(idx, dist, 0.5, method, tie="highest").tolist() == [-1, 0, 0, 1, 1]
    assert lc.linkage_ref(idx, dist, 0.5, "single").tolist() == [0] * 5


def test_height_equal_to_the_cut_merges():
    """d01 = 0.25, d02 = d12 = 0.5, complete: (0, 1) at 0.25, then row 2 at max(0.5, 0.5) = 0.5.  Cut at exactly 0.5 the test
    is `<=`: one cluster.  One float32 ulp below, the 0.5 slots are no edges either: rows 0, 1 and a group of one."""
    idx, dist = _lists([([1, 2], [.25, .5]), ([0, 2], [.25, .5]), ([0, 1], [.5, .5])])
    assert lc.linkage_ref(idx, dist, 0.5, "complete").tolist() == [0, 0, 0]
    assert lc.linkage_ref(idx, dist, float(np.nextafter(np.float32(0.5), np.float32(0))), "complete").tolist() == [0, 0, -1]


def test_a_stored_distance_above_the_cut_enters_the_average():
    """d01 = 0.125, d12 = 0.25 and a STORED d02 = 0.75 above the cut of 0.5 (no edge, but rows 0 and 2 share a group through
    row 1).  Average: (0, 1) at 0.125, then row 2 at (0.75 + 0.25) / 2 = 0.5 <= 0.5: one cluster.  Were the slot dropped the
    pair would count as missing, (1 + 0.25) / 2 = 0.625: row 2 stays out -- as it does with complete linkage, max = 0.75."""
    idx, dist = _lists([([1, 2], [.125, .75]), ([0, 2], [.125, .25]), ([], [])])
    assert lc.linkage_ref(idx, dist, 0.5, "average").tolist() == [0, 0, 0]
    assert lc.linkage_ref(idx, dist, 0.5, "complete").tolist() == [0, 0, -1]
    idx2, dist2 = _lists([([1], [.125]), ([0, 2], [.125, .25]), ([], [])])
    assert lc.linkage_ref(idx2, dist2, 0.5, "average").tolist() == [0, 0, -1]


def test_a_pair_stored_in_one_direction_only():
    """row 1 lists row 0 (0.25), row 0 lists nobody: the edge holds in either direction and d(0, 1) = min(1, 0.25)"""
    idx, dist = _lists([([], []), ([0], [.25]), ([], [])])
    for method in ("single", "complete", "average"):
        assert lc.linkage_ref(idx, dist, 0.3, method).tolist() == [0, 0, -1]


def test_pairs_and_triples_with_ids_outside_the_table():
    """`pairs_and_triples_graph` (k = 1) cut at 0.5.  0-1: a pair.  2 -> 3: a pair (3 -> 13 is outside the 13 rows: ignored).
    4 -> 5 (0.125), 5 -> 6, 6 -> 5 (0.25): (4, 5) first, then row 6 is max(1, 0.25) = 1 or (1 + 0.25) / 2 = 0.625 away: out.
    7 -> 7: a self id, no edge.  8 -> 9 at 0.75: above the cut.  10 - 11 - 12 at 0.25 each: the tie goes to (10, 11), row 12
    stays out (the opposite rule takes (11, 12)).  Single linkage keeps the two triples whole."""
    idx, dist = lc.pairs_and_triples_graph()
    for method in ("complete", "average"):
        assert lc.linkage_ref(idx, dist, 0.5, method).tolist() == [0, 0, 1, 1, 2, 2, -1, -1, -1, -1, 3, 3, -1]
        assert lc.linkage_ref(idx, dist, 0.5, method, tie="highest").tolist() == [0, 0, 1, 1, 2, 2, -1, -1, -1, -1, -1, 3, 3]
    assert lc.linkage_ref(idx, dist, 0.5, "single").tolist() == [0, 0, 1, 1, 2, 2, 2, -1, -1, -1, 3, 3, 3]


def test_agglomerate_ref_on_a_matrix_by_hand():
    """average, sizes in the weights: d01 = 1/64, d23 = 2/64, d02 = d03 = d12 = 3/64, d13 = 5/64, cut 4/64.  (0, 1) at 1/64:
    d(01, 2) = 3/64, d(01, 3) = 4/64.  (2, 3) at 2/64: d(01, 23) = (1 * 3/64 + 1 * 4/64) / 2 = 3.5/64 <= 4/64: one cluster.
    Complete: d(01, 23) = max(3, 5)/64 > 4/64: two pairs."""
    D = np.array([[0, 1, 3, 3], [1, 0, 3, 5], [3, 3, 0, 2], [3, 5, 2, 0]], np.float64) / 64
    assert lc.agglomerate_ref(D, 4 / 64, "average").tolist() == [0, 0, 0, 0]
    assert lc.agglomerate_ref(D, 4 / 64, "complete").tolist() == [0, 0, 2, 2]
    assert lc.agglomerate_ref(D, 0.5 / 64, "complete").tolist() == [-1, -1, -1, -1]


# --------------------------------------------------------------------------- the tie inputs do what they are for
def test_composite_groups_sit_on_both_sides_of_every_stride():
    idx, dist = lc.tie_input("composite")
    single = lc.linkage_ref(idx, dist, lc.CUT["single"], "single")
    assert lc.component_sizes(single) == [2, 3, 5, 63, 64, 65, 255, 256, 257, 1024, 1025]
    assert int((single == -1).sum()) == lc.COMPOSITE_ISOLATED
    assert idx.shape == (3019 + lc.COMPOSITE_ISOLATED, lc.LATTICE_K)


@pytest.mark.parametrize("method", ["complete", "average"])
@pytest.mark.parametrize("name", TIE_INPUTS)
def test_tie_inputs_are_made_of_ties(name, method):
    """the minimum is tied at half of the merges at least (measured: 87 % .. 99 %), and a kernel with the opposite tie order
    would give other labels"""
    lab, steps, tied = lc.tie_reference(name, method)
    print(f"{name} {method}: {steps} merges, {tied} tied ({tied / steps:.3f})")
    assert steps >= 100 and 2 * tied >= steps
    opposite, _, _ = lc.tie_reference(name, method, "highest")
    assert not np.array_equal(opposite, lab)


@pytest.mark.parametrize("method", ["complete", "average"])
def test_the_scipy_oracle_cannot_pin_the_composite_graph(method):
    idx, dist = lc.tie_input("composite")
    lab, _, _ = lc.tie_reference("composite", method)
    old = fo.linkage_clusters(idx, dist, lc.CUT[method], method)
    assert int((old != lab).sum()) > 1000                       # (measured: 2,427 and 2,567 of 3,026 rows)


def test_neighbour_ids_are_distinct_within_every_row():
    """the contract of fal_linkage_cluster the builders keep (two slots of one row to one neighbour would be one matrix cell)"""
    for name in TIE_INPUTS:
        idx, _ = lc.tie_input(name)
        s = np.sort(idx, axis=1)
        assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)).any(), name


def test_few_values_inputs_have_a_degree_above_64_and_one_group():
    for name, m, big in (("few150", 150, False), ("few300", 300, True)):
        idx, dist = lc.tie_input(name)
        assert idx.shape[0] == m and idx.shape[1] > 64
        assert lc.component_sizes(lc.linkage_ref(idx, dist, lc.CUT["single"], "single")) == [m]
        assert (m > lc.WAVE_MAX) == big
        assert np.array_equal(lc.to_matrix(idx, dist), lc.few_values_matrix(m, m))


def test_csr_input_and_its_reference():
    idx, dist = lc.tie_input("csr")
    ptr, cidx, cdist = lc.neighbour_lists_to_csr(idx, dist)
    n = len(idx)
    assert lc.component_sizes(lc.linkage_ref(idx, dist, lc.CUT["single"], "single")) == [2, 3, 20, 255, 256, 257]
    assert ptr[0] == 0 and ptr[-1] == len(cidx) == len(cdist) and cidx.dtype == np.int32 and cdist.dtype == np.float64
    dense = np.ones((n, n))
    rows = np.repeat(np.arange(n), np.diff(ptr))
    dense[rows, cidx] = cdist
    assert np.array_equal(dense, dense.T)                       # symmetric, as exact mode's
    assert all(np.all(np.diff(cidx[ptr[i]:ptr[i + 1]]) > 0) for i in range(n))
    assert (cdist > lc.CUT["complete"]).any()                   # entries above the cut: no edges, yet part of the matrix
    for method in ("single", "complete"):
        assert np.array_equal(lc.linkage_ref_csr(ptr, cidx, cdist, lc.CUT[method], method),
                              lc.linkage_ref(idx, dist, lc.CUT[method], method)), method


def _by_lowest_row(lab):
    out = np.full(len(lab), -1, np.int64)
    for c in np.unique(lab[lab >= 0]):
        out[lab == c] = np.flatnonzero(lab == c).min()
    return out


@pytest.mark.parametrize("method", ["complete", "average"])
def test_the_row_that_crosses_the_cut_leaves_the_other_clusters_alone(method):
    """grid257 = grid256 + row 256.  On THIS input (not in general: other shuffles of the grid break it) the clusters that do
    not hold row 256 are those of grid256; the GPU test states the same of the two kernels."""
    a, _, _ = lc.tie_reference("grid256", method)
    b, _, _ = lc.tie_reference("grid257", method)
    assert b[256] >= 0
    keep = b[:256] != b[256]
    assert 0 < int((~keep).sum()) < 10
    assert np.array_equal(_by_lowest_row(a)[keep], _by_lowest_row(b[:256])[keep])


# --------------------------------------------------------------------------- the big kernel's bookkeeping, sequentially
def _tie_heavy_matrices():
    out = [(f"few{seed}", lc.few_values_matrix(40 + (seed * 37) % 101, seed)) for seed in range(32)]
    for seed, size in enumerate([(8, 8), (9, 7), (13, 5), (12, 11), (70, 2), (140, 1)]):
        out.append((f"lattice{size}", lc.to_matrix(*lc.lattice_graph([size], lc.LATTICE_K, seed))))
    return out


def test_cached_partner_bookkeeping_equals_the_naive_agglomeration():
    """38 tie-heavy matrices of 40 .. 140 rows, both methods, a low cut and a cut of 0.6 (long merge sequences for average:
    the 1.0 of the missing pairs enters the means).  On these the in-place replacement does not fire: before the merge either
    D[c][ba] > nnv[c] or nni[c] < ba (else ba would be row c's cached partner), the same for bb, and a reducible update
    cannot go below min(D[c][ba], D[c][bb]) -- in exact arithmetic, which is what these inputs get: every height is a small
    multiple of 1/64 or a float32, and the means of equal heights come out exact.  The test below is the other case."""
    sizes, long_runs = set(), 0
    for name, D in _tie_heavy_matrices():
        sizes.add(len(D))
        assert 40 <= len(D) <= 140
        for method in ("complete", "average"):
            for t in (2.5 / 64, 0.6):
                st = {}
                naive = lc.agglomerate_ref(D, t, method, stats=st)
                cached, replaced = lc.agglomerate_cached_ref(D, t, method)
                assert np.array_equal(cached, naive), (name, method, t)
                assert replaced == 0, (name, method, t, replaced)
                assert 2 * st["tied"] >= st["steps"] > 0 or t == 0.6, (name, method, t, st)
                long_runs += st["steps"] >= len(D) - 5
    assert len(sizes) >= 20 and long_runs >= 10


@pytest.mark.parametrize("m,seed,share,f32,t,fired", [(40, 4, 0.15, False, 0.6, 1), (40, 51, 0.15, False, 0.6, 1),
                                                      (300, 20, 0.05, True, None, 2)])
def test_in_place_replacement_fires_when_a_mean_of_equal_heights_rounds_down(m, seed, share, f32, t, fired):
    """Two heights that are no binary fractions, average linkage.  Two clusters at the SAME height x from row c merge into
    (sa*x + sb*x) / (sa + sb), which float64 rounds one ulp below x for some (x, sa, sb) -- x = 0.04097352393619469,
    sa = 25, sb = 37 is one.  That is below row c's cached nnv[c] = x: the in-place rule of `lk_agglomerate_big_kernel` is
    what keeps the cache equal to the matrix, so the branch is live on float64 heights in general (exact mode's cosines, or
    float32 distances after a few unequal means) and only dead in exact arithmetic.  The counts are those measured on these
    inputs (the first two of 60 seeds at 40 rows; the third is the GPU test's input, `rounding_input`); with the rule in
    place the bookkeeping still equals the naive agglomeration."""
    assert fired > 0
    D = lc.two_values_matrix(m, seed, share, f32)
    if t is None:
        idx, dist, t = lc.rounding_input()
        assert np.array_equal(lc.to_matrix(idx, dist), D) and idx.shape == (300, 299) and t < D.max()
    naive = lc.agglomerate_ref(D, t, "average")
    cached, replaced = lc.agglomerate_cached_ref(D, t, "average")
    assert np.array_equal(cached, naive)
    assert replaced == fired
    x = 0.04097352393619469
    assert (25.0 * x + 37.0 * x) / (25.0 + 37.0) < x


def test_rounding_input_leaves_a_partition_to_compare():
    idx, dist, t = lc.rounding_input()
    st = {}
    lab = lc.linkage_ref(idx, dist, t, "average", stats=st)
    assert lc.component_sizes(lc.linkage_ref(idx, dist, t, "single")) == [300]
    assert (st["steps"], int(lab.max()) + 1) == (251, 49) and 2 * st["tied"] >= st["steps"]
    assert not np.array_equal(lc.linkage_ref(idx, dist, t, "average", tie="highest"), lab)
