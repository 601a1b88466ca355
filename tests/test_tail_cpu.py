"""tests/tail_cases.py held to the oracle, to the committed goldens and to results worked out by hand -- and every input of
the graph-tail tests shown to separate the rule it is there for from the rule next to it (the `variant=` of the references):
an input that gives the same result under a variant would let a kernel with that defect pass test_gpu_tail.py.  No GPU."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import tail_cases as tc


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


# --------------------------------------------------------------------------- a8
@pytest.mark.parametrize("k_ann", tc.F_K_ANN)
def test_filter_reference_equals_oracle_and_separates_its_variants(k_ann):
    mz, _ = tc.filter_rows()
    hi, up = mz[257], mz[258]
    assert abs(tc.mass_diff(hi, mz[256], False)) <= 20.0 < abs(tc.mass_diff(up, mz[256], False))
    assert np.array_equal(tc.mass_diff(mz[1:], mz[:-1], False), fo.mass_diff(mz[1:], mz[:-1], False))
    assert mz[254] - mz[253] == 0.25 and mz[255] - mz[253] > 0.25
    for nn in tc.F_N_NEIGHBORS:
        sim, idx = tc.filter_input(k_ann, nn)
        assert set(np.unique(sim).tolist()) <= {float(np.float32(1.0000001)), 1.0, float(np.float32(0.3)), 0.0, float(np.float32(-0.2))}
        if k_ann > 2:
            assert (idx[:, 1:-1] == -1).any() and (idx == np.arange(tc.F_N)[:, None]).any()
        for cfg in tc.F_CONFIGS:
            args = tc.filter_args(k_ann, nn, cfg)
            ref = tc.filter_reference(k_ann, nn, cfg)
            oi, od = fo.filter_neighbors(*args)
            assert np.array_equal(ref[0], oi) and np.array_equal(_bits(ref[1]), _bits(od)), (k_ann, nn, cfg)
            catches = tc.filter_catches(k_ann, nn, cfg)
            assert catches
            for v in catches:
                assert not _same(tc.filter_ref(*args, variant=v), ref), (k_ann, nn, cfg, v)
            if k_ann == 200 or (k_ann == 65 and nn in (1, 64)):
                # `kept` reaches n_neighbors inside the second 64-candidate chunk on some row
                full = tc.filter_ref(*args[:-1], k_ann)[0]                 # every survivor, in slot order
                hit = False
                for i in range(tc.F_N):
                    if full[i, nn - 1] >= 0:
                        slot = np.flatnonzero(idx[i] == full[i, nn - 1])[0]
                        hit |= 64 <= slot < 128
                assert hit, (k_ann, nn, cfg)


def test_filter_special_rows_by_hand():
    """k_ann 1: slot 0 of rows 253..258 is the next row of the triple (700, 700.25, next float32; 800, last float32 within
    20 ppm, first beyond): kept AT 0.25 Da, kept one float32 further on (0.000061 from its neighbour), dropped back to 700"""
    ref = tc.filter_reference(1, 1, "da")[0]
    assert ref[253:256, 0].tolist() == [254, 255, -1]
    ref = tc.filter_reference(1, 1, "ppm")[0]
    assert ref[256:259, 0].tolist() == [257, 258, -1]


# --------------------------------------------------------------------------- a9
def test_border_graph_by_hand():
    idx, dist, _ = tc.graph_input("border")
    lab, n_cl = tc.dbscan_ref(idx, dist, tc.EPS)
    assert np.array_equal(lab, tc.G_BORDER_LABELS) and n_cl == 4
    assert tc.drop_single_member_clusters(lab).tolist() == [0, 1, 0, 1, 1, 0, -1, -1, 2, 1, 0, 2]


@pytest.mark.parametrize("name", tc.graph_names())
def test_dbscan_reference_equals_oracle_and_separates_its_variants(name):
    idx, dist, count = tc.graph_input(name)
    ref = tc.dbscan_ref(idx, dist, tc.EPS, count)
    cut = tc.cut_at_count(idx, dist, count)
    assert np.array_equal(ref[0], fo.dbscan_components(*cut, tc.EPS)) and ref[1] == int(ref[0].max()) + 1
    if count is not None:                                                  # the uncounted call sees the whole rows
        assert np.array_equal(tc.dbscan_ref(idx, dist, tc.EPS)[0], fo.dbscan_components(idx, dist, tc.EPS))
    catches = tc.graph_catches(name)
    assert catches
    for v in catches:
        assert not _same(tc.dbscan_ref(idx, dist, tc.EPS, count, variant=v), ref), (name, v)
    if name.startswith("slots"):
        k = idx.shape[1]
        within = (idx >= 0) & (dist <= tc.EPS32)
        assert np.array_equal(within.sum(1), np.ones(len(idx), int))
        assert np.array_equal(np.nonzero(within)[1], np.arange(len(idx)) % k)
        assert np.array_equal(tc.g_slot_leaf_slots(k), np.arange(k))       # a row nobody else names keeps its neighbour at every slot
    if name == "eps":
        assert set(_bits(dist[idx >= 0]).tolist()) == set(_bits([tc.EPS32, tc.EPS_UP, tc.EPS_DOWN]).tolist())
    if name == "count":
        stored = (idx >= 0).sum(1)
        assert (count < stored).sum() > len(idx) // 4 and (count == 0).any() and (count == idx.shape[1] + 3).any()
        assert len(idx) % 8 != 0


def test_every_dbscan_variant_is_caught():
    caught = {v for g in tc.graph_names() for v in tc.graph_catches(g)}
    assert caught == set(tc.DBSCAN_VARIANTS)


def test_dbscan_reference_on_the_sklearn_golden(dbscan_golden):
    g = dbscan_golden
    for i in range(int(g["db_n"])):
        idx, dist, eps = g[f"db{i}_idx"], g[f"db{i}_dist"], float(g[f"db{i}_eps"])
        lab, _ = tc.dbscan_ref(idx, dist, eps)
        assert np.array_equal(lab, fo.dbscan_components(idx, dist, eps))
        assert np.array_equal(lab == -1, g[f"db{i}_labels"] == -1)


# --------------------------------------------------------------------------- a10
def test_collision_cluster_and_shortcut_pair_by_hand():
    sub, kept = tc.postprocess_ref(tc.COLLISION_MZ, tc.COLLISION_RT, 20.0, "ppm", 5.0)
    assert np.array_equal(sub, tc.COLLISION_LABELS) and kept == 5
    sub, kept = tc.postprocess_ref(tc.COLLISION_MZ, tc.COLLISION_RT, 20.0, "ppm", 5.0, variant="pairs")
    assert kept == 6
    lo = np.float32(510.0)
    at = np.array([lo, lo + np.float32(0.5)], np.float32)
    above = np.array([lo, np.nextafter(at[1], np.float32(np.inf))], np.float32)
    assert tc.postprocess_ref(at, None, 0.5, "Da", None)[0].tolist() == [0, 0]
    assert tc.postprocess_ref(above, None, 0.5, "Da", None)[0].tolist() == [-1, -1]
    hi, up = tc.ppm_pair(600.0)
    assert tc.postprocess_ref(np.array([600.0, hi], np.float32), None, 20.0, "ppm", None)[0].tolist() == [0, 0]
    assert tc.postprocess_ref(np.array([600.0, up], np.float32), None, 20.0, "ppm", None)[0].tolist() == [-1, -1]


def test_refine_reference_on_the_reference_golden(ref_golden):
    g = ref_golden
    for i in range(int(g["pp_n"])):
        tol, is_da, rt_tol, ms, sl = g[f"pp{i}_par"]
        sub, kept = tc.postprocess_ref(g[f"pp{i}_mz"].astype(np.float32), g[f"pp{i}_rt"].astype(np.float32), tol,
                                       "Da" if is_da else "ppm", None if rt_tol < 0 else rt_tol)
        exp = g[f"pp{i}_labels"].astype(np.int64)
        assert kept == int(g[f"pp{i}_n"]), i
        assert np.array_equal(sub, np.where(exp >= 0, exp - int(sl), -1)), i


@pytest.mark.parametrize("run", list(tc.R_RUNS))
def test_refine_reference_equals_oracle(run):
    lab, mz, rt, n_in, names = tc.refine_input()
    tol, mode, rt_tol = tc.R_RUNS[run]
    ref, total = tc.refine_reference(run)
    assert np.array_equal(ref, fo.refine_and_number(lab, None, mz, rt, tol, mode, rt_tol))
    assert total == int(ref.max()) + 1
    for c in names:                                                        # every cluster alone against `postprocess_cluster`
        rows = np.flatnonzero(lab == c)
        sub = np.zeros(len(rows), np.int32)
        kept = fo.postprocess_cluster(sub, mz[rows], rt[rows], tol, mode, rt_tol, 2, 0)
        mine = tc.postprocess_ref(mz[rows], rt[rows], tol, mode, rt_tol)
        assert np.array_equal(mine[0], sub) and mine[1] == kept, (run, names[c], len(rows))


def test_refine_input_has_what_it_is_there_for():
    lab, mz, rt, n_in, names = tc.refine_input()
    assert np.all(np.diff(mz) >= 0)
    used = np.unique(lab[lab >= 0])
    assert n_in > used.max() + 1 and len(used) < used.max() + 1 and n_in <= len(lab)   # ids without members, gaps
    size = np.bincount(lab[lab >= 0])
    assert (size == 1).sum() >= 6
    for pat in ("lattice", "dup_one", "dup_30ppm", "cut_da_at", "cut_da_above", "cut_ppm_at", "cut_ppm_above"):
        assert sorted(size[c] for c, p in names.items() if p == pat) == list(tc.R_SIZES)
    for c, p in names.items():
        rows = np.flatnonzero(lab == c)
        if len(rows) > 2:
            assert np.any(np.diff(rows) > 1), (p, len(rows))               # interleaved with other clusters
        da = tc.postprocess_ref(mz[rows], None, 0.5, "Da", None)
        ppm = tc.postprocess_ref(mz[rows], None, 20.0, "ppm", None)
        if p == "cut_da_at":
            assert mz[rows].max() - mz[rows].min() == 0.5 and da[1] == 1 and np.all(da[0] == 0)
        if p == "cut_da_above":
            assert mz[rows].max() - mz[rows].min() > 0.5 and not np.all(da[0] == 0)
        if p == "cut_ppm_at":
            assert ppm[1] == 1 and np.all(ppm[0] == 0)
        if p == "cut_ppm_above":
            assert not np.all(ppm[0] == 0)
        if p == "apart":
            assert len(rows) > 64 and np.all(da[0] == -1) and np.all(ppm[0] == -1)          # n_flat == m above 64 members
        if p == "apart_pair":
            assert da[1] == 1 and (da[0] == 0).sum() == 2 and (da[0] == -1).sum() == len(rows) - 2


def test_lattice_merges_are_ties():
    """share of the merges of a lattice cluster whose height another merge of the same dendrogram has: m/z 0.952 / 0.952 /
    0.953 / 0.977 / 0.985 and RT 0.968 / 0.968 / 0.969 / 0.984 / 0.990 at 63 / 64 / 65 / 129 / 200 members (the clusters of 2
    and 3 members have one and two merges: nothing to tie with)"""
    lab, mz, rt, _, names = tc.refine_input()
    seen = 0
    for c, p in names.items():
        rows = np.flatnonzero(lab == c)
        if p == "lattice" and len(rows) >= 63:
            seen += 1
            assert tc.tie_share(tc.linkage_1d_ref(mz[rows], False)) >= 0.85
            assert tc.tie_share(tc.linkage_1d_ref(rt[rows], False)) >= 0.85
            assert len(np.unique(mz[rows])) == 16 and len(np.unique(rt[rows])) == 5
    assert seen == 5


def test_refine_patterns_separate_their_variants():
    """every pattern differs from the reference under each variant it lists, at one size and run setting at least; patterns
    that list none are the far side of a threshold or a shape (n_flat == m above 64 members, ids of one member).
    "unstable" is caught by NO input and cannot be: equal values merge first, at height 0, into one flat cluster at any
    tolerance >= 0, and neither the later merges nor the walk's numbering depend on which of the equal leaves is which --
    the stability of the counting argsort is not observable on well-formed values, only its being a permutation is."""
    lab, mz, rt, _, names = tc.refine_input()
    caught = {}
    for run, (tol, mode, rt_tol) in tc.R_RUNS.items():
        for c, p in names.items():
            rows = np.flatnonzero(lab == c)
            ref = tc.postprocess_ref(mz[rows], rt[rows], tol, mode, rt_tol)
            for v in tc.REFINE_VARIANTS:
                if not _same(tc.postprocess_ref(mz[rows], rt[rows], tol, mode, rt_tol, variant=v), ref):
                    caught.setdefault(p, set()).add(v)
    for p, listed in tc.R_CATCHES.items():
        assert set(listed) <= caught.get(p, set()), (p, listed, caught.get(p))
    assert set().union(*[set(v) for v in tc.R_CATCHES.values()]) == set(tc.REFINE_VARIANTS) - {"unstable"}
    assert not any("unstable" in v for v in caught.values())


# --------------------------------------------------------------------------- a11 / a12
def _oracle_finalize(lab, order, idx, dist):
    return tc.labels_and_medoids(lab, fo.medoid_scores_sparse(lab, idx, dist), order)


@pytest.mark.parametrize("name", tc.medoid_names())
def test_medoid_reference_equals_oracle_and_separates_its_variants(name):
    lab, n_cl, order, idx, dist = tc.medoid_input(name)
    assert sorted(order.tolist()) == list(range(len(lab)))
    assert n_cl == 0 or np.array_equal(np.unique(lab[lab >= 0]), np.arange(n_cl))        # dense, every id has a member
    ref = tc.medoid_reference(name)
    assert np.array_equal(_bits(tc.medoid_scores_ref(lab, idx, dist)), _bits(fo.medoid_scores_sparse(lab, idx, dist)))
    assert _same(ref, _oracle_finalize(lab, order, idx, dist))
    assert np.array_equal(ref[0][ref[1]], np.arange(len(ref[1])))
    for v in tc.M_CATCHES[name]:
        assert not _same(tc.finalize_ref(lab, n_cl, order, idx, dist, variant=v), ref), (name, v)
    assert tc.M_CATCHES[name] or name.startswith("one_row")
    if name.startswith("wide"):
        same = (idx >= 0) & (lab[np.where(idx < 0, 0, idx)] == lab[:, None]) & (lab >= 0)[:, None] & (idx != np.arange(len(lab))[:, None])
        assert same[:, 64:].any() and not same[:, :64].any()
        assert (idx[:, :64] == np.arange(len(lab))[:, None]).any(1).all()


def test_every_medoid_and_label_variant_is_caught():
    caught = {v for m in tc.medoid_names() for v in tc.M_CATCHES[m]}
    assert caught == set(tc.MEDOID_VARIANTS) | set(tc.LABEL_VARIANTS)


def test_float_order_medoid_by_hand():
    """in slot order 0.5 + 2^-25 + 2^-25 stays 0.5 and 2^-25 + 2^-25 + 0.5 is 0.5 + 2^-24: the medoid is the cluster's second row"""
    lab, n_cl, order, idx, dist = tc.medoid_input("float_order")
    score = tc.medoid_scores_ref(lab, idx, dist)
    _, med = tc.medoid_reference("float_order")
    for c in range(n_cl):
        B, A, C, D = np.flatnonzero(lab == c)
        assert score[A] == np.float32(0.5) and score[B] == np.float32(0.5) + np.float32(2.0 ** -24) and score[C] == 3.0
        assert med[c] == order[A]


# --------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("name", tc.chain_names())
def test_chain_reference_equals_oracle(name):
    idx, dist, count, own, eps, mz, order = tc.chain_input(name)
    for counted in ((False, True) if own else (False,)):
        labels, medoids, lab, n_cl, (db, n_db) = tc.chain_reference(name, counted)
        gi, gd = tc.cut_at_count(idx, dist, count) if counted else (idx, dist)
        odb = fo.dbscan_components(gi, gd, eps)
        assert np.array_equal(db, odb)
        if np.bincount(db[db >= 0], minlength=1).max() <= 300:            # (the oracle's and the reference's a10 are quadratic)
            assert np.array_equal(lab, fo.refine_and_number(odb, None, mz, None, **tc.WIDE))
            assert np.array_equal(lab, tc.refine_ref(db, mz, None, **tc.WIDE)[0])
        assert _same((labels, medoids), _oracle_finalize(lab, order, gi, gd))
    if not own:
        assert _same(tc.chain_reference(name, True)[:4], tc.chain_reference(name, False)[:4])


def test_single_linkage_agrees_on_enough_inputs():
    ok = [c for c in tc.chain_names() if tc.single_linkage_agrees(c)]
    assert len(ok) >= 20 and "G:hub_core" in ok and "M:cliques" in ok and "M:big" in ok
    for c in ok[:3] + ["M:cliques"]:
        idx, dist, _, _, eps, _, _ = tc.chain_input(c)
        assert np.array_equal(tc.single_linkage_ref(idx, dist, eps), fo.linkage_clusters(idx, dist, eps, "single"))
