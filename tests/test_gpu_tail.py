"""The graph tail -- `filter_kernel`, the DBSCAN kernels (wave-per-row and counted core pass, edges), `refine_kernel`, both
medoid kernels and `finalize_kernel`, staged and behind the fused `fal_cluster_graph` / `fal_cluster_graph_counted` /
`fal_cluster_graph_linkage` -- on the tie-heavy and slot-edge inputs of tests/tail_cases.py, against its plain references
(held to the oracle, the goldens and hand-worked results by test_tail_cpu.py, which also shows what each input separates).
Every comparison is `np.array_equal` on integers or on float32 bit patterns; every input runs once."""
import numpy as np
import pytest

from tests import tail_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _dev(ctx, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.tdev)


def _np(t):
    return t.cpu().numpy()


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


@pytest.mark.parametrize("k_ann", tc.F_K_ANN)
def test_filter(ctx, k_ann):
    mz, rt = tc.filter_rows()
    for nn in tc.F_N_NEIGHBORS:
        sim, idx = tc.filter_input(k_ann, nn)
        for cfg, (tol, mode, rt_tol, with_rt) in tc.F_CONFIGS.items():
            ri, rd = tc.filter_reference(k_ann, nn, cfg)
            gi, gd = ctx.filter_neighbors(_dev(ctx, sim), _dev(ctx, idx), _dev(ctx, mz), _dev(ctx, rt if with_rt else None),
                                          tol, mode, rt_tol, nn)
            assert np.array_equal(_np(gi), ri), (k_ann, nn, cfg)
            assert np.array_equal(_bits(_np(gd)), _bits(rd)), (k_ann, nn, cfg)


@pytest.mark.parametrize("name", tc.graph_names())
def test_dbscan(ctx, name):
    """`fal_dbscan` on the whole rows (the holes version of the slot inputs included)"""
    idx, dist, _ = tc.graph_input(name)
    ref, n_ref = tc.dbscan_ref(idx, dist, tc.EPS)
    lab, n_cl = ctx.dbscan(_dev(ctx, idx), _dev(ctx, dist), tc.EPS)
    assert np.array_equal(_np(lab), ref), name
    assert n_cl == n_ref, name


@pytest.mark.parametrize("run", list(tc.R_RUNS))
def test_refine(ctx, run):
    lab, mz, rt, n_in, _ = tc.refine_input()
    tol, mode, rt_tol = tc.R_RUNS[run]
    ref, total = tc.refine_reference(run)
    out, n_out = ctx.refine_clusters(_dev(ctx, lab.copy()), n_in, _dev(ctx, mz), _dev(ctx, rt), tol, mode, rt_tol)
    assert np.array_equal(_np(out), ref), run
    assert n_out == total, run


@pytest.mark.parametrize("name", tc.medoid_names())
def test_finalize(ctx, name):
    """`fal_finalize`: the wave-per-row medoid kernel on handed-in labels under a random row_order"""
    lab, n_cl, order, idx, dist = tc.medoid_input(name)
    rl, rm = tc.medoid_reference(name)
    labels, medoids = ctx.finalize(_dev(ctx, lab), n_cl, _dev(ctx, order), _dev(ctx, idx), _dev(ctx, dist))
    assert np.array_equal(_np(labels), rl), name
    assert np.array_equal(_np(medoids), rm), name


def _check_fused(out, ref, what):
    labels, medoids, lab_sorted, n_cl = out
    assert np.array_equal(_np(lab_sorted), ref[2]), what
    assert n_cl == ref[3], what
    assert np.array_equal(_np(labels), ref[0]), what
    assert np.array_equal(_np(medoids), ref[1]), what


@pytest.mark.parametrize("name", tc.chain_names())
def test_fused_equals_staged_equals_reference(ctx, name):
    """a9 -> a10 -> a11 / a12 on every G and M graph, one m/z for all rows and a tolerance that splits nothing (the labels
    are then DBSCAN's with the one-member clusters dropped: test_tail_cpu.py): the fused call (rows medoid kernel), the
    counted call (counted core pass; on the graph cut at nb_count where the input has counts, else nb_count = k), single
    linkage behind the fused call (wave medoid kernel) where it must give the same labels, and the three staged calls"""
    idx, dist, count, own, eps, mz, order = tc.chain_input(name)
    ti, td, tm, to = _dev(ctx, idx), _dev(ctx, dist), _dev(ctx, mz), _dev(ctx, order)
    tol, mode, rt_tol = tc.WIDE["tol"], tc.WIDE["mode"], tc.WIDE["rt_tol"]
    ref = tc.chain_reference(name, False)
    _check_fused(ctx.cluster_graph(ti, td, eps, tm, None, tol, mode, rt_tol, to), ref, (name, "fused"))
    _check_fused(ctx.cluster_graph(ti, td, eps, tm, None, tol, mode, rt_tol, to, nb_count=_dev(ctx, count)),
                 tc.chain_reference(name, True), (name, "counted"))
    if tc.single_linkage_agrees(name):
        _check_fused(ctx.cluster_graph(ti, td, eps, tm, None, tol, mode, rt_tol, to, linkage="single"), ref, (name, "single"))
    db, n_db = ctx.dbscan(ti, td, eps)
    assert np.array_equal(_np(db), ref[4][0]) and n_db == ref[4][1], name
    lab, n_cl = ctx.refine_clusters(db, n_db, tm, None, tol, mode, rt_tol)
    assert np.array_equal(_np(lab), ref[2]) and n_cl == ref[3], name
    labels, medoids = ctx.finalize(lab, n_cl, to, ti, td)
    assert np.array_equal(_np(labels), ref[0]) and np.array_equal(_np(medoids), ref[1]), name
