"""`fal_cluster_graph_tiled` -- the graph tail per bucket tile (tile_dbscan / tile_members / tile_medoid kernels, DESIGN
section 3) -- against `fal_cluster_graph_counted`, the three staged calls and the plain references of tests/tail_cases.py.
Every case expects all four equal in labels, medoids, sorted labels and both counts (`np.array_equal` on integers), and
names the path that has to have run (`fal_ctx_counter(10)`).  The tile limits come from the library (`fal_graph_tile_limits`)."""
import functools

import numpy as np
import pytest

from tests import tail_cases as tc

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def limits(ctx):
    return ctx.graph_tile_limits()


def _dev(ctx, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.tdev)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------- inputs
def replicate(idx, dist, count, fillers):
    """the graph once per entry of `fillers`, each copy a bucket of its own with its ids shifted, followed by a bucket of
    `filler` rows that store nothing (noise): buckets of unequal size -> idx, dist, count, splits"""
    n, k = idx.shape
    I, D, Cn, splits, off = [], [], [], [0], 0
    for fill in fillers:
        I.append(np.where(idx >= 0, idx + off, idx).astype(np.int32))
        D.append(dist)
        Cn.append(count)
        off += n
        splits.append(off)
        if fill:
            I.append(np.full((fill, k), -1, np.int32))
            D.append(np.full((fill, k), np.inf, f32))
            Cn.append(np.zeros(fill, np.int32))
            off += fill
            splits.append(off)
    return np.concatenate(I), np.concatenate(D), np.concatenate(Cn), np.array(splits, np.int64)


def bucket_graph(sizes, k, seed):
    """front-packed random rows, neighbours inside the row's bucket only: 0..k stored, distances at eps, one float32 either
    side, well inside and far -> idx, dist, count (the stored length; on some rows 0 or k + 2), splits"""
    rng = np.random.default_rng(seed)
    splits = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(splits[-1])
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    count = np.zeros(n, np.int32)
    near = np.array([0.05, tc.EPS32, tc.EPS_DOWN, 0.01], f32)
    far = np.array([0.5, tc.EPS_UP, 0.11], f32)
    for b in range(len(sizes)):
        lo, hi = int(splits[b]), int(splits[b + 1])
        for i in range(lo, hi):
            a, z = max(lo, i - 6), min(hi, i + 7)             # neighbours among the rows close by: many small clusters
            pool = np.setdiff1d(np.arange(a, z), [i])
            c = min(len(pool), int(rng.integers(0, k + 1)), 4 if i % 3 else k)
            idx[i, :c] = rng.choice(pool, c, replace=False)
            dist[i, :c] = np.where(rng.random(c) < 0.3, rng.choice(near, c), rng.choice(far, c))
            count[i] = c
            if i % 11 == 0:
                count[i] = 0                                  # stored neighbours the count hides
            elif c == k and i % 2:
                count[i] = k + 2                              # a count above k
    return idx, dist, count, splits


def chain_graph(n, breaks=()):
    """row i names row i + 1 at 0.05 (one component of n rows: the depth that exposed the path-halving race, graph.hip);
    no edge leaves a row in `breaks`"""
    idx = np.full((n, 4), -1, np.int32)
    dist = np.full((n, 4), np.inf, f32)
    idx[:-1, 0] = np.arange(1, n)
    dist[:-1, 0] = 0.05
    for b in breaks:
        idx[b, 0], dist[b, 0] = -1, np.inf
    return idx, dist, np.full(n, 4, np.int32)


# ------------------------------------------------------------------------------------------- the four results
def reference(idx, dist, count, eps, mz, rt, tol, mode, rt_tol, order, refine):
    """tail_cases' rules on the graph cut at the counts -> labels, medoids, labels_sorted, n_clusters.  refine = False: one
    m/z for every row under WIDE, a10 only drops the clusters of one row (`chain_reference` does the same)"""
    ci, cd = tc.cut_at_count(idx, dist, count)
    db, _ = tc.dbscan_ref(ci, cd, eps)
    if refine:
        lab, n_cl = tc.refine_ref(db, mz, rt, tol, mode, rt_tol)
    else:
        lab = tc.drop_single_member_clusters(db)
        n_cl = int(lab.max()) + 1 if len(lab) else 0
    labels, medoids = tc.finalize_ref(lab, n_cl, order, ci, cd)
    return labels, medoids, lab, n_cl


def _same(out, ref, what):
    labels, medoids, lab_sorted, n_cl = out
    assert n_cl == ref[3], what
    assert np.array_equal(_np(lab_sorted), ref[2]), what
    assert np.array_equal(_np(labels), ref[0]), what
    assert np.array_equal(_np(medoids), ref[1]), what
    assert len(ref[1]) == ref[3] + int((np.asarray(ref[2]) < 0).sum()), what      # n_labels = clusters + noise rows


def check_all(ctx, limits, idx, dist, count, splits, eps, mz=None, rt=None, tol=None, mode=None, rt_tol=None, what=""):
    """tiled == counted == staged == reference; the tiled call must have run per tile exactly when no bucket exceeds the
    library's limit"""
    n, k = idx.shape
    refine = mz is not None
    if not refine:
        mz, tol, mode, rt_tol = np.full(n, 500.0, f32), tc.WIDE["tol"], tc.WIDE["mode"], tc.WIDE["rt_tol"]
    order = np.random.default_rng(n + 1).permutation(n).astype(np.int64)
    ref = reference(idx, dist, count, eps, mz, rt, tol, mode, rt_tol, order, refine)
    ti, td, tcn, tm, tr, to = (_dev(ctx, a) for a in (idx, dist, count, mz, rt, order))
    _same(ctx.cluster_graph(ti, td, eps, tm, tr, tol, mode, rt_tol, to, nb_count=tcn, splits=splits), ref, (what, "tiled"))
    assert ctx.counter(10) == int(np.diff(splits).max(initial=0) <= limits[1]), (what, "path")
    _same(ctx.cluster_graph(ti, td, eps, tm, tr, tol, mode, rt_tol, to, nb_count=tcn), ref, (what, "counted"))
    ci, cd = (_dev(ctx, a) for a in tc.cut_at_count(idx, dist, count))
    db, n_db = ctx.dbscan(ci, cd, eps)
    lab, n_cl = ctx.refine_clusters(db, n_db, tm, tr, tol, mode, rt_tol)
    labels, medoids = ctx.finalize(lab, n_cl, to, ci, cd)
    _same((labels, medoids, lab, n_cl), ref, (what, "staged"))


# ------------------------------------------------------------------------------------------- every chain graph, two forms
@pytest.mark.parametrize("name", tc.chain_names())
def test_chain_graph_as_one_bucket(ctx, limits, name):
    idx, dist, count, _, eps, _, _ = tc.chain_input(name)
    check_all(ctx, limits, idx, dist, count, np.array([0, len(idx)], np.int64), eps, what=name)


@pytest.mark.parametrize("name", tc.chain_names())
def test_chain_graph_replicated_into_buckets(ctx, limits, name):
    """copies as buckets with noise buckets of 3, 20 and 0 rows between them: small graphs share a tile, the numbering of
    clusters, members and kept clusters crosses tile borders (graphs beyond the limit: two copies, the per-row path)"""
    idx, dist, count, _, eps, _, _ = tc.chain_input(name)
    fillers = (3, 20, 0) if len(idx) <= limits[1] else (3, 0)
    I, D, Cn, splits = replicate(idx, dist, count, fillers)
    check_all(ctx, limits, I, D, Cn, splits, eps, what=name)


# ------------------------------------------------------------------------------------------- tile edges
def _edge_sizes(T):
    return {
        "bucket_T": [T],
        "bucket_T_plus_1": [T + 1],
        "sum_T": [T // 3, T // 3 + 1, T - 2 * (T // 3) - 1],
        "sum_T_then_more": [T // 3, T // 3 + 1, T - 2 * (T // 3) - 1, 1, T // 2 + 90, T // 2 - 100],
        "one_row_buckets": [1] * 70 + [9] + [1] * 1100,
        "first_last_single": [T, 10, 20, 33, T],
        "one_row": [1],
    }


@pytest.mark.parametrize("case", list(_edge_sizes(1024)))
def test_tile_edges(ctx, limits, case):
    sizes = _edge_sizes(limits[0])[case]
    idx, dist, count, splits = bucket_graph(sizes, 6, len(sizes) + sizes[0])
    check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what=case)


def test_empty_partition(ctx):
    import torch
    e = lambda dt, *s: torch.empty(s, dtype=dt, device=ctx.tdev)
    for splits in (np.zeros(1, np.int64), np.zeros(4, np.int64)):
        labels, medoids, lab, n_cl = ctx.cluster_graph(e(torch.int32, 0, 5), e(torch.float32, 0, 5), tc.EPS, e(torch.float32, 0),
                                                       None, 1.0, "Da", None, e(torch.int64, 0), nb_count=e(torch.int32, 0),
                                                       splits=splits)
        assert n_cl == 0 and len(labels) == 0 and len(medoids) == 0 and len(lab) == 0


@pytest.mark.parametrize("over", [0, 1])
def test_lds_limit(ctx, limits, over):
    """a bucket of max_tile_rows rows runs per tile, one row more sends the call down the per-row path (check_all asserts
    the counter); a small bucket behind it either way"""
    idx, dist, count, splits = bucket_graph([limits[1] + over, 40], 5, 8192 + over)
    check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what=("lds", over))


def test_union_find_depth(ctx, limits):
    idx, dist, count = chain_graph(3000)
    check_all(ctx, limits, idx, dist, count, np.array([0, 3000], np.int64), tc.EPS, what="chain")
    idx, dist, count = chain_graph(3000, breaks=(1499,))
    check_all(ctx, limits, idx, dist, count, np.array([0, 1500, 3000], np.int64), tc.EPS, what="chain, two buckets")


# ------------------------------------------------------------------------------------------- the rules inside one tile
def test_rules_share_a_tile(ctx, limits):
    """g_border (a border with several core in-neighbours, the one-member cluster, the self slot), g_eps (distances at eps and
    one float32 either side) and rows with nb_count 0 / above k as neighbouring buckets of ONE tile"""
    parts = [tc.graph_input("border"), tc.graph_input("eps"), bucket_graph([97], 5, 3)[:3], tc.graph_input("border")]
    k = 5
    I, D, Cn, splits, off = [], [], [], [0], 0
    for idx, dist, count in parts:
        n, kk = idx.shape
        pi, pd = np.full((n, k), -1, np.int32), np.full((n, k), np.inf, f32)
        pi[:, :kk], pd[:, :kk] = np.where(idx >= 0, idx + off, idx), dist
        I.append(pi)
        D.append(pd)
        Cn.append(np.full(n, kk, np.int32) if count is None else count)
        off += n
        splits.append(off)
    assert off <= limits[0]
    check_all(ctx, limits, np.concatenate(I), np.concatenate(D), np.concatenate(Cn), np.array(splits, np.int64), tc.EPS, what="rules")


@functools.lru_cache(maxsize=None)
def _refine_graph():
    """a graph whose DBSCAN clusters are the clusters of `tc.refine_input()` (every member names the cluster's next member,
    the last names the first, at 0.05 and 0.02 in turn), as ONE bucket; clusters of one row stay noise rows"""
    lab, mz, rt, _, _ = tc.refine_input()
    n, k = len(lab), 3
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    for c in np.unique(lab[lab >= 0]).tolist():
        rows = np.flatnonzero(lab == c)
        if len(rows) >= 2:
            idx[rows, 0] = np.roll(rows, -1)
            dist[rows, 0] = np.where(np.arange(len(rows)) % 2, f32(0.02), f32(0.05))
    return idx, dist, np.full(n, k, np.int32), mz, rt


@pytest.mark.parametrize("run", list(tc.R_RUNS))
def test_refinement_splits_inside_a_tile(ctx, limits, run):
    """a10 with m/z spread (Da, ppm) and with an RT tolerance on tail_cases' refinement patterns -- clusters that split,
    dissolve, collide and stay whole, up to 200 members, interleaved rows"""
    idx, dist, count, mz, rt = _refine_graph()
    n = len(idx)
    tol, mode, rt_tol = tc.R_RUNS[run]
    check_all(ctx, limits, idx, dist, count, np.array([0, n], np.int64), tc.EPS, mz, rt, tol, mode, rt_tol, what=run)
    # the same rows cut into buckets the tile kernels take (the edges across a cut go, so clusters split at it)
    pieces = -(-n // min(limits[1], 1500))
    splits = np.array([n * b // pieces for b in range(pieces + 1)], np.int64)
    assert np.diff(splits).max() <= limits[1]
    bucket = np.searchsorted(splits, np.arange(n), side="right") - 1
    across = (idx >= 0) & (bucket[np.where(idx >= 0, idx, 0)] != bucket[:, None])
    i2, d2 = np.where(across, -1, idx).astype(np.int32), np.where(across, np.inf, dist).astype(f32)
    check_all(ctx, limits, i2, d2, count, splits, tc.EPS, mz, rt, tol, mode, rt_tol, what=(run, "cut"))


def test_medoid_ties_across_tiles(ctx, limits):
    """tail_cases' cliques (every member of a cluster has the same score: the lowest row wins) and float_order (the float32
    slot-order sum decides) as buckets of three tiles"""
    for name in ("cliques", "float_order"):
        _, _, _, idx, dist = tc.medoid_input(name)
        I, D, Cn, splits = replicate(idx, dist, np.full(len(idx), idx.shape[1], np.int32), (0, 5, 0))
        check_all(ctx, limits, I, D, Cn, splits, tc.M_EPS, what=name)


# ------------------------------------------------------------------------------------------- contract breach
def test_id_outside_the_tile_fails_the_call(ctx, limits):
    from falcon_amd._lib import FalconHipError
    T = limits[0]
    idx, dist, count, splits = bucket_graph([T, T], 6, 12)
    bad = idx.copy()
    row = np.flatnonzero(count[:T] >= 1)[5]
    bad[row, 0] = T + 17                                        # a row of the other bucket, inside [0, n)
    order = np.arange(2 * T, dtype=np.int64)
    mz = np.full(2 * T, 500.0, f32)
    args = lambda i: (_dev(ctx, i), _dev(ctx, dist), tc.EPS, _dev(ctx, mz), None, 1.0, "Da", None, _dev(ctx, order))
    with pytest.raises(FalconHipError, match="code -1"):
        ctx.cluster_graph(*args(bad), nb_count=_dev(ctx, count), splits=splits)
    good = ctx.cluster_graph(*args(idx), nb_count=_dev(ctx, count), splits=splits)      # the context still works
    ref = ctx.cluster_graph(*args(idx), nb_count=_dev(ctx, count))
    for a, b in zip(good[:3], ref[:3]):
        assert np.array_equal(_np(a), _np(b))
    assert good[3] == ref[3] and ctx.counter(10) == 1


# ------------------------------------------------------------------------------------------- the pipeline
def test_pipeline_with_and_without_tiles(monkeypatch):
    from falcon_amd import synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    d = synth.select_charge(synth.generate(28000, seed=7), 2)
    ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    out = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("FALCON_GRAPH_TILED", switch)
        pipe = ClusterPipeline(device=0)
        labels, medoids = pipe.run(ds, 20.0, "ppm", None, 0.05, 2 ** 15, AnnParams())
        out[switch] = (_np(labels), _np(medoids), pipe.ctx.counter(10))
    assert out["0"][2] == 0 and out["1"][2] == 1
    assert np.array_equal(out["0"][0], out["1"][0]) and np.array_equal(out["0"][1], out["1"][1])
    assert len(out["1"][1]) < len(out["1"][0])                  # (something clustered)
