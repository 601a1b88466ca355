"""`fal_cluster_graph_tiled` -- the graph tail per bucket tile (tile_dbscan / tile_members / tile_medoid kernels, DESIGN
section 3) -- against `fal_cluster_graph_counted`, the three staged calls and the plain references of tests/tail_cases.py.
Every case expects all four equal in labels, medoids, sorted labels and both counts (`np.array_equal` on integers), and
names the path that has to have run (`fal_ctx_counter(10)`) and the number of tiles whose eps-edges overflowed the edge list
of tile_dbscan_kernel and took its second pass (`fal_ctx_counter(11)`), counted from the input's own eps-edges.  The tile limits
and the list's capacity come from the library (`fal_graph_tile_limits`, `fal_graph_tile_capacity`)."""
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


def overflowing(ctx, limits, idx, dist, count, splits, eps):
    """-> per tile: whether its eps-edges (tail_cases.tile_eps_edges) exceed the capacity the library states for a tile of
    its rows in a call with this largest tile; no tile when a bucket sends the call down the per-row path"""
    sizes = np.diff(splits)
    if len(idx) == 0 or sizes.max() > limits[1]:
        return np.zeros(0, bool)
    tiles = tc.tile_table(sizes.tolist(), limits[0])
    rows = np.diff(tiles)
    cap = np.array([ctx.graph_tile_capacity(int(rows.max()), int(m))[1] for m in rows], np.int64)
    return tc.tile_eps_edges(idx, dist, count, tiles, eps) > cap


def check_all(ctx, limits, idx, dist, count, splits, eps, mz=None, rt=None, tol=None, mode=None, rt_tol=None, what="",
              ref_idx=None):
    """tiled == counted == staged == reference; the tiled call must have run per tile exactly when no bucket exceeds the
    library's limit, and as many tiles must have taken the second pass as have more eps-edges than their list holds.
    ref_idx: the ids the reference sees where `idx` holds ids outside [0, n) (they stand for empty slots).
    -> the per-tile overflow flags"""
    n, k = idx.shape
    refine = mz is not None
    if not refine:
        mz, tol, mode, rt_tol = np.full(n, 500.0, f32), tc.WIDE["tol"], tc.WIDE["mode"], tc.WIDE["rt_tol"]
    order = np.random.default_rng(n + 1).permutation(n).astype(np.int64)
    ref = reference(idx if ref_idx is None else ref_idx, dist, count, eps, mz, rt, tol, mode, rt_tol, order, refine)
    over = overflowing(ctx, limits, idx, dist, count, splits, eps)
    ti, td, tcn, tm, tr, to = (_dev(ctx, a) for a in (idx, dist, count, mz, rt, order))
    _same(ctx.cluster_graph(ti, td, eps, tm, tr, tol, mode, rt_tol, to, nb_count=tcn, splits=splits), ref, (what, "tiled"))
    assert ctx.counter(10) == int(np.diff(splits).max(initial=0) <= limits[1]), (what, "path")
    assert ctx.counter(11) == int(over.sum()), (what, "tiles on the second pass", over)
    _same(ctx.cluster_graph(ti, td, eps, tm, tr, tol, mode, rt_tol, to, nb_count=tcn), ref, (what, "counted"))
    ci, cd = (_dev(ctx, a) for a in tc.cut_at_count(idx, dist, count))
    db, n_db = ctx.dbscan(ci, cd, eps)
    lab, n_cl = ctx.refine_clusters(db, n_db, tm, tr, tol, mode, rt_tol)
    labels, medoids = ctx.finalize(lab, n_cl, to, ci, cd)
    _same((labels, medoids, lab, n_cl), ref, (what, "staged"))
    return over


# ------------------------------------------------------------------------------------------- every chain graph, two forms
@pytest.mark.parametrize("name", tc.chain_names())
def test_chain_graph_as_one_bucket(ctx, limits, name):
    idx, dist, count, _, eps, _, _ = tc.chain_input(name)
    over = check_all(ctx, limits, idx, dist, count, np.array([0, len(idx)], np.int64), eps, what=name)
    if name == "M:big":                                         # 5,000 rows of eight eps-edges: twice what the list holds
        assert over.tolist() == [True]


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
    assert not check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what=case).any()      # sparse: every tile on the list


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
    second = check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what=("lds", over))
    assert second.tolist() == ([] if over else [False, False])  # (about 5,300 eps-edges in the large tile: the list holds them)


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


# ------------------------------------------------------------------------------------------- the edge-list cut
def _one(n):
    return np.array([0, n], np.int64)


def _both_kinds_of_edge(idx, dist, count):
    """(core -> core edges, core -> border edges) of a one-bucket graph at EPS"""
    edge = (np.arange(idx.shape[1])[None, :] < count[:, None]) & (idx >= 0) & (dist <= tc.EPS32)
    core = edge.any(1)
    to_core = core[np.where(edge, idx, 0)]
    return int((edge & to_core).sum()), int((edge & ~to_core).sum())


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("rows", [64, 8192])
def test_edge_list_cut(ctx, limits, rows, delta):
    """one bucket alone in the call with cap - 1, cap and cap + 1 eps-edges (cap from the library: 4 a row at 64 rows, 6,144
    at 8,192): the list until it is full, the second pass from one edge more; unions and border votes on either side.  At
    8,192 rows three rows in four are noise, the others lie anywhere in the tile (rows 0 and 8,191 are core)"""
    assert rows <= limits[1]
    cap = ctx.graph_tile_capacity(rows, rows)[1]
    assert 0 < cap <= 4 * rows
    n_core = cap // 4 if rows > 64 else 48                      # (64 rows: 48 rows of 5 or 6 edges, 16 borders, no noise)
    idx, dist, count = tc.cut_graph(rows, 8, n_core, rows // 4 if rows == 64 else n_core // 3, cap + delta, rows + delta)
    assert tc.tile_eps_edges(idx, dist, count, [0, rows], tc.EPS).tolist() == [cap + delta]
    assert min(_both_kinds_of_edge(idx, dist, count)) >= 32
    over = check_all(ctx, limits, idx, dist, count, _one(rows), tc.EPS, what=(rows, delta))
    assert over.tolist() == [delta > 0]


# ------------------------------------------------------------------------------------------- density
DENSITIES = (0, 1, 3.9, 4.1, 8, 16)


def _sweep_cases(T):
    """(name, bucket sizes, eps-edges per row).  [T // 2, 40, T, 7] makes tiles of T // 2 + 40, T and 7 rows; the last
    cannot overflow whatever it stores (7 rows of k slots against a list of thousands), so the call in which EVERY tile
    overflows has buckets of its own: tiles of T, T // 2 and T rows with every slot an eps-edge"""
    return [(f"d{d}", [T // 2, 40, T, 7], d) for d in DENSITIES] + [("full", [T, T // 2, T], 16)]


@functools.lru_cache(maxsize=None)
def _sweep_graph(T, name):
    _, sizes, d = next(c for c in _sweep_cases(T) if c[0] == name)
    return tc.density_graph(sizes, 16, d, 1000 + 10 * DENSITIES.index(d) + len(sizes))


@pytest.mark.parametrize("name", [c[0] for c in _sweep_cases(1024)])
def test_density_sweep(ctx, limits, name):
    idx, dist, count, splits = _sweep_graph(limits[0], name)
    check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what=name)


def test_density_sweep_reaches_both_branches(ctx, limits):
    """the sweep holds a call without an overflowing tile, one with some and one with all: a capacity that moves must not
    empty a class unnoticed"""
    seen = set()
    for name, _, _ in _sweep_cases(limits[0]):
        idx, dist, count, splits = _sweep_graph(limits[0], name)
        over = overflowing(ctx, limits, idx, dist, count, splits, tc.EPS)
        assert len(over) == 3
        seen.add("none" if not over.any() else "all" if over.all() else "some")
    assert seen == {"none", "some", "all"}


@pytest.mark.parametrize("large_first", [True, False])
def test_list_and_second_pass_in_one_launch(ctx, limits, large_first):
    """a 5,000-row bucket of 4.5 eps-edges a row is the call's largest tile and overflows the list it sizes; the 100-row
    bucket beside it, every one of its 40 slots an eps-edge, keeps its 4,000 edges on the list only because it has the rest of
    that block (alone in a call it would have 400)"""
    k = 40
    assert 5000 <= limits[1]
    big = tc.density_graph([5000], k, 4.5, 45, hide=False)
    small = tc.density_graph([100], k, 40, 46, hide=False)
    assert tc.tile_eps_edges(*small[:3], [0, 100], tc.EPS).tolist() == [4000]
    assert ctx.graph_tile_capacity(100, 100)[1] < 4000 <= ctx.graph_tile_capacity(5000, 100)[1]
    parts = [big, small] if large_first else [small, big]
    off = len(parts[0][0])
    idx = np.concatenate([parts[0][0], np.where(parts[1][0] >= 0, parts[1][0] + off, -1).astype(np.int32)])
    dist, count = np.concatenate([parts[0][1], parts[1][1]]), np.concatenate([parts[0][2], parts[1][2]])
    splits = np.array([0, off, len(idx)], np.int64)
    over = check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what=("mixed", large_first))
    assert over.tolist() == ([True, False] if large_first else [False, True])


# ------------------------------------------------------------------------------------------- both 16-bit fields at their top
def _long_range(L, filled):
    """rows 0 and L - 1 name each other; row L - 2 stores nothing within eps and is named by rows 3 and L // 2 + 4 only (it
    joins row 3's cluster, the lower core; row L // 2 + 4 keeps a border of its own, row L // 2 + 5); all else noise, or
    (filled) rows 8 .. L - 9 in pairs (r, r + 1) that name each other: an eps-edge a row, more than the widest tile's list holds"""
    idx = np.full((L, 4), -1, np.int32)
    dist = np.full((L, 4), np.inf, f32)
    h = L // 2 + 4
    for i, nb in {0: [(L - 1, 0.05)], L - 1: [(7, 0.5), (0, tc.EPS32)], 3: [(L - 2, 0.05)], h: [(h + 1, 0.02), (L - 2, 0.01)],
                  L - 2: [(3, tc.EPS_UP), (h, 0.5)]}.items():
        for s, (j, d) in enumerate(nb):
            idx[i, s], dist[i, s] = j, f32(d)
    if filled:
        r = np.setdiff1d(np.arange(8, L - 8, 2), [h])
        idx[r, 2], dist[r, 2] = r + 1, f32(0.05)
        idx[r + 1, 0], dist[r + 1, 0] = r, f32(0.05)
    return idx, dist, np.full(L, 4, np.int32)


def _pairs(L, doubled):
    """L / 2 clusters of two rows, (i, i + L / 2): row i names its partner, the partner stores a far row.  doubled: twice the
    eps-edges on the same pairs -- even i name the partner in two slots (the same id twice, 0.55 each: at eps 0.6 the score
    0.55 + 0.55 + (2 - 1 - 2) stays positive), odd i are named back by their partner"""
    half = L // 2
    i = np.arange(half)
    idx = np.full((L, 4), -1, np.int32)
    dist = np.full((L, 4), np.inf, f32)
    idx[i, 1], dist[i, 1] = i + half, f32(0.55)
    idx[i + half, 0], dist[i + half, 0] = (i + 1) % half, f32(0.9)
    if doubled:
        ev, od = i[::2], i[1::2]
        idx[ev, 3], dist[ev, 3] = ev + half, f32(0.55)
        idx[od + half, 2], dist[od + half, 2] = od, f32(0.25)
    return idx, dist, np.full(L, 4, np.int32)


@pytest.mark.parametrize("case", ["long_range", "long_range_filled", "pairs", "pairs_doubled"])
def test_widest_tile_rows_and_labels(ctx, limits, case):
    """a bucket of max_tile_rows rows: eps-edges between its first and last row and to a border thousands of rows from its
    cores (source and target fields of the packed edge at their top), and the most clusters a tile can have, half its rows
    (tile label and tile row of the member key at their top) -- on the list, and with twice the edges on the second pass"""
    L = limits[1]
    assert L % 2 == 0 and L <= 65536
    cap = ctx.graph_tile_capacity(L, L)[1]
    if case.startswith("long_range"):
        idx, dist, count = _long_range(L, case.endswith("filled"))
        over = check_all(ctx, limits, idx, dist, count, _one(L), tc.EPS, what=case)
        assert over.tolist() == [case.endswith("filled")]
        return
    idx, dist, count = _pairs(L, case == "pairs_doubled")
    ne = int(tc.tile_eps_edges(idx, dist, count, [0, L], tc.M_EPS)[0])
    assert ne == (L if case == "pairs_doubled" else L // 2)
    over = check_all(ctx, limits, idx, dist, count, _one(L), tc.M_EPS, what=case)
    assert over.tolist() == [ne > cap]
    if case == "pairs_doubled":
        assert ne > cap                                         # (the variant exists for the second pass)


# ------------------------------------------------------------------------------------------- ids that are no neighbours
@functools.lru_cache(maxsize=None)
def _three_tiles(T):
    """tiles of T rows: sparse, dense enough for the second pass, sparse"""
    return tc.density_graph([T, T, T], 8, [1, 6, 1], 31)


def test_ids_outside_the_dataset_are_empty_slots(ctx, limits):
    """ids >= n, n - 1 + 2^20, -7 and INT32_MIN in slots below the count, at distance 0.05, in a tile on the list and in one
    on the second pass: no error, the slots count as empty (`test_dbscan_ignores_neighbour_ids_outside_the_dataset`: staged)"""
    T = limits[0]
    idx, dist, count, splits = (a.copy() for a in _three_tiles(T))
    idx, dist, count, splits = idx[:2 * T], dist[:2 * T], count[:2 * T], splits[:3]
    n, k = idx.shape
    junk = [n, n + 5, n - 1 + 2 ** 20, -7, np.iinfo(np.int32).min, 2 ** 31 - 1]
    rows = np.flatnonzero((count >= 1) & (np.arange(n) % 3 == 0))
    for q, i in enumerate(rows.tolist()):
        s = (q // len(junk)) % min(int(count[i]), k)
        idx[i, s], dist[i, s] = junk[q % len(junk)], f32(0.05)
    assert all((idx[:T] == v).any() and (idx[T:] == v).any() for v in junk)
    clean = np.where((idx < -1) | (idx >= n), -1, idx).astype(np.int32)
    over = check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what="junk ids", ref_idx=clean)
    assert over.tolist() == [False, True]


# ------------------------------------------------------------------------------------------- contract breach
def _plant(T, tile, hidden):
    """`_three_tiles` with one id of another tile, at 0.05, in a row of `tile`: in the first slot BEHIND the row's count
    (hidden) or in its slot 0"""
    idx, dist, count, splits = (a.copy() for a in _three_tiles(T))
    inside = np.arange(tile * T, (tile + 1) * T)
    row = inside[np.flatnonzero((count[inside] >= 1) & (count[inside] < idx.shape[1]))[7]]
    s = int(count[row]) if hidden else 0
    idx[row, s], dist[row, s] = ((tile + 1) % 3) * T + 17, f32(0.05)
    return idx, dist, count, splits


@pytest.mark.parametrize("tile", [0, 1, 2])
def test_id_outside_the_tile_behind_the_count_is_not_read(ctx, limits, tile):
    idx, dist, count, splits = _plant(limits[0], tile, True)
    over = check_all(ctx, limits, idx, dist, count, splits, tc.EPS, what=("hidden", tile))
    assert over.tolist() == [False, True, False]


@pytest.mark.parametrize("tile", [1, 2])
def test_id_outside_a_later_or_an_overflowing_tile_fails_the_call(ctx, limits, tile):
    """the breach in the last tile (on the list) and in the tile on the second pass"""
    from falcon_amd._lib import FalconHipError
    T = limits[0]
    bad, dist, count, splits = _plant(T, tile, False)
    idx = _three_tiles(T)[0]
    order = np.arange(3 * T, dtype=np.int64)
    mz = np.full(3 * T, 500.0, f32)
    args = lambda i: (_dev(ctx, i), _dev(ctx, dist), tc.EPS, _dev(ctx, mz), None, 1.0, "Da", None, _dev(ctx, order))
    assert overflowing(ctx, limits, bad, dist, count, splits, tc.EPS).tolist() == [False, True, False]
    with pytest.raises(FalconHipError, match="code -1"):
        ctx.cluster_graph(*args(bad), nb_count=_dev(ctx, count), splits=splits)
    good = ctx.cluster_graph(*args(idx), nb_count=_dev(ctx, count), splits=splits)      # the context still works
    assert ctx.counter(10) == 1 and ctx.counter(11) == 1
    ref = ctx.cluster_graph(*args(idx), nb_count=_dev(ctx, count))
    for a, b in zip(good[:3], ref[:3]):
        assert np.array_equal(_np(a), _np(b))
    assert good[3] == ref[3]


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
