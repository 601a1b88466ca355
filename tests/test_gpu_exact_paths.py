"""Exact mode on the GPU, the paths test_gpu_exact.py's generator (30-40 peaks a spectrum, components of at most six peaks,
half a million edges) never enters:

  staging matrix   `exact_edges_kernel` keeps a 64-row tile side in LDS only when its rows hold <= 3,200 peaks, else reads the
                   peaks from global memory; the two sides decide independently.  Every combination, the boundary included.
  growth           more stored edges than one buffer of 2^25 holds: `exact_edges_dev` moves them to a larger block.
  solver sizes     the Hungarian solver of peakmatch.h as the device compiles it: every component size 2..32 on both sides,
                   both orientations, tie-heavy inputs, exactly 32 (solved) and 33 (refused) through every consumer.
  edges            empty buckets, buckets of 1 / 2 / 63 / 64 / 65 / 128 / 129 rows, d == t, fragment_tol = 0, a peak
                   difference equal to the tolerance, n = 0 / 1, spectra without peaks.

Expected values come from the pieces test_gpu_exact.py uses (its helpers are imported, not copied): `fo.cosine_fast` per pair,
scipy's linkage / fcluster, `fo.postprocess_cluster`, float32 medoid sums in ascending member order -- never from the library.
Which path an input takes is computed here from the input and asserted."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import linkage_cases as lc
from tests import peakmatch_cases as pc
from tests import test_gpu_exact as base
from tests.test_gpu_exact import _block_matrix, _expected_csr, _gpu_clusters, _peaks, _restate, _scipy_labels, _sorted, _to_np

pytestmark = pytest.mark.gpu

LDS_PEAKS = 3200             # csrc/exwalk.h kExLdsPeaks
TILE = 64                    # kExTile
EDGE_BUDGET = 2 ** 25        # kExEdgeBudget


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _normalise(x):
    x = np.asarray(x, np.float32)
    nrm = np.sqrt(np.sum(x.astype(np.float64) ** 2)).astype(np.float32)
    return x / nrm if nrm > 0 else x


# ---------------------------------------------------------------------------------------------------------- 1. staging
def _template_rows(rng, counts, n_templates=4, chained_templates=1, jitter=0.002):
    """one bucket in sorted-row order: row r holds exactly counts[r] peaks -- the counts[r] most intense peaks of one of the
    bucket's templates (jittered m/z, intensities x 1 +- 0.3), so rows of different sizes still resemble each other.  The
    first `chained_templates` templates carry six intense peaks 0.03 apart (components of several peaks at tolerance 0.05:
    the fallback list).  A count above 1,000 is the template's 40 top peaks + weak uniform peaks.
    -> (mz list, intensity list, template of every row, -1 for rows of 0 / 1 peaks)"""
    size = int(1.1 * max(c for c in counts if c <= 1000)) + 8
    temps = []
    for ti in range(n_templates):
        m = rng.uniform(150, 1400, size)
        it = rng.uniform(0.1, 1.0, size)
        if ti < chained_templates:
            m[:6] = rng.uniform(300, 900) + 0.03 * np.arange(6)
            it[:6] = rng.uniform(1.5, 2.0, 6)
        o = np.argsort(-it)
        temps.append((m[o], it[o]))
    mz, it, tpl = [], [], []
    for c in counts:
        ti = int(rng.integers(n_templates))
        tm, tit = temps[ti]
        if c > 1000:
            m = np.concatenate([tm[:40] + rng.normal(0, jitter, 40), rng.uniform(150, 1400, c - 40)])
            i = np.concatenate([tit[:40] * rng.uniform(0.7, 1.3, 40), rng.uniform(0.01, 0.05, c - 40)])
        else:
            m = tm[:c] + rng.normal(0, jitter, c)
            i = tit[:c] * rng.uniform(0.7, 1.3, c)
        o = np.argsort(m)
        mz.append(m[o].astype(np.float32))
        it.append(_normalise(i[o]))
        tpl.append(ti if c >= 8 else -1)
    return mz, it, tpl


def _assemble(buckets, centres, seed):
    """buckets of sorted rows -> a dataset in shuffled row order whose precursor sort restores the buckets' row order"""
    rng = np.random.default_rng(seed)
    mz = [m for b in buckets for m in b[0]]
    it = [i for b in buckets for i in b[1]]
    pmz = np.concatenate([c + 1e-4 * np.arange(len(b[0])) for b, c in zip(buckets, centres)]).astype(np.float32)
    perm = rng.permutation(len(mz))
    mz, it, pmz = [mz[i] for i in perm], [it[i] for i in perm], pmz[perm]
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in mz])]).astype(np.int64)
    return dict(mz=np.concatenate(mz).astype(np.float32), intensity=np.concatenate(it).astype(np.float32), indptr=indptr,
                precursor_mz=pmz, retention_time=rng.uniform(0, 100, len(pmz)).astype(np.float32))


def _tile_kinds(counts_sorted, splits):
    """the kernel's tiles restated from the input: {(A side in LDS, B side in LDS, diagonal, partial B side)} and per tile
    (a0, b0, fits_a, fits_b)"""
    kinds, tiles = set(), []
    for s0, s1 in zip(splits[:-1], splits[1:]):
        for a0 in range(s0, s1, TILE):
            for b0 in range(a0, s1, TILE):
                ta = int(counts_sorted[a0:min(a0 + TILE, s1)].sum())
                tb = int(counts_sorted[b0:min(b0 + TILE, s1)].sum())
                fa, fb = ta <= LDS_PEAKS, tb <= LDS_PEAKS
                kinds.add((fa, fb, a0 == b0, s1 - b0 < TILE))
                tiles.append((a0, b0, fa, fb))
    return kinds, tiles


STAGE_TOL, STAGE_MM, STAGE_T = 0.05, 3, 0.6


@pytest.fixture(scope="module")
def staging():
    rng = np.random.default_rng(41)
    a = [0, 1, 149] + [50] * 61                 # 3,200 exactly: 64 rows x the default max_peaks_used
    b = [0, 1, 150] + [50] * 61                 # 3,201
    small = [0, 1] + [36] * 62
    big = [0, 1] + [60] * 62                    # 3,721
    part = [0, 1] + [165] * 20                  # a last, partial tile that does not fit: 22 rows, 3,301 peaks
    giant = [36] * 30 + [3300] + [36] * 31 + [0, 1]     # one row above 3,200 by itself
    counts = [a + b + small, big + small + part, small + giant + [36, 36]]
    shuffled = []
    for c in counts:                                         # shuffled inside every tile: the tiles keep their rows
        c = np.asarray(c)
        for x in range(0, len(c), TILE):
            seg = c[x:x + TILE].copy()
            rng.shuffle(seg)
            c[x:x + TILE] = seg
        shuffled.append(c.tolist())
    buckets = [_template_rows(rng, c) for c in shuffled]
    d = _assemble(buckets, [400.0, 450.0, 500.0], seed=42)
    order, mzs, splits = _sorted(d, 20.0, "ppm")
    assert list(splits) == [0, 192, 342, 472]
    counts_sorted = np.diff(d["indptr"])[order]
    assert list(counts_sorted) == [x for c in shuffled for x in c]
    mats = [_block_matrix(d, order, s0, s1, STAGE_TOL, STAGE_MM) for s0, s1 in zip(splits[:-1], splits[1:])]
    tpl = np.array([t for b in buckets for t in b[2]])
    return dict(d=d, order=order, splits=splits, counts=counts_sorted, mats=mats, tpl=tpl)


def test_staging_matrix_covers_every_case(staging):
    """the inputs reach every (A in LDS, B in LDS, diagonal) case, the boundary and the odd rows -- computed from the input"""
    counts, splits = staging["counts"], staging["splits"]
    kinds, tiles = _tile_kinds(counts, splits)
    have = {k[:3] for k in kinds}
    assert have == {(True, True, True), (False, False, True), (True, True, False), (True, False, False), (False, True, False),
                    (False, False, False)}
    assert (True, False, False, True) in kinds or (False, False, False, True) in kinds      # a partial last tile not in LDS
    sides = {}
    for s0, s1 in zip(splits[:-1], splits[1:]):
        for a0 in range(s0, s1, TILE):
            sides[a0] = counts[a0:min(a0 + TILE, s1)]
    totals = sorted(int(c.sum()) for c in sides.values())
    assert LDS_PEAKS in totals and LDS_PEAKS + 1 in totals
    assert any(len(c) < TILE and c.sum() > LDS_PEAKS for c in sides.values())
    assert counts.max() > LDS_PEAKS
    for fits in (True, False):                                # rows of 0 peaks and 1 peak inside each kind of tile side
        cs = [c for c in sides.values() if (c.sum() <= LDS_PEAKS) == fits]
        assert any(0 in c for c in cs) and any(1 in c for c in cs)
    # pairs of the fallback list (a component of two or more query peaks) inside tiles that read global memory
    d, order, tpl = staging["d"], staging["order"], staging["tpl"]
    n_fall = 0
    for a0, b0, fa, fb in tiles:
        if fa and fb:
            continue
        s1 = splits[np.searchsorted(splits, a0, side="right")]
        for i in range(a0, min(a0 + TILE, s1)):
            for j in range(b0, min(b0 + TILE, s1)):
                if j > i and tpl[i] == 0 and tpl[j] == 0:
                    comps = pc.components(_peaks(d, order[i])[0], _peaks(d, order[j])[0], STAGE_TOL)
                    n_fall += any(nr > 1 for nr, _ in comps)
    assert n_fall > 50


def test_staging_edges_equal_brute_force(ctx, staging):
    d, order, splits, mats = (staging[k] for k in ("d", "order", "splits", "mats"))
    n = len(order)
    ptr, idx, dist = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, STAGE_TOL, STAGE_MM, STAGE_T))
    eptr, eidx, edist = _expected_csr(mats, splits, n, STAGE_T)
    assert len(eidx) > 5000
    # edges exist in every tile with a side in global memory (a wrong operand there cannot hide behind distances of 1)
    _, tiles = _tile_kinds(staging["counts"], splits)
    erow = np.repeat(np.arange(n), np.diff(eptr))
    for a0, b0, fa, fb in tiles:
        if fa and fb:
            continue
        sel = (erow >= a0) & (erow < a0 + TILE) & (eidx >= b0) & (eidx < b0 + TILE)
        assert sel.sum() > 0, (a0, b0, fa, fb)
    assert np.array_equal(ptr, eptr)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(dist, edist), int((dist != edist).sum())


@pytest.mark.parametrize("method", ["average", "complete"])
def test_staging_generate_clusters_equals_the_restatement(staging, method, monkeypatch):
    from falcon_amd.cluster.cluster import AnnParams, SpectrumDataset, generate_clusters
    d, splits, mats = staging["d"], staging["splits"], staging["mats"]
    cache = {(int(s0), int(s1)): D for s0, s1, D in zip(splits[:-1], splits[1:], mats)}

    def cached(d_, order_, s0, s1, tol, mm):                 # the same brute force, computed once by the fixture
        assert d_ is d and (tol, mm) == (STAGE_TOL, STAGE_MM) and np.array_equal(order_, staging["order"])
        return cache[(int(s0), int(s1))]
    monkeypatch.setattr(base, "_block_matrix", cached)
    ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    labels, medoids = generate_clusters(ds, method, STAGE_T, STAGE_MM, 20.0, "ppm", None, STAGE_TOL, 2 ** 15,
                                        ann=AnnParams(eps=STAGE_T, exact=True, mz_interval=0))
    exp = _restate(d, 20.0, "ppm", None, STAGE_TOL, STAGE_T, method, STAGE_MM)
    assert len(exp) >= 6
    assert _gpu_clusters(labels, medoids) == exp


def test_main_exact_with_100_peaks_a_spectrum(tmp_path):
    """--max_peaks_used 100 is the command line's way past 3,200 peaks a tile side (complete linkage: the clusters come from
    the stored edge distances themselves; average linkage would score every member pair again in the fill.  The threshold
    sits at the median distance of spectra of one template: a wrong distance moves the partition)"""
    from falcon_amd.falcon import main
    from falcon_amd.ms_io import ms_io
    d = base._spectra(3, 140, [520.0], seed=47, jitter=0.004, n_peaks=100, drop=0.3)
    specs = []
    for i in range(len(d["precursor_mz"])):
        m, it = _peaks(d, i)
        specs.append({"identifier": f"scan={i}", "precursor_mz": float(d["precursor_mz"][i]), "precursor_charge": 2,
                      "retention_time": float(d["retention_time"][i]), "mz": m.astype(np.float64), "intensity": it})
    mgf = str(tmp_path / "in.mgf")
    ms_io.write_spectra(mgf, specs)
    out, work = str(tmp_path / "res"), tmp_path / "work"
    assert main([mgf, out, "--exact", "--linkage", "complete", "--eps", "0.43", "--min_matched_peaks", "2", "--max_peaks_used", "100",
                 "--work_dir", str(work), "--mz_interval", "0"]) == 0
    lines = open(out + ".csv").read().splitlines()
    body = [l.split(",") for l in lines if not l.startswith("#")][1:]
    table = {r[1]: int(r[5]) for r in body}
    z = np.load(work / "spectra" / "spectra_charge_2.npz")
    part = {k: z[k] for k in z.files}
    order, mzs, splits = _sorted(part, 20.0, "ppm")
    counts = np.diff(part["indptr"])[order]
    assert counts.min() > 50                                  # the spectra kept more than the default 50 peaks
    kinds, _ = _tile_kinds(counts, splits)
    assert {k[:3] for k in kinds} >= {(False, False, True), (False, False, False)}
    names = [str(x) for x in part["identifier"]]
    exp = _restate(part, 20.0, "ppm", None, 0.05, 0.43, "complete", 2)
    assert len(exp) >= 20 and max(map(len, exp)) < 20         # many small clusters, far from one per template
    lab = np.array([table[nm] for nm in names])
    groups = {}
    for r, l in enumerate(lab):
        groups.setdefault(l, []).append(r)
    assert {frozenset(v) for v in groups.values() if len(v) >= 2} == set(exp)


# ---------------------------------------------------------------------------------------------------------- 2. growth
GROW_N, GROW_K, GROW_T = 8400, 8, 0.3


@pytest.fixture(scope="module")
def growth():
    """8,400 rows, exact copies of 8 templates: every one of the 35.3 M pairs is an edge"""
    rng = np.random.default_rng(53)
    n, K = GROW_N, GROW_K
    assert n * (n - 1) // 2 > EDGE_BUDGET
    t_mz = np.sort(rng.uniform(150, 1400, 40)).astype(np.float32)
    base_it = rng.uniform(0.1, 1.0, 40)
    t_it = [_normalise(base_it * rng.uniform(0.95, 1.05, 40)) for _ in range(K)]
    Dk = np.zeros((K, K))
    for a in range(K):
        for b in range(K):                                   # a = the query (the lower sorted row), the diagonal included
            sim, _ = fo.cosine_fast(t_mz, t_it[a], t_mz, t_it[b], 0.05)
            Dk[a, b] = 1.0 - sim
    assert (Dk <= GROW_T).all() and len(np.unique(Dk)) > K
    tpl = rng.integers(K, size=n)
    d = dict(mz=np.tile(t_mz, n), intensity=np.concatenate([t_it[k] for k in tpl]).astype(np.float32),
             indptr=(40 * np.arange(n + 1)).astype(np.int64),
             precursor_mz=(700.0 + 2.0 ** -14 * rng.permutation(n)).astype(np.float32),     # distinct float32 values
             retention_time=rng.uniform(0, 100, n).astype(np.float32))
    assert len(np.unique(d["precursor_mz"])) == n
    order, mzs, splits = _sorted(d, 1.0, "Da")
    assert list(splits) == [0, n]
    return dict(d=d, order=order, splits=splits, tpl=tpl[order], Dk=Dk)


def _grown_rows(tpl, Dk, r0, r1):
    """expected CSR rows r0..r1 of the all-edges bucket: columns = every other row ascending, distance by (lower, higher)"""
    n = len(tpl)
    i = np.arange(r0, r1)[:, None]
    j = np.arange(n - 1)[None, :]
    j = j + (j >= i)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return j.astype(np.int32), Dk[tpl[lo], tpl[hi]]


def test_growth_of_the_edge_buffers(ctx, growth):
    """The stored edges pass the 2^25 the first block holds before the last tiles: the grow branch of `exact_edges_dev` moves
    them to a larger block (about 2 GB of keys / values + the retired 1 GB block, 1.1 GB of sorted copies, 0.85 GB of CSR
    outputs on the device; 0.85 GB on the host).  Run twice: the retired block is freed by the second call."""
    import torch
    d, order, splits, tpl, Dk = (growth[k] for k in ("d", "order", "splits", "tpl", "Dk"))
    n = GROW_N
    first = ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, 0.05, 0, GROW_T)
    ptr, idx, dist = _to_np(*first)
    assert ptr[-1] == n * (n - 1) == len(idx) == len(dist)
    assert np.array_equal(ptr, (n - 1) * np.arange(n + 1))
    idx, dist = idx.reshape(n, n - 1), dist.reshape(n, n - 1)
    for r0 in range(0, n, 400):
        eidx, edist = _grown_rows(tpl, Dk, r0, min(r0 + 400, n))
        assert np.array_equal(idx[r0:r0 + 400], eidx), r0
        assert np.array_equal(dist[r0:r0 + 400], edist), r0
    del idx, dist
    again = ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, 0.05, 0, GROW_T)
    assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_growth_single_linkage_cluster_and_medoid(growth):
    """the fused pass on the grown buffers (`exact_csr_dev` sizes its arrays by the grown capacity): one cluster; the medoid
    = argmin of the float32 running sums over the other members in ascending row order, ties to the lowest row"""
    from falcon_amd.cluster.cluster import AnnParams, SpectrumDataset, generate_clusters
    d, order, tpl, Dk = (growth[k] for k in ("d", "order", "tpl", "Dk"))
    n = GROW_N
    ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    labels, medoids = generate_clusters(ds, "single", GROW_T, 0, 1.0, "Da", None, 0.05, 2 ** 15,
                                        ann=AnnParams(eps=GROW_T, exact=True, mz_interval=0))
    assert len(medoids) == 1 and bool((np.asarray(labels) == 0).all())
    score = np.zeros(n, np.float32)
    for r0 in range(0, n, 400):
        _, dd = _grown_rows(tpl, Dk, r0, min(r0 + 400, n))
        score[r0:r0 + 400] = np.cumsum(dd.astype(np.float32), axis=1, dtype=np.float32)[:, -1]
    assert int(np.asarray(medoids)[0]) == int(order[int(np.argmin(score))])


# ---------------------------------------------------------------------------------------------------------- 3 / 4. solver
def _kept(pairs):
    """the pairs the library takes (no component above 32 -- by the test's own window walk) and what they cover"""
    cov = pc.Coverage()
    keep = [p for p in pairs if cov.add(pc.components(p[0], p[2], p[4]))]
    return keep, cov


def _check_pairs_on_the_device(ctx, pairs, min_matches_list):
    """every pair as its own 2-row bucket through `exact_edges` (float64 `==`) and as a neighbour slot through
    `rescore_neighbors` (float32 bit patterns)"""
    import torch
    oracle = [fo.cosine_fast(*p) for p in pairs]
    for tol in pc.TOLS:
        ks = [k for k, p in enumerate(pairs) if p[4] == tol]
        m = len(ks)
        assert m > 0
        mz, it, ptr = pc.to_csr([pairs[k] for k in ks])
        order = np.arange(2 * m, dtype=np.int64)
        splits = np.arange(0, 2 * m + 1, 2, dtype=np.int64)
        for mm in min_matches_list:
            want = np.array([1.0 - (0.0 if oracle[k][1] < mm else oracle[k][0]) for k in ks])
            t = 0.999999
            got = _to_np(*ctx.exact_edges(mz, it, ptr, order, splits, tol, mm, t))
            has = want <= t
            assert has.any()
            eptr = np.concatenate([[0], np.cumsum(np.repeat(has, 2))])
            eidx = np.stack([2 * np.flatnonzero(has) + 1, 2 * np.flatnonzero(has)], 1).ravel().astype(np.int32)
            edist = np.repeat(want[has], 2)
            assert np.array_equal(got[0], eptr), (tol, mm)
            assert np.array_equal(got[1], eidx), (tol, mm)
            assert np.array_equal(got[2], edist), (tol, mm, int((got[2] != edist).sum()))
            nb_idx = np.full((2 * m, 2), -1, np.int32)
            nb_idx[0::2, 1] = 2 * np.arange(m) + 1
            nb_dist = np.full((2 * m, 2), np.inf, np.float32)
            out = ctx.rescore_neighbors(torch.from_numpy(nb_idx).to(ctx.tdev), torch.from_numpy(nb_dist).to(ctx.tdev),
                                        mz, it, ptr, order, tol, mm).cpu().numpy()
            assert np.array_equal(out[0::2, 1].view(np.uint32), want.astype(np.float32).view(np.uint32)), (tol, mm)
            assert np.isinf(out[:, 0]).all() and np.isinf(out[1::2]).all()


def test_solver_every_component_size_on_the_device(ctx):
    pairs, cov = _kept(pc.make_pairs(2000, seed=101))
    cov.check()                                              # <= 2 % dropped, every size 2..32 on both sides, transposed ones
    assert cov.pairs >= 2000 and cov.transposed > 100
    _check_pairs_on_the_device(ctx, pairs, (0, 3, 12))


@pytest.mark.parametrize("kind", ["equal", "zeros", "dupmz"])
def test_solver_tie_heavy_inputs_on_the_device(ctx, kind):
    pairs, cov = _kept(pc.make_pairs(700, seed=200 + pc.KINDS.index(kind), kind=kind))
    assert cov.dropped <= 0.02 * cov.pairs and len(cov.rows) > 20
    _check_pairs_on_the_device(ctx, pairs, (0, 3, 12))


def test_solver_quantised_intensities_on_the_device(ctx):
    """intensities from {1, 2, 3}: the matched-peak count of the optimum is ambiguous, the score is not --
    min_matches = 0 only, bit for bit"""
    pairs, cov = _kept(pc.make_pairs(700, seed=300, kind="quant"))
    assert cov.dropped <= 0.02 * cov.pairs
    _check_pairs_on_the_device(ctx, pairs, (0,))


def _three_rows(n_side):
    """rows 0 and 2: a pair whose one component is n_side x n_side; row 1: row 0 with its intensities perturbed (the first
    perturbation with d01 < d12 < d02, so that a CSR of the edges 0-1 and 1-2 alone is what exact mode would store at the
    height where average linkage joins row 2).  Distances by the oracle where it can (n_side <= 32)."""
    a_mz, a_it, b_mz, b_it, tol = pc.exact_pair(n_side)
    assert (n_side, n_side) in pc.components(a_mz, b_mz, tol)
    for seed in range(50):
        rng = np.random.default_rng(seed)
        c_it = _normalise(a_it * rng.uniform(0.85, 1.15, len(a_it)))
        mzs, its = [a_mz, a_mz, b_mz], [a_it, c_it, b_it]
        D = np.zeros((3, 3))
        for i in range(3):
            for j in range(i + 1, 3):
                D[i, j] = D[j, i] = 1.0 - fo.cosine_fast(mzs[i], its[i], mzs[j], its[j], tol)[0]
        if D[0, 1] < D[1, 2] < D[0, 2] < 0.999:
            break
    else:
        raise AssertionError("no perturbation with d01 < d12 < d02")
    d = dict(mz=np.concatenate(mzs), intensity=np.concatenate(its).astype(np.float32),
             indptr=np.concatenate([[0], np.cumsum([len(x) for x in mzs])]).astype(np.int64),
             precursor_mz=np.array([600.0, 600.0001, 600.0002], np.float32), retention_time=np.zeros(3, np.float32))
    return d, D, tol


def _hand_csr(ctx, D):
    import torch
    assert D[0, 1] == D[1, 0] and D[1, 2] == D[2, 1]
    ptr, idx, dist = lc.pairs_to_csr(3, [0, 1], [1, 2], [D[0, 1], D[1, 2]])    # the pairs (0, 1) and (1, 2), not (0, 2)
    assert ptr.tolist() == [0, 1, 3, 4] and idx.tolist() == [1, 0, 2, 1]
    assert dist.tolist() == [D[0, 1], D[1, 0], D[1, 2], D[2, 1]]
    return tuple(torch.from_numpy(x).to(ctx.tdev) for x in (ptr, idx, dist))


def test_component_of_exactly_32_through_every_consumer(ctx):
    import torch
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    from falcon_amd.cluster.cluster import AnnParams, SpectrumDataset, generate_clusters
    d, D, tol = _three_rows(32)
    order, splits = np.arange(3, dtype=np.int64), np.array([0, 3], np.int64)
    # the edge pass
    ptr, idx, dist = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, tol, 0, 0.999))
    eptr, eidx, edist = _expected_csr([D], splits, 3, 0.999)
    assert len(eidx) == 6
    assert np.array_equal(ptr, eptr) and np.array_equal(idx, eidx) and np.array_equal(dist, edist)
    # re-scoring: slot (0 -> 2)
    nb_idx = torch.tensor([[2], [-1], [-1]], dtype=torch.int32, device=ctx.tdev)
    nb_dist = torch.full((3, 1), float("inf"), dtype=torch.float32, device=ctx.tdev)
    out = ctx.rescore_neighbors(nb_idx, nb_dist, d["mz"], d["intensity"], d["indptr"], order, tol, 0).cpu().numpy()
    assert out[0, 0].view(np.uint32) == np.float32(D[0, 2]).view(np.uint32)
    # the average-linkage fill: the CSR joins 0-1 and 1-2 only, the pair (0, 2) is scored by the fill alone.  Cut at the very
    # height where scipy joins row 2 (one cluster of three) and one ulp below (rows 0, 1 and a group of one)
    Z = linkage(squareform(D, checks=False), "average")
    h = float(Z[-1, 2])
    assert D[1, 2] <= h < D[0, 2]
    for t, n_members in ((h, 3), (np.nextafter(h, 0.0), 2)):
        exp = _scipy_labels([D], splits, 3, t, "average")
        assert (exp >= 0).sum() == n_members
        lab, n_cl = ctx.linkage_cluster_csr(*_hand_csr(ctx, D), t, "average", d["mz"], d["intensity"], d["indptr"], order, tol, 0)
        assert n_cl == 1 and np.array_equal(lab.cpu().numpy(), exp), t
    # the fused pass: labels and the medoid of the 3-row cluster (the medoid pass scores (0, 2) again)
    for method in ("average", "complete"):
        ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
        labels, medoids = generate_clusters(ds, method, 0.999, 0, 20.0, "ppm", None, tol, 2 ** 15,
                                            ann=AnnParams(eps=0.999, exact=True, mz_interval=0))
        exp = _restate(d, 20.0, "ppm", None, tol, 0.999, method, 0)
        assert list(map(len, exp)) == [3]
        assert _gpu_clusters(labels, medoids) == exp


def test_component_of_33_raises_from_every_consumer(ctx):
    """(the medoid pass has an error path of its own, `ex_medoid_score_kernel`; it cannot be isolated through the public
    calls -- the edge pass of the same call has seen every pair of the bucket before -- and is not covered here)"""
    import torch
    from falcon_amd._lib import FalconHipError
    d, D, tol = _three_rows(32)
    d33, _, _ = _three_rows_33()
    order, splits = np.arange(3, dtype=np.int64), np.array([0, 3], np.int64)
    peaks = (d33["mz"], d33["intensity"], d33["indptr"], order)
    with pytest.raises(FalconHipError, match="32 peaks"):
        ctx.exact_edges(*peaks, splits, tol, 0, 0.999)
    nb_idx = torch.tensor([[2], [-1], [-1]], dtype=torch.int32, device=ctx.tdev)
    nb_dist = torch.full((3, 1), float("inf"), dtype=torch.float32, device=ctx.tdev)
    with pytest.raises(FalconHipError, match="32 peaks"):
        ctx.rescore_neighbors(nb_idx, nb_dist, *peaks, tol, 0)
    with pytest.raises(FalconHipError, match="32 peaks"):      # the same hand-written CSR: only the fill sees the pair (0, 2)
        ctx.linkage_cluster_csr(*_hand_csr(ctx, D), 0.999, "average", *peaks, tol, 0)
    mz_sorted = torch.from_numpy(d33["precursor_mz"]).to(ctx.tdev)
    rt_sorted = torch.from_numpy(d33["retention_time"]).to(ctx.tdev)
    with pytest.raises(FalconHipError, match="32 peaks"):
        ctx.cluster_exact(*peaks, splits, tol, 0, 0.999, "average", mz_sorted, rt_sorted, 20.0, "ppm", None)
    # and the context still works afterwards
    ptr, idx, dist = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, tol, 0, 0.999))
    assert len(idx) == 6


def _three_rows_33():
    """rows 0 and 2 with a 33 x 33 component, row 1 three far-away peaks: (0, 2) is the only pair above the limit"""
    a_mz, a_it, b_mz, b_it, tol = pc.exact_pair(33)
    c_mz = np.array([200.0, 300.0, 900.0], np.float32)
    assert (33, 33) in pc.components(a_mz, b_mz, tol) and pc.too_large(pc.components(a_mz, b_mz, tol))
    assert not pc.too_large(pc.components(a_mz, c_mz, tol)) and not pc.too_large(pc.components(c_mz, b_mz, tol))
    mzs, its = [a_mz, c_mz, b_mz], [a_it, _normalise(np.ones(3)), b_it]
    d = dict(mz=np.concatenate(mzs), intensity=np.concatenate(its).astype(np.float32),
             indptr=np.concatenate([[0], np.cumsum([len(x) for x in mzs])]).astype(np.int64),
             precursor_mz=np.array([600.0, 600.0001, 600.0002], np.float32), retention_time=np.zeros(3, np.float32))
    return d, None, tol


# ---------------------------------------------------------------------------------------------------------- 5. edges
@pytest.fixture(scope="module")
def odd_buckets():
    sizes = [0, 1, 2, 0, 63, 64, 65, 0, 128, 129, 0]
    n = sum(sizes)
    d = base._spectra(5, n, [600.0], seed=61, chained=0)
    rng = np.random.default_rng(62)
    order = rng.permutation(n).astype(np.int64)
    splits = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    mats = [_block_matrix(d, order, s0, s1, 0.05, 0) for s0, s1 in zip(splits[:-1], splits[1:])]
    return d, order, splits, mats


def test_empty_and_odd_sized_buckets_in_one_call(ctx, odd_buckets):
    d, order, splits, mats = odd_buckets
    assert splits[0] == splits[1] and splits[-1] == splits[-2] and (np.diff(splits) == 0).sum() == 4
    t = 0.45
    got = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, 0.05, 0, t))
    exp = _expected_csr(mats, splits, len(order), t)
    assert len(exp[1]) > 2000
    assert all(np.array_equal(g, e) for g, e in zip(got, exp))


def test_distance_equal_to_the_threshold_is_an_edge(ctx, odd_buckets):
    d, order, splits, mats = odd_buckets
    D = mats[-2]                                             # the 129-row bucket
    vals = D[np.triu_indices(len(D), 1)]
    v = float(np.sort(vals[(vals > 0) & (vals < 1)])[len(vals[(vals > 0) & (vals < 1)]) // 3])
    assert 0.0 < v < 1.0
    n = len(order)
    at = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, 0.05, 0, v))
    below = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, 0.05, 0, float(np.nextafter(v, 0.0))))
    e_at, e_below = _expected_csr(mats, splits, n, v), _expected_csr(mats, splits, n, float(np.nextafter(v, 0.0)))
    n_eq = sum(int((np.triu(M, 1) == v).sum()) for M in mats)
    assert n_eq >= 1 and len(e_at[1]) == len(e_below[1]) + 2 * n_eq
    assert all(np.array_equal(g, e) for g, e in zip(at, e_at))
    assert all(np.array_equal(g, e) for g, e in zip(below, e_below))


def _grid_spectra(rng, n, n_peaks, lo=400.0, slots=160, step=0.25):
    """m/z on a grid of multiples of 0.25 (exact in float32): identical values across spectra, differences of exactly 0.5"""
    mz, it = [], []
    for _ in range(n):
        m = np.sort(lo + step * rng.choice(slots, n_peaks, replace=False)).astype(np.float32)
        mz.append(m)
        it.append(_normalise(rng.uniform(0.1, 1.0, n_peaks)))
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in mz])]).astype(np.int64)
    return dict(mz=np.concatenate(mz), intensity=np.concatenate(it), indptr=indptr)


@pytest.mark.parametrize("tol", [0.0, 0.5])
def test_fragment_tolerance_zero_and_differences_equal_to_it(ctx, tol):
    rng = np.random.default_rng(71)
    n = 70
    d = _grid_spectra(rng, n, 14)
    order, splits = rng.permutation(n).astype(np.int64), np.array([0, n], np.int64)
    D = _block_matrix(d, order, 0, n, tol, 0)
    n_at_tol = 0                                             # peak pairs exactly `tol` apart exist (computed from the input)
    for i in range(0, n, 7):
        a, b = _peaks(d, order[i])[0], _peaks(d, order[(i + 1) % n])[0]
        n_at_tol += int((np.abs(a[:, None] - b[None, :]) == np.float32(tol)).sum())
    assert n_at_tol > 0
    t = 0.95
    got = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, tol, 0, t))
    exp = _expected_csr([D], splits, n, t)
    assert len(exp[1]) > 200
    assert all(np.array_equal(g, e) for g, e in zip(got, exp))


def test_one_ulp_outside_the_tolerance_does_not_match(ctx):
    one = np.array([1.0], np.float32)
    inside, outside = np.float32(500.5), np.nextafter(np.float32(500.5), np.float32(np.inf))
    assert fo.cosine_fast(np.array([500.0], np.float32), one, np.array([inside]), one, 0.5) == (1.0, 1)
    assert fo.cosine_fast(np.array([500.0], np.float32), one, np.array([outside]), one, 0.5) == (0.0, 0)
    mz = np.array([500.0, inside, 500.0, outside, inside, 500.0, outside, 500.0], np.float32)        # both orientations
    it = np.ones(8, np.float32)
    ptr, idx, dist = _to_np(*ctx.exact_edges(mz, it, np.arange(9, dtype=np.int64), np.arange(8, dtype=np.int64),
                                             np.arange(0, 9, 2, dtype=np.int64), 0.5, 0, 0.5))
    assert np.array_equal(ptr, [0, 1, 2, 2, 2, 3, 4, 4, 4])
    assert np.array_equal(idx, [1, 0, 5, 4]) and np.array_equal(dist, np.zeros(4))


def test_no_rows_and_one_row(ctx):
    e32, e64 = np.zeros(0, np.float32), np.zeros(0, np.int64)
    ptr, idx, dist = _to_np(*ctx.exact_edges(e32, e32, np.zeros(1, np.int64), e64, np.zeros(1, np.int64), 0.05, 0, 0.5))
    assert np.array_equal(ptr, [0]) and len(idx) == 0 and len(dist) == 0
    mz = np.array([200.0, 300.0], np.float32)
    ptr, idx, dist = _to_np(*ctx.exact_edges(mz, np.ones(2, np.float32), np.array([0, 2], np.int64), np.zeros(1, np.int64),
                                             np.array([0, 1], np.int64), 0.05, 0, 0.5))
    assert np.array_equal(ptr, [0, 0]) and len(idx) == 0


def test_spectra_without_peaks(ctx):
    """a bucket of spectra that hold no peaks at all: every distance is 1, no edge, every row a group of one"""
    import torch
    n = 70
    e32 = np.zeros(0, np.float32)
    indptr, order, splits = np.zeros(n + 1, np.int64), np.arange(n, dtype=np.int64), np.array([0, n], np.int64)
    ptr, idx, dist = ctx.exact_edges(e32, e32, indptr, order, splits, 0.05, 0, 0.999999)
    assert np.array_equal(ptr.cpu().numpy(), np.zeros(n + 1)) and idx.numel() == 0
    pm = torch.full((n,), 600.0, dtype=torch.float32, device=ctx.tdev)
    rt = torch.zeros(n, dtype=torch.float32, device=ctx.tdev)
    for method in ("single", "complete", "average"):
        labels, medoids, lab_sorted, n_cl = ctx.cluster_exact(e32, e32, indptr, order, splits, 0.05, 0, 0.999999, method, pm, rt,
                                                              20.0, "ppm", None)
        assert n_cl == 0
        assert np.array_equal(np.sort(labels.cpu().numpy()), np.arange(n)) and len(medoids) == n
