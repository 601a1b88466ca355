"""Exact mode on the GPU (`fal_exact_edges`, `fal_linkage_cluster_csr`, `fal_cluster_exact`, `AnnParams(exact=True)`,
`--exact`): the snapshot's own clustering -- the matched-peak cosine of every pair of a precursor block, linkage + fcluster at
the distance threshold, refinement, medoids over the full matrix (reference cluster.py:212-331, 512-553, 593-639).  The
expected results are built here from pieces pinned to reference goldens: `fo.cosine_fast`, `fo.bucket_splits`, scipy's
`linkage` + `fcluster` on the float64 condensed matrix, `fo.postprocess_cluster`, and the float32 medoid sums of
`fo.medoids_dense` in ascending member order."""
import os

import numpy as np
import pytest

from oracle import falcon_oracle as fo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------- data
def _spectra(n_templates, per, pmz_centres, seed, jitter=0.002, chained=0, n_peaks=40, drop=0.15, it_noise=None):
    """spectra drawn around peak templates (jittered m/z, a `drop` share of the peaks left out, random intensities -- or the
    template's times 1 +- it_noise --, L2-normalised) + `chained` spectra per bucket whose peaks sit closer than the fragment
    tolerance (components of several peaks: the fallback solver)"""
    rng = np.random.default_rng(seed)
    mz, it, pmz = [], [], []
    for b, centre in enumerate(pmz_centres):
        temps = [np.sort(rng.uniform(150, 1400, n_peaks)) for _ in range(n_templates)]
        t_it = [rng.uniform(0.1, 1.0, n_peaks) for _ in range(n_templates)]
        for _ in range(per):
            ti = rng.integers(n_templates)
            t = temps[ti]
            keep = rng.random(len(t)) >= drop
            m = t[keep] + rng.normal(0, jitter, keep.sum())
            o = np.argsort(m)
            mz.append(m[o].astype(np.float32))
            if it_noise is None:
                it.append(rng.uniform(0.1, 1.0, len(m)).astype(np.float32))
            else:
                it.append((t_it[ti][keep] * rng.uniform(1 - it_noise, 1 + it_noise, len(m)))[o].astype(np.float32))
            pmz.append(centre + rng.uniform(-0.002, 0.002))
        for _ in range(chained):
            base = rng.uniform(300, 900)
            m = np.sort(np.concatenate([base + 0.03 * np.arange(6) + rng.normal(0, 0.002, 6), rng.uniform(150, 1400, 10)]))
            mz.append(m.astype(np.float32))
            it.append(rng.uniform(0.1, 1.0, len(m)).astype(np.float32))
            pmz.append(centre + rng.uniform(-0.002, 0.002))
    it = [x / np.sqrt(np.sum(x.astype(np.float64) ** 2)).astype(np.float32) for x in it]
    perm = rng.permutation(len(mz))                          # dataset order != precursor order
    mz, it, pmz = [mz[i] for i in perm], [it[i] for i in perm], np.asarray(pmz, np.float32)[perm]
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in mz])]).astype(np.int64)
    return dict(mz=np.concatenate(mz).astype(np.float32), intensity=np.concatenate(it).astype(np.float32), indptr=indptr,
                precursor_mz=pmz, retention_time=rng.uniform(0, 100, len(pmz)).astype(np.float32))


def _peaks(d, r):
    a, b = d["indptr"][r], d["indptr"][r + 1]
    return d["mz"][a:b], d["intensity"][a:b]


def _dist(d, order, i, j, tol, min_matches):
    """the reference's pair distance of sorted rows i < j (cluster.py:617-626)"""
    sim, nm = fo.cosine_fast(*_peaks(d, order[i]), *_peaks(d, order[j]), tol)
    return 1.0 - (0.0 if nm < min_matches else sim)


def _block_matrix(d, order, s0, s1, tol, min_matches):
    m = s1 - s0
    D = np.zeros((m, m))
    for a in range(m):
        for b in range(a + 1, m):
            D[a, b] = D[b, a] = _dist(d, order, s0 + a, s0 + b, tol, min_matches)
    return D


def _sorted(d, tol, mode, batch_size=2 ** 15):
    order = np.argsort(d["precursor_mz"], kind="stable")
    mzs = d["precursor_mz"][order]
    return order, mzs, fo.bucket_splits(mzs, tol, mode, batch_size, 0.0)


def _expected_csr(mats, splits, n, t):
    rows, cols, vals = [], [], []
    for (s0, s1), D in zip(zip(splits[:-1], splits[1:]), mats):
        a, b = np.nonzero((D <= t) & ~np.eye(len(D), dtype=bool))
        rows.append(a + s0)
        cols.append(b + s0)
        vals.append(D[a, b])
    rows, cols, vals = (np.concatenate(x) for x in (rows, cols, vals))
    o = np.lexsort((cols, rows))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return ptr, cols[o].astype(np.int32), vals[o]


def _to_np(*ts):
    return [t.cpu().numpy() for t in ts]


# ---------------------------------------------------------------------------------------------------------- 1. edges
@pytest.fixture(scope="module")
def edge_data():
    d = _spectra(6, 110, [500.0, 520.0, 640.0, 700.0], seed=3, chained=8)
    return d


@pytest.mark.parametrize("min_matches,tol,mode", [(0, 0.05, "ppm"), (3, 0.05, "Da"), (0, 0.5, "Da"), (3, 0.5, "ppm")])
def test_edges_equal_brute_force(ctx, edge_data, min_matches, tol, mode):
    d = edge_data
    n = len(d["precursor_mz"])
    order, mzs, splits = _sorted(d, 20.0 if mode == "ppm" else 0.05, mode, batch_size=200)
    assert len(splits) == 5                                  # four buckets
    t = 0.45
    mats = [_block_matrix(d, order, s0, s1, tol, min_matches) for s0, s1 in zip(splits[:-1], splits[1:])]
    ptr, idx, dist = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, tol, min_matches, t))
    eptr, eidx, edist = _expected_csr(mats, splits, n, t)
    assert len(eidx) > 1000
    assert np.array_equal(ptr, eptr)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(dist, edist)                       # float64, bit for bit
    again = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, tol, min_matches, t))
    assert all(np.array_equal(x, y) for x, y in zip((ptr, idx, dist), again))


def test_edges_of_the_cosine_fast_golden(ctx):
    """the golden's pairs (reference `cosine_fast` outputs): pair k = spectra (2k, 2k + 1), one bucket each"""
    g = np.load(os.path.join(GOLDEN, "cosine_fast.npz"))
    for tol in np.unique(g["tol"]):
        ks = np.flatnonzero(g["tol"] == tol)
        mz, it, ptr = [], [], [0]
        for k in ks:
            for side in ("a", "b"):
                p = g[f"{side}_ptr"]
                mz.append(g[f"{side}_mz"][p[k]:p[k + 1]])
                it.append(g[f"{side}_it"][p[k]:p[k + 1]])
                ptr.append(ptr[-1] + p[k + 1] - p[k])
        n = 2 * len(ks)
        splits = np.arange(0, n + 1, 2, dtype=np.int64)
        e_ptr, e_idx, e_dist = _to_np(*ctx.exact_edges(np.concatenate(mz).astype(np.float32),
                                                       np.concatenate(it).astype(np.float32), np.asarray(ptr, np.int64),
                                                       np.arange(n, dtype=np.int64), splits, float(tol), 0, 0.999999))
        for x, k in enumerate(ks):
            got = e_dist[e_ptr[2 * x]:e_ptr[2 * x + 1]]
            # the oracle's cosine_fast is pinned to the golden (stored as float32); the distance is 1 - its float64 score
            sim, _ = fo.cosine_fast(mz[2 * x], it[2 * x], mz[2 * x + 1], it[2 * x + 1], float(tol))
            assert abs(sim - float(g["score"][k])) <= 1e-6
            want = 1.0 - sim
            if want <= 0.999999:
                assert len(got) == 1 and e_idx[e_ptr[2 * x]] == 2 * x + 1 and got[0] == want, (k, got, want)
            else:
                assert len(got) == 0


def test_component_beyond_32_peaks_raises(ctx):
    from falcon_amd._lib import FalconHipError
    mz = np.concatenate([500 + 0.01 * np.arange(40), 500 + 0.01 * np.arange(40)]).astype(np.float32)
    it = np.full(80, 0.15, np.float32)
    with pytest.raises(FalconHipError, match="32 peaks"):
        ctx.exact_edges(mz, it, np.array([0, 40, 80], np.int64), np.arange(2, dtype=np.int64), np.array([0, 2], np.int64),
                        0.5, 0, 0.5)


# ---------------------------------------------------------------------------------------------------------- 2. linkage
def _scipy_labels(mats, splits, n, t, method):
    """fcluster(linkage(pdist, method), t, "distance") per block -> labels numbered by lowest row, groups of one = -1"""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    rep = np.full(n, -1, np.int64)
    for (s0, s1), D in zip(zip(splits[:-1], splits[1:]), mats):
        if s1 - s0 < 2:
            continue
        lab = fcluster(linkage(squareform(D, checks=False), method), t, "distance")
        for c in np.unique(lab):
            m = np.flatnonzero(lab == c)
            if len(m) >= 2:
                rep[s0 + m] = s0 + m.min()
    is_rep = np.zeros(n, np.int64)
    is_rep[rep[rep >= 0]] = 1
    rank = np.cumsum(is_rep) - is_rep
    return np.where(rep >= 0, rank[np.maximum(rep, 0)], -1).astype(np.int32)


@pytest.mark.parametrize("method", ["single", "complete", "average"])
def test_linkage_on_the_csr_equals_scipy(ctx, edge_data, method):
    d = edge_data
    n = len(d["precursor_mz"])
    tol, mm, t = 0.05, 0, 0.45
    order, mzs, splits = _sorted(d, 20.0, "ppm", batch_size=200)
    mats = [_block_matrix(d, order, s0, s1, tol, mm) for s0, s1 in zip(splits[:-1], splits[1:])]
    ptr, idx, dist = ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, tol, mm, t)
    lab, n_cl = ctx.linkage_cluster_csr(ptr, idx, dist, t, method, d["mz"], d["intensity"], d["indptr"], order, tol, mm)
    exp = _scipy_labels(mats, splits, n, t, method)
    lab = lab.cpu().numpy()
    assert n_cl == exp.max() + 1 and n_cl > 10
    assert np.array_equal(lab, exp), int((lab != exp).sum())


# ---------------------------------------------------------------------------------------------------------- 3. motivation
def test_300_spectra_of_one_peptide_form_one_cluster():
    """ISSUE: one 40-peak template, m/z jitter 0.002, random intensities, one precursor bucket; every pair has d <= 0.073.
    The reference (all pairs -> complete linkage -> fcluster(0.3)) makes ONE cluster of 300; the ANN path's linkage on
    neighbour lists cannot (a cluster needs all its pairs stored, a row stores n_neighbors of them)."""
    from falcon_amd.cluster.cluster import AnnParams, SpectrumDataset, generate_clusters
    d = _spectra(1, 300, [600.0], seed=11, drop=0.0, it_noise=0.3)
    ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    labels, medoids = generate_clusters(ds, "complete", 0.3, 0, 20.0, "ppm", None, 0.05, 2 ** 15,
                                        ann=AnnParams(eps=0.3, exact=True, mz_interval=0))
    assert len(medoids) == 1 and bool((labels == 0).all())


# ---------------------------------------------------------------------------------------------------------- 4. end to end
def _restate(d, tol_mass, mode, rt_tol, frag_tol, t, method, min_matches, batch_size=2 ** 15):
    """the reference's _cluster_interval per block (cluster.py:266-331): -> {frozenset(dataset rows): medoid dataset row}"""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    order, mzs, splits = _sorted(d, tol_mass, mode, batch_size)
    rts = d["retention_time"][order]
    out = {}
    for s0, s1 in zip(splits[:-1], splits[1:]):
        if s1 - s0 < 2:
            continue
        D = _block_matrix(d, order, s0, s1, frag_tol, min_matches)
        lab = fcluster(linkage(squareform(D, checks=False), method), t, "distance") - 1
        o = np.argsort(lab, kind="stable")
        lab = lab[o].astype(np.int64)
        cur = 0
        for a, b in fo.cluster_group_idx(lab):
            seg = lab[a:b].copy()
            k = fo.postprocess_cluster(seg, mzs[s0:s1][o][a:b], rts[s0:s1][o][a:b] if rt_tol is not None else None,
                                       tol_mass, mode, rt_tol, 2, cur)
            lab[a:b] = seg
            cur += k
        for c in range(cur):
            mem = np.sort(o[lab == c])                          # block positions, ascending
            s = np.zeros(len(mem), np.float32)
            for x in range(len(mem)):
                for y in range(len(mem)):
                    if x != y:
                        i, j = sorted((mem[x], mem[y]))
                        s[x] = np.float32(s[x] + np.float32(D[i, j]))
            out[frozenset(order[s0 + mem].tolist())] = int(order[s0 + mem[int(np.argmin(s))]])
    return out


def _gpu_clusters(labels, medoids):
    out = {}
    for c in range(len(medoids)):
        m = np.flatnonzero(labels == c)
        if len(m) >= 2:
            out[frozenset(m.tolist())] = int(medoids[c])
    return out


@pytest.mark.parametrize("method,rt_tol,mode", [("complete", None, "ppm"), ("average", 5.0, "Da"), ("single", None, "Da"),
                                                ("complete", 30.0, "ppm"), ("average", None, "ppm")])
def test_generate_clusters_exact_equals_the_restatement(method, rt_tol, mode):
    from falcon_amd.cluster.cluster import AnnParams, SpectrumDataset, generate_clusters
    d = _spectra(5, 70, [450.0, 451.5, 800.0, 1200.0], seed=17, jitter=0.01, chained=4)
    tol_mass = 20.0 if mode == "ppm" else 0.05
    t, mm = 0.35, 2
    ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    labels, medoids = generate_clusters(ds, method, t, mm, tol_mass, mode, rt_tol, 0.05, 2 ** 15,
                                        ann=AnnParams(eps=t, exact=True, mz_interval=0))
    got = _gpu_clusters(labels, medoids)
    exp = _restate(d, tol_mass, mode, rt_tol, 0.05, t, method, mm)
    assert len(exp) > 8
    assert got == exp


def test_block_of_16k_rows_sampled_rows_equal_brute_force(ctx):
    """one bucket of 16,500 rows (258 tiles a side): sampled rows -- tile edges and the last, partial tile -- against brute force"""
    rng = np.random.default_rng(5)
    n = 16500
    d = _spectra(300, n, [700.0], seed=23, n_peaks=30)
    d["precursor_mz"] = (700.0 + 1e-5 * np.arange(n)).astype(np.float32)[rng.permutation(n)]
    order, mzs, splits = _sorted(d, 20.0, "ppm")
    assert len(splits) == 2 and splits[-1] == n
    tol, mm, t = 0.05, 0, 0.3
    ptr, idx, dist = _to_np(*ctx.exact_edges(d["mz"], d["intensity"], d["indptr"], order, splits, tol, mm, t,
                                             max_edges=60_000_000))
    assert ptr[-1] == len(idx) > n
    for i in [0, 1, 63, 64, 65, 127, 128, 8191, 16383, 16384, 16447, 16448, n - 2, n - 1]:
        cand = np.array([j for j in range(n) if j != i])
        ds_ = np.array([_dist(d, order, min(i, j), max(i, j), tol, mm) for j in cand])
        keep = ds_ <= t
        assert np.array_equal(idx[ptr[i]:ptr[i + 1]], cand[keep].astype(np.int32)), i
        assert np.array_equal(dist[ptr[i]:ptr[i + 1]], ds_[keep]), i


# ---------------------------------------------------------------------------------------------------------- 5. CLI
def test_main_exact_average_csv_and_representatives(tmp_path):
    from falcon_amd.falcon import main
    from falcon_amd.ms_io import ms_io
    d = _spectra(4, 60, [500.0, 620.0], seed=29, jitter=0.005, n_peaks=30)
    specs = []
    for i in range(len(d["precursor_mz"])):
        m, it = _peaks(d, i)
        specs.append({"identifier": f"scan={i}", "precursor_mz": float(d["precursor_mz"][i]), "precursor_charge": 2,
                      "retention_time": float(d["retention_time"][i]), "mz": m.astype(np.float64), "intensity": it})
    mgf = str(tmp_path / "in.mgf")
    ms_io.write_spectra(mgf, specs)
    out, work = str(tmp_path / "res"), tmp_path / "work"
    args = [mgf, out, "--exact", "--linkage", "average", "--eps", "0.35", "--min_matched_peaks", "2", "--export_representatives",
            "--work_dir", str(work), "--mz_interval", "0"]
    assert main(args) == 0
    lines = open(out + ".csv").read().splitlines()
    assert "# exact = True" in lines and "# clustering = hierarchical" in lines
    body = [l.split(",") for l in lines if not l.startswith("#")][1:]
    table = {r[1]: int(r[5]) for r in body}
    z = np.load(work / "spectra" / "spectra_charge_2.npz")
    part = {k: z[k] for k in z.files}
    names = [str(x) for x in part["identifier"]]              # row r of the charge's partition
    exp = _restate(part, 20.0, "ppm", None, 0.05, 0.35, "average", 2)
    assert len(exp) > 4
    lab = np.array([table[nm] for nm in names])
    groups = {}
    for r, l in enumerate(lab):
        groups.setdefault(l, []).append(r)
    got = {frozenset(v) for v in groups.values() if len(v) >= 2}
    assert got == set(exp)
    reps = {s["identifier"] for s in ms_io.get_spectra(out + ".mgf")}
    assert len(reps) == len(set(lab))
    for members, med in exp.items():
        assert names[med] in reps                              # the exact medoid represents its cluster
