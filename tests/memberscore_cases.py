"""Member scores and cluster summary (`fal_member_scores`, `fal_cluster_summary`; DESIGN.md "Member scores and cluster summary"):
the numpy restatement of the rule -- per pair the oracle's `cosine_fast`, per cluster the fold in the stated order -- and the case
generators of the CPU and GPU tests.

A case is a dict: mz, intensity f32[nnz], indptr i64[n+1], labels i32[n], medoids i32[n_clusters], precursor_mz,
retention_time f32[n].  A representative CSR is a dict(mz, intensity, indptr) with a `rep_row` i32[n_clusters] beside it."""
import numpy as np

from oracle import falcon_oracle as fo
from tests import assign_cases as ac
from tests import consensus_cases as cc
from tests import peakmatch_cases as pc

f32, f64 = np.float32, np.float64
CHAINS = 64            # csrc/memberscore.h kMsChains
COLUMNS = ("size", "sim_min", "worst_row", "sim_mean", "pmz_min", "pmz_max", "rt_min", "rt_max")


def peaks(d, r):
    a, b = d["indptr"][r], d["indptr"][r + 1]
    return d["mz"][a:b], d["intensity"][a:b]


def medoid_form(case):
    """the representatives of the medoid form: the partition's own CSR, rep_row = medoids"""
    return dict(mz=case["mz"], intensity=case["intensity"], indptr=case["indptr"]), np.asarray(case["medoids"], np.int32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def scores_ref(case, rep, rep_row, fragment_tol, stats=None, rows=None):
    """per member cosine_fast(member, representative of its label) -> (similarity f32[n], matched i32[n]).  `stats` (a dict)
    receives solver_pairs (pairs with a component of two or more member peaks) and max_component.  `rows`: only these members
    (the others stay 0)."""
    labels = np.asarray(case["labels"])
    n, nc, n_rep = len(labels), len(rep_row), len(rep["indptr"]) - 1
    sim, matched = np.zeros(n, f32), np.zeros(n, np.int32)
    solver = max_comp = 0
    empty = (np.zeros(0, f32), np.zeros(0, f32))
    for i in (range(n) if rows is None else rows):
        c = int(labels[i])
        if not 0 <= c < nc:
            continue
        r = int(rep_row[c])
        b = peaks(rep, r) if 0 <= r < n_rep else empty
        a = peaks(case, i)
        s, m = fo.cosine_fast(*a, *b, fragment_tol)
        sim[i], matched[i] = f32(s), m
        if stats is not None:
            comps = pc.components(a[0], b[0], fragment_tol)
            solver += any(x >= 2 for x, _ in comps)
            max_comp = max([max_comp] + [max(x, y) for x, y in comps if x >= 2])
    if stats is not None:
        stats.update(solver_pairs=int(solver), max_component=int(max_comp))
    return sim, matched


def mean_ref(sims):
    """the float64 sum in the stated order, over the size: member p (row order) goes to chain p mod 64, every chain one member
    after the other; then the chains one after the other from 0.0, chain 0 first"""
    chain = [0.0] * CHAINS
    for p, s in enumerate(sims):
        chain[p % CHAINS] += float(f32(s))
    total = 0.0
    for x in chain:
        total += x
    return total / len(sims) if len(sims) else 0.0


def summary_ref(labels, n_clusters, sim, pmz, rt=None, clusters=None):
    """-> dict of the per-cluster columns (COLUMNS); `clusters`: only these ids (the others stay as if empty)"""
    labels, sim, pmz = np.asarray(labels), np.asarray(sim, f32), np.asarray(pmz, f32)
    rt = np.zeros(len(labels), f32) if rt is None else np.asarray(rt, f32)
    out = dict(size=np.zeros(n_clusters, np.int32), sim_min=np.zeros(n_clusters, f32), worst_row=np.full(n_clusters, -1, np.int32),
               sim_mean=np.zeros(n_clusters, f64), pmz_min=np.zeros(n_clusters, f32), pmz_max=np.zeros(n_clusters, f32),
               rt_min=np.zeros(n_clusters, f32), rt_max=np.zeros(n_clusters, f32))
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(n_clusters + 1))
    for c in (range(n_clusters) if clusters is None else clusters):
        rows = order[bounds[c]:bounds[c + 1]]                # ascending rows
        if len(rows) == 0:
            continue
        s = sim[rows]
        w = int(np.argmin(s))                                 # (the first of equals: the lowest row)
        out["size"][c], out["sim_min"][c], out["worst_row"][c] = len(rows), s[w], rows[w]
        out["sim_mean"][c] = mean_ref(s)
        out["pmz_min"][c], out["pmz_max"][c] = pmz[rows].min(), pmz[rows].max()
        out["rt_min"][c], out["rt_max"][c] = rt[rows].min(), rt[rows].max()
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- generators --------------------------------------------------------------------------------------------------------------
def with_columns(part, rng):
    """a partition of consensus_cases -> a case (precursor m/z around the cluster, retention times anywhere)"""
    n = len(part["labels"])
    part = dict(part)
    part["precursor_mz"] = (500.0 + 3.0 * part["labels"] + rng.uniform(-0.01, 0.01, n)).astype(f32)
    part["retention_time"] = rng.uniform(0.0, 3600.0, n).astype(f32)
    return part


def from_spectra(mzs, its, labels, medoids, rng):
    side = ac.side(mzs, its, np.zeros(len(mzs), f32))
    return with_columns(dict(mz=side["mz"], intensity=side["intensity"], indptr=side["indptr"],
                             labels=np.asarray(labels, np.int32), medoids=np.asarray(medoids, np.int32)), rng)


FRAGMENT_TOL_TEMPLATE = 1.0


def template_case(seed=3):
    """consensus_cases.template_spectra (300 spectra drawn from 8 peak templates; it tells which, assign_cases' generator does
    not) clustered by template, a random member as medoid: at a fragment tolerance of 1.0 the templates' close peaks chain, and
    most pairs have a component for the solver"""
    d = cc.template_spectra(seed, n_templates=8, n_spectra=300)
    rng = np.random.default_rng(seed)
    labels = d["template"].astype(np.int32)
    medoids = np.array([rng.choice(np.flatnonzero(labels == c)) for c in range(8)], np.int32)
    case = dict(mz=d["mz"], intensity=d["intensity"], indptr=d["indptr"], labels=labels, medoids=medoids,
                precursor_mz=d["precursor_mz"], retention_time=d["retention_time"])
    return case, FRAGMENT_TOL_TEMPLATE


def solver_pairs_case(n_pairs=60, seed=11, tol=0.05):
    """clusters of two from peakmatch_cases.make_pair (dense groups of 1..32 peaks a side): member 2k against medoid 2k + 1 and
    the medoid against itself; pairs with a component beyond the solver are left out"""
    rng = np.random.default_rng(seed)
    mzs, its = [], []
    while len(mzs) < 2 * n_pairs:
        a_mz, a_it, b_mz, b_it, _ = pc.make_pair(rng, kind=str(rng.choice(pc.KINDS)), tol=tol)
        if pc.too_large(pc.components(a_mz, b_mz, tol)) or pc.too_large(pc.components(b_mz, b_mz, tol)):
            continue
        mzs += [a_mz, b_mz]
        its += [a_it, b_it]
    labels = np.repeat(np.arange(n_pairs), 2)
    return from_spectra(mzs, its, labels, 2 * np.arange(n_pairs) + 1, rng), tol


TILE_SIZES = (1, 63, 64, 65, 130)


def tile_layouts(n):
    """cluster sizes per layout name for n members"""
    out = {"singletons": [1] * n, "one": [n]}
    if n >= 3:
        k = n // 3
        out["interleaved"] = [k, k, n - 2 * k]
    if n >= 128:
        out["straddle"] = [63, 65] + [1] * (n - 128)         # a 65-member cluster from sorted position 63
    return out


def tile_case(n, layout, seed=0):
    """make_partition's clusters (rows shuffled: labels interleave in row order, the (label, row) sort matters), a few members
    without peaks"""
    rng = np.random.default_rng(1000 * n + seed)
    sizes = tile_layouts(n)[layout]
    return with_columns(cc.make_partition(rng, sizes, p_empty=0.05), rng), 0.05


def consensus_rep(case, fragment_tol, min_fraction=0.25):
    """the consensus form: the numpy consensus of the case's clusters as representative CSR, rep_row = arange"""
    ptr, mz, it, _ = cc.consensus_reference(case["mz"], case["intensity"], case["indptr"], case["labels"], case["medoids"],
                                            fragment_tol, min_fraction)
    return dict(mz=mz, intensity=it, indptr=ptr), np.arange(len(case["medoids"]), dtype=np.int32)


def permute_rep(rep, rep_row, rng):
    """the same representatives stored in another row order, rep_row permuted to match"""
    n = len(rep["indptr"]) - 1
    new_of_old = rng.permutation(n)
    old_of_new = np.argsort(new_of_old)
    spectra = [peaks(rep, r) for r in old_of_new]
    side = ac.side([s[0] for s in spectra], [s[1] for s in spectra], np.zeros(n, f32))
    return dict(mz=side["mz"], intensity=side["intensity"], indptr=side["indptr"]), new_of_old[rep_row].astype(np.int32)


def big_rep_case(seed=21, n_rep_peaks=4000):
    """three clusters; cluster 1's representative holds 4,000 peaks (more than a tile side stages in LDS), cluster 2's none;
    cluster 0 has 64 members of 60 peaks (the member side of its tile does not fit either) -> (case, rep, rep_row, tol)"""
    rng = np.random.default_rng(seed)
    case = with_columns(cc.make_partition(rng, [64, 40, 7], p_empty=0.05, overrides={0: dict(fixed_peaks=60, n_template=80)},
                                          shuffle=False), rng)
    rep, rep_row = medoid_form(case)
    reps = [peaks(rep, r) for r in rep_row]
    x = np.sort(rng.uniform(150.0, 1400.0, n_rep_peaks)).astype(f32)
    y = rng.uniform(0.1, 1.0, n_rep_peaks)
    reps[1] = (x, (y / np.sqrt(np.sum(y ** 2))).astype(f32))
    reps[2] = (np.zeros(0, f32), np.zeros(0, f32))
    side = ac.side([r[0] for r in reps], [r[1] for r in reps], np.zeros(3, f32))
    return case, dict(mz=side["mz"], intensity=side["intensity"], indptr=side["indptr"]), np.arange(3, dtype=np.int32), 0.05


def unsupported_case():
    """peakmatch_cases.exact_pair(33) (one 33 x 33 component: beyond the solver) as member and medoid of one cluster among
    ordinary clusters -> (case, tol)"""
    rng = np.random.default_rng(33)
    mz_a, it_a, mz_b, it_b, tol = pc.exact_pair(33)
    m, it = ac.small_spectra(6, rng)
    return from_spectra(m + [mz_a, mz_b], it + [it_a, it_b], [0, 0, 0, 1, 1, 1, 2, 2], [0, 3, 7], rng), tol


def fold_similarities(n, rng):
    """similarities spanning 2^-30 .. 1 (the order of a float64 sum of these is visible in its last bits), some of them equal"""
    s = (2.0 ** rng.uniform(-30.0, 0.0, n)).astype(f32)
    if n > 3:
        s[rng.integers(0, n, max(2, n // 8))] = s.min()       # ties of the minimum
    return s


def summary_case(sizes, seed=0, interleave=True):
    """clusters of `sizes` members with fold_similarities -> (labels, similarity, pmz, rt)"""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    if interleave:
        labels = labels[rng.permutation(len(labels))]
    n = len(labels)
    sim = np.zeros(n, f32)
    for c, m in enumerate(sizes):
        sim[labels == c] = fold_similarities(m, rng)
    return labels, sim, rng.uniform(300.0, 900.0, n).astype(f32), rng.uniform(0.0, 3600.0, n).astype(f32)


SUMMARY_SIZES = [1, 2, 64, 65, 5000, 0, 3]                   # (with an empty cluster in the middle)
