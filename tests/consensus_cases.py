"""Consensus representatives: the numpy restatement of the definition (DESIGN.md "Consensus representatives") and the case
generators of the CPU and GPU tests.  The restatement is a plain loop over clusters, groups and peaks: float64 sums in pooled
order (m/z, dataset row, peak index), one peak after the other, for every cluster size.  Below the random generators: the
designed cases (one per decision of the definition, each with a witness that the restatement alone must show) and the grid-turn
cases, whose sizes follow from a CU count and whose expected output is gathered from a small library of clusters."""
import functools
import math

import numpy as np

FALLBACK, GLOBAL, CAPACITY = 1, 2, 4


def consensus_cluster(rows, mz, intensity, indptr, medoid, fragment_tol, min_fraction):
    """one cluster: its member rows (ascending) -> (mz f32[], intensity f32[], status)"""
    m = len(rows)
    if m == 1:
        r = int(rows[0])
        return mz[indptr[r]:indptr[r + 1]].copy(), intensity[indptr[r]:indptr[r + 1]].copy(), 0
    if m >= 2:
        cnt = (indptr[rows + 1] - indptr[rows]).astype(np.int64)
        p_row = np.repeat(rows, cnt)
        p_idx = np.concatenate([np.arange(c) for c in cnt]) if len(cnt) else np.zeros(0, np.int64)
        pos = indptr[p_row] + p_idx
        p_mz, p_it = mz[pos], intensity[pos]
        order = np.lexsort((p_idx, p_row, p_mz))              # m/z, then dataset row, then peak index
        xs = p_mz[order].astype(np.float64).tolist()
        ys = p_it[order].astype(np.float64).tolist()
        tol, need = float(fragment_tol), max(1, math.ceil(float(min_fraction) * m))
        out_mz, raws = [], []
        k, n = 0, len(xs)
        while k < n:
            w = mw = ms = 0.0
            count = 0
            j = k
            while True:
                w += ys[j]
                mw += xs[j] * ys[j]
                ms += xs[j]
                count += 1
                j += 1
                if j >= n or xs[j] - xs[j - 1] > tol:
                    break
            if min(count, m) >= need:
                out_mz.append(np.float32(mw / w) if w != 0.0 else np.float32(ms / count))
                raws.append(w / m)
            k = j
        if out_mz:
            norm2 = 0.0
            for r in raws:
                norm2 += r * r
            it = [np.float32(r / math.sqrt(norm2)) if norm2 != 0.0 else np.float32(0.0) for r in raws]
            return np.array(out_mz, np.float32), np.array(it, np.float32), 0
    r = int(medoid)
    if not 0 <= r < len(indptr) - 1:                          # a medoid that is no row of the dataset: nothing to copy
        return np.zeros(0, np.float32), np.zeros(0, np.float32), FALLBACK
    return mz[indptr[r]:indptr[r + 1]].copy(), intensity[indptr[r]:indptr[r + 1]].copy(), FALLBACK


def consensus_reference(mz, intensity, indptr, labels, medoids, fragment_tol, min_fraction, clusters=None):
    """the whole partition -> (indptr i64[n_clusters+1], mz f32, intensity f32, status i32[n_clusters]); `clusters`: only these
    ids (the others come back empty with status 0)"""
    mz, intensity = np.asarray(mz, np.float32), np.asarray(intensity, np.float32)
    indptr, labels, medoids = np.asarray(indptr, np.int64), np.asarray(labels), np.asarray(medoids)
    nc = len(medoids)
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(nc + 1))
    todo = range(nc) if clusters is None else clusters
    res = {}
    for c in todo:
        res[c] = consensus_cluster(order[bounds[c]:bounds[c + 1]], mz, intensity, indptr, medoids[c], fragment_tol, min_fraction)
    out_ptr = np.zeros(nc + 1, np.int64)
    status = np.zeros(nc, np.int32)
    for c, (a, _, st) in res.items():
        out_ptr[c + 1] = len(a)
        status[c] = st
    np.cumsum(out_ptr, out=out_ptr)
    out_mz, out_it = np.zeros(out_ptr[-1], np.float32), np.zeros(out_ptr[-1], np.float32)
    for c, (a, b, _) in res.items():
        out_mz[out_ptr[c]:out_ptr[c + 1]] = a
        out_it[out_ptr[c]:out_ptr[c + 1]] = b
    return out_ptr, out_mz, out_it, status


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- generators --------------------------------------------------------------------------------------------------------------
def make_partition(rng, sizes, peaks=(1, 12), n_template=14, p_empty=0.0, p_zero=0.0, grid_jitter=True, disjoint=False,
                   fixed_peaks=None, shuffle=True, overrides=None):
    """clusters of `sizes` members in one partition, rows in shuffled dataset order -> dict(mz, intensity, indptr, labels, medoids).
    Every cluster has a template of n_template m/z values; a member draws peaks from it (with repeats, so an m/z can occur twice
    inside a member), jittered on a coarse grid (grid_jitter: exact duplicates across members are common) or continuously.
    p_empty: share of members without peaks; p_zero: share of template peaks whose intensity is 0 in every member.
    disjoint: every peak of the partition lies 1 m/z from the next one (no group of two peaks).
    fixed_peaks: every member has exactly this many peaks.  overrides: {cluster: dict(fixed_peaks=, n_template=)}."""
    n = int(np.sum(sizes))
    perm = rng.permutation(n) if shuffle else np.arange(n)
    labels = np.zeros(n, np.int32)
    medoids = np.zeros(len(sizes), np.int32)
    spectra = [None] * n
    off, serial = 0, 0
    for c, m in enumerate(sizes):
        rows = perm[off:off + m]
        off += m
        labels[rows] = c
        medoids[c] = rows[rng.integers(m)]
        own = (overrides or {}).get(c, {})
        n_t, fixed = own.get("n_template", n_template), own.get("fixed_peaks", fixed_peaks)
        t_mz = np.sort(rng.uniform(150.0, 1400.0, n_t))
        t_zero = rng.random(n_t) < p_zero
        for r in rows:
            if fixed is not None:
                k = fixed
            elif rng.random() < p_empty:
                k = 0
            else:
                k = int(rng.integers(peaks[0], peaks[1] + 1))
            pick = rng.integers(0, n_t, k)
            if disjoint:
                x = 150.0 + serial + np.arange(k, dtype=np.float64)
                serial += k
            elif grid_jitter:
                x = t_mz[pick] + rng.integers(-2, 3, k) * 0.01
            else:
                x = t_mz[pick] + rng.normal(0.0, 0.004, k)
            y = rng.uniform(0.1, 1.0, k)
            y[t_zero[pick]] = 0.0
            o = np.argsort(x, kind="stable")
            spectra[r] = (x[o].astype(np.float32), y[o].astype(np.float32))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(s[0]) for s in spectra], out=indptr[1:])
    cat = lambda i: np.concatenate([s[i] for s in spectra]) if n else np.zeros(0, np.float32)
    return dict(mz=cat(0).astype(np.float32), intensity=cat(1).astype(np.float32), indptr=indptr, labels=labels, medoids=medoids)


def permute_rows(part, rng):
    """the same clusters with the dataset rows in another order -> the permuted partition"""
    n = len(part["labels"])
    new_of_old = rng.permutation(n)
    old_of_new = np.argsort(new_of_old)
    ip = part["indptr"]
    cnt = np.diff(ip)[old_of_new]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=indptr[1:])
    pos = np.repeat(ip[old_of_new] - indptr[:-1], cnt) + np.arange(indptr[-1])
    return dict(mz=part["mz"][pos], intensity=part["intensity"][pos], indptr=indptr, labels=part["labels"][old_of_new],
                medoids=new_of_old[part["medoids"]].astype(np.int32))


def template_spectra(seed, n_templates=8, n_spectra=160, n_peaks=40):
    """the generator of the quality property: spectra drawn from templates (15 % of the peaks dropped, m/z jitter sigma 0.002,
    intensity x U(0.7, 1.3), 5 noise peaks), L2-normalised -> dict(mz, intensity, indptr, precursor_mz, retention_time, template)"""
    rng = np.random.default_rng(seed)
    t_mz = np.sort(rng.uniform(150.0, 1400.0, (n_templates, n_peaks)), axis=1)
    t_it = rng.uniform(0.1, 1.0, (n_templates, n_peaks))
    t_pmz = 400.5 + 25.0 * np.arange(n_templates)            # (mid-window: a template does not straddle a 1 m/z precursor window)
    which = rng.integers(0, n_templates, n_spectra)
    mzs, its = [], []
    for t in which:
        keep = rng.random(n_peaks) >= 0.15
        x = t_mz[t][keep] + rng.normal(0.0, 0.002, int(keep.sum()))
        y = t_it[t][keep] * rng.uniform(0.7, 1.3, int(keep.sum()))
        x = np.concatenate([x, rng.uniform(150.0, 1400.0, 5)])
        y = np.concatenate([y, rng.uniform(0.02, 0.3, 5)])
        o = np.argsort(x, kind="stable")
        x, y = x[o].astype(np.float32), y[o].astype(np.float32)
        y = (y / np.sqrt(np.sum(y.astype(np.float64) ** 2))).astype(np.float32)
        mzs.append(x)
        its.append(y)
    indptr = np.zeros(n_spectra + 1, np.int64)
    np.cumsum([len(x) for x in mzs], out=indptr[1:])
    return dict(mz=np.concatenate(mzs), intensity=np.concatenate(its), indptr=indptr,
                precursor_mz=(t_pmz[which] * (1.0 + rng.normal(0.0, 1e-6, n_spectra))).astype(np.float32),
                retention_time=rng.uniform(0.0, 3600.0, n_spectra).astype(np.float32), template=which)


# ---- designed cases ------------------------------------------------------------------------------------------------------------
# A case is dict(part=, tol=, q=, witness=): `witness(ref)` asserts, on the restatement's output alone, that the case reaches the
# decision it was built for (tests/test_consensus_cpu.py runs it, so a case that misses its target fails without a GPU).
F32 = np.float32
CUT = 4096                                                    # FAL_CONS_LDS_PEAKS (the tests check it against the library's)


def up(x, k=1):
    """the k-th float32 above x"""
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(np.inf))
    return x


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def assemble(clusters, medoids=None, stray=(), rng=None):
    """clusters: per id, the members [(mz, intensity), ...] in dataset-row order; medoids: per id a member index of the cluster
    itself (default 0), a pair (cluster, member) anywhere in the partition, "lo" (-1) or "hi" (n); stray: (label, (mz,
    intensity)) rows whose label names no cluster.  rng: the rows of all clusters interleaved at random, every cluster's own
    members keeping their order -> the partition"""
    rows, first = [], {}
    for c, members in enumerate(clusters):
        for k, (x, y) in enumerate(members):
            first[(c, k)] = len(rows)
            rows.append((c, np.asarray(x, F32).reshape(-1), np.asarray(y, F32).reshape(-1)))
    for lab, (x, y) in stray:
        rows.append((lab, np.asarray(x, F32).reshape(-1), np.asarray(y, F32).reshape(-1)))
    n = len(rows)
    lab = np.array([r[0] for r in rows], np.int64)
    place = np.arange(n)
    if rng is not None and n:
        drawn = rng.permutation(n)
        place = np.empty(n, np.int64)
        place[np.argsort(lab, kind="stable")] = drawn[np.lexsort((drawn, lab))]
    at = np.empty(n, np.int64)
    at[place] = np.arange(n)                                  # dataset row -> index into `rows`
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(rows[i][1]) for i in at], out=indptr[1:])
    cat = lambda j: np.concatenate([rows[i][j] for i in at]).astype(F32) if n else np.zeros(0, F32)
    med = np.zeros(len(clusters), np.int32)
    for c in range(len(clusters)):
        want = 0 if medoids is None or medoids[c] is None else medoids[c]
        if want == "lo":
            med[c] = -1
        elif want == "hi":
            med[c] = n
        else:
            med[c] = place[first[want if isinstance(want, tuple) else (c, want)]]
    return dict(mz=cat(1), intensity=cat(2), indptr=indptr, labels=lab[at].astype(np.int32), medoids=med)


def deal(mzs, its, m):
    """peaks dealt to m members in turn (each member's peaks keep the order given) -> the members"""
    mzs, its = np.asarray(mzs, F32), np.asarray(its, F32)
    return [(mzs[k::m], its[k::m]) for k in range(m)]


def pooled_sizes(part):
    """pooled peaks and members of every cluster (labels that name no cluster pool nothing)"""
    nc, lab = len(part["medoids"]), np.asarray(part["labels"], np.int64)
    ok = (lab >= 0) & (lab < nc)
    cnt = np.diff(part["indptr"])
    return np.bincount(lab[ok], weights=cnt[ok], minlength=nc).astype(np.int64), np.bincount(lab[ok], minlength=nc)


def pooled_walk(part, c, tol):
    """cluster c's pooled order cut by the gap rule -> (m/z f32[] in pooled order, group starts, group sizes)"""
    ip = part["indptr"]
    pos = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in np.flatnonzero(part["labels"] == c)] + [np.zeros(0, np.int64)])
    pos = pos.astype(np.int64)
    xs = part["mz"][pos][np.lexsort((pos, part["mz"][pos]))]
    starts = np.flatnonzero(np.concatenate([[True], np.diff(xs.astype(np.float64)) > tol])) if len(xs) else np.zeros(0, np.int64)
    return xs, starts, np.diff(np.append(starts, len(xs)))


def cluster_out(ref, c):
    return ref[1][ref[0][c]:ref[0][c + 1]], ref[2][ref[0][c]:ref[0][c + 1]], int(ref[3][c])


def _case(part, tol, q, witness):
    return dict(part=part, tol=tol, q=q, witness=witness)


def _group_count_witness(part, tol, counts):
    def witness(ref):
        for c, want in enumerate(counts):
            assert len(pooled_walk(part, c, tol)[1]) == want, (c, want)
            assert ref[0][c + 1] - ref[0][c] == want and ref[3][c] == 0, (c, want)        # need = 1: every group is kept
    return witness


def case_gap_dyadic():
    """tol = 2^-4: a gap can equal the tolerance exactly (one group) or exceed it by one float32 ulp (two)"""
    rng, tol = np.random.default_rng(101), 0.0625
    chain = 500.0 + 0.0625 * np.arange(40)
    sets = [([500.0, 500.0625], 1),
            ([500.0, 500.0625, up(500.125)], 2),
            (chain, 1),
            ([511.96875, 512.03125], 1),                                  # the ulp doubles at 512: the difference is still exact
            ([511.96875, up(512.03125)], 2),
            ([down(511.96875), 512.03125], 2),
            (np.concatenate([[100.0, 100.0625, up(100.125)], chain, [511.96875, 512.03125, up(512.09375)]]), 5)]
    clusters = [deal(x, rng.uniform(0.1, 1.0, len(x)), 2 + i % 2) for i, (x, _) in enumerate(sets)]
    part = assemble(clusters, rng=rng)
    count = _group_count_witness(part, tol, [k for _, k in sets])

    def witness(ref):
        count(ref)
        xs, starts, sizes = pooled_walk(part, 2, tol)
        assert sizes.tolist() == [40] and float(xs[-1]) - float(xs[0]) == 2.4375
    return _case(part, tol, 0.01, witness)


def case_gap_005():
    """tol = 0.05 (no float32): the float32 neighbours of 500.05 against 500, float32(0.05) against 0, and the two zeros"""
    rng, tol = np.random.default_rng(102), 0.05
    x = F32(500.05)
    assert float(down(x)) - 500.0 <= tol and float(x) - 500.0 <= tol < float(up(x)) - 500.0
    assert float(F32(0.05)) > tol and not F32(0.05) - F32(0.0) > F32(tol)      # float64 splits; a float32 compare would merge
    sets = [([500.0, down(x)], 1), ([500.0, x], 1), ([500.0, up(x)], 2), ([0.0, F32(0.05)], 2),
            ([-0.0, 0.0], 1), ([0.0, -0.0], 1), ([0.0, -0.0, F32(0.05)], 2), ([-0.0, -0.0], 1)]
    clusters = [deal(v, rng.uniform(0.1, 1.0, len(v)), 2) for v, _ in sets]
    clusters.append([([-0.0, 0.0, -0.0], [0.5, 0.25, 0.0])])                     # one member: its bits are copied, signs included
    part = assemble(clusters, rng=rng)
    count = _group_count_witness(part, tol, [k for _, k in sets])

    def witness(ref):
        count(ref)
        assert bits(cluster_out(ref, 8)[0]).tolist() == bits([-0.0, 0.0, -0.0]).tolist()
    return _case(part, tol, 0.01, witness)


def case_gap_zero():
    """tol = 0: equal m/z merge, one float32 ulp apart splits"""
    rng, tol = np.random.default_rng(103), 0.0
    sets = [([300.0, 300.0], 1), ([300.0, up(300.0)], 2), ([300.0, 300.0, 300.0, up(300.0), up(300.0), up(300.0, 2)], 3),
            ([0.0, -0.0], 1), ([down(512.0), 512.0, up(512.0)], 3), ([700.0] * 9, 1)]
    clusters = [deal(v, rng.uniform(0.1, 1.0, len(v)), 2 + i % 2) for i, (v, _) in enumerate(sets)]
    part = assemble(clusters, rng=rng)
    return _case(part, tol, 0.01, _group_count_witness(part, tol, [k for _, k in sets]))


# (min_fraction, members) -> peaks a group needs; found by search: the double product of the first is 7.000000000000001, a
# float32 product of the second and third gives 16
QUORUM_PAIRS = {0.28: (25, 8), 0.3: (50, 15), 0.6: (25, 15), 0.25: (4, 1), 0.01: (99, 1), 1.0: (7, 7)}


def case_quorum(q):
    """per member count m of (4, 7, 25, 50, 99): groups of 1 .. min(m + 1, 17), m - 1, m and m + 1 peaks at 200 + 10 * size,
    and at 150 one group of more than m peaks that members 0 and 1 alone contribute (support is min(count, m) = m)"""
    rng, tol = np.random.default_rng(104), 0.05
    ms = (4, 7, 25, 50, 99)
    clusters, sizes_of = [], []
    for m in ms:
        sizes = sorted(set(range(1, min(m + 1, 17) + 1)) | {m - 1, m, m + 1})
        members = [([], []) for _ in range(m)]
        for k in range(m + 2):
            members[k % 2][0].append(150.0 + (k % 3) * 0.01)
            members[k % 2][1].append(rng.uniform(0.1, 1.0))
        for s in sizes:
            for k in range(s):
                members[k % m][0].append(200.0 + 10.0 * s + (k % 3) * 0.01)
                members[k % m][1].append(rng.uniform(0.1, 1.0))
        clusters.append(members)
        sizes_of.append(sizes)
    part = assemble(clusters, rng=rng)
    m_pin, need = QUORUM_PAIRS[q]

    def witness(ref):
        c = ms.index(m_pin)
        assert need - 1 in [0] + sizes_of[c] and need in sizes_of[c] and need + 1 in sizes_of[c]
        xs, starts, sizes = pooled_walk(part, c, tol)
        assert sizes.tolist() == [m_pin + 2] + sizes_of[c]                        # the groups are the ones designed
        out = cluster_out(ref, c)
        assert out[2] == 0 and np.round((out[0].astype(np.float64) - 200.0) / 10.0).astype(int).tolist() == \
            [-5] + [s for s in sizes_of[c] if s >= need]
    return _case(part, tol, q, witness)


def case_zero_weight():
    """groups without weight: all intensities 0 (m/z = the plain mean), one float32 denormal among zeros (m/z = the weighted
    mean = that peak's), and clusters whose every kept group is 0"""
    d = F32(1e-45)
    assert 0.0 < float(d) < 1.5e-45
    clusters = [[([300.0, 500.0], [0.0, 1.0]), ([300.03125, 500.0], [0.0, 0.5])],
                [([300.0, 600.0], [0.0, 1.0]), ([300.03125], [d])],
                [([300.0], [0.0]), ([300.03125], [d])],
                [([300.0, 400.0], [0.0, 0.0]), ([300.03125], [0.0])],
                [([300.0, 300.03125, 300.0625], [0.0, 0.0, 0.0]), ([], []), ([300.0], [0.0])]]
    part = assemble(clusters, rng=np.random.default_rng(105))

    def witness(ref):
        assert (ref[3] == 0).all()
        same = lambda a, lit: np.array_equal(bits(a), bits(np.array(lit, F32)))
        assert same(cluster_out(ref, 0)[0], [300.015625, 500.0]) and same(cluster_out(ref, 0)[1], [0.0, 1.0])
        assert same(cluster_out(ref, 1)[0], [300.03125, 600.0]) and same(cluster_out(ref, 1)[1], [d, 1.0])
        assert same(cluster_out(ref, 2)[0], [300.03125]) and same(cluster_out(ref, 2)[1], [1.0])
        assert same(cluster_out(ref, 3)[0], [300.015625, 400.0]) and same(cluster_out(ref, 3)[1], [0.0, 0.0])
        assert same(cluster_out(ref, 4)[0], [300.0234375]) and same(cluster_out(ref, 4)[1], [0.0])
    return _case(part, 0.05, 0.5, witness)


def case_intensity_range():
    """intensities near 1e25 and near 1e-30: raw * raw leaves the float32 range at both ends, the float64 norm does not care"""
    rng = np.random.default_rng(106)
    sizes = [2, 3, 8, 40, 2, 3, 8, 40]
    part = make_partition(rng, sizes, peaks=(2, 9))
    scale = np.where(np.repeat(part["labels"], np.diff(part["indptr"])) < 4, F32(1e25), F32(1e-30)).astype(F32)
    part["intensity"] = (part["intensity"] * scale).astype(F32)

    def witness(ref):
        with np.errstate(over="ignore", under="ignore"):
            big, small = F32(1e24) * F32(1e24), F32(1e-30) * F32(1e-30)
        assert np.isinf(big) and small == 0.0
        for c in range(len(sizes)):
            x, y, st = cluster_out(ref, c)
            assert st == 0 and len(y) and np.isfinite(y).all() and y.max() > 0.0
            assert abs(np.sum(y.astype(np.float64) ** 2) - 1.0) < 1e-5                # L2-normalised
    return _case(part, 0.05, 0.25, witness)


def case_chain_order(cut=CUT):
    """an arithmetic probe of the pooled order with signed intensities: 2^60, -2^60, 1 at one m/z sum to 1 in that order and
    to 0 in the order 2^60, 1, -2^60 (2^60 + 1 rounds to 2^60).  Clusters come in pairs (even id: w = 1, odd id: w = 0), the
    tie broken by dataset row or by peak index inside one member, with k lone peaks below (the tie sits at another place of the
    sort) and once inside more than `cut` pooled peaks"""
    B = 2.0 ** 60
    fill_x = 100.0 + 0.125 * np.arange(2050)
    fill_y = np.linspace(0.5, 1.5, 2050)
    clusters = []
    for k in (0, 1, 2, 3, 5, 8, 13, 29, 61, 250, None):
        lo_x, lo_y = (list(100.0 + np.arange(k)), [1.0] * k) if k is not None else ([], [])
        extra = [] if k is not None else [(fill_x, fill_y), (fill_x, fill_y[::-1])]
        head = (lo_x + [500.0, 700.0], lo_y + [B, 9.0])
        clusters.append([head, ([500.0], [-B]), ([500.0], [1.0])] + extra)          # by row: B, -B, 1
        clusters.append([head, ([500.0], [1.0]), ([500.0], [-B])] + extra)          # by row: B, 1, -B
        clusters.append([(lo_x + [500.0, 500.0, 500.0, 700.0], lo_y + [B, -B, 1.0, 9.0]), ([700.0], [0.0])] + extra)   # by index
        clusters.append([(lo_x + [500.0, 500.0, 500.0, 700.0], lo_y + [B, 1.0, -B, 9.0]), ([700.0], [0.0])] + extra)
    part = assemble(clusters, rng=np.random.default_rng(107))

    def witness(ref):
        pooled, _ = pooled_sizes(part)
        assert (pooled[-4:] > cut).all() and (pooled[:-4] <= cut).all()              # both sort paths
        for c in range(0, len(clusters), 2):
            a, b = cluster_out(ref, c), cluster_out(ref, c + 1)
            assert a[2] == 0 and b[2] == 0 and np.array_equal(a[0], b[0])
            ia, ib = a[1][a[0] == 500.0], b[1][b[0] == 500.0]
            assert len(ia) == 1 and len(ib) == 1 and ia[0] > 0.0 and ib[0] == 0.0, (c, ia, ib)   # the two orders differ
        assert np.allclose(cluster_out(ref, 0)[1], [0.1104, 0.9939], atol=5e-5) and cluster_out(ref, 1)[1].tolist() == [0.0, 1.0]
    return _case(part, 0.05, 0.01, witness)


def case_labels_and_medoids():
    """what the C entry tolerates: labels that name no cluster, ids without a member, medoids that are no row"""
    sp = lambda *x: (list(x), [0.5] * len(x))
    clusters = [[sp(100.0, 200.0), sp(100.03125, 300.0)],       # 0: merged
                [],                                             # 1: no member -> the peaks of its medoid, a row of cluster 0
                [],                                             # 2: no member, medoid -1
                [],                                             # 3: no member, medoid n
                [sp(), sp()],                                   # 4: members without peaks, medoid -1
                [sp(), sp()],                                   # 5: members without peaks, medoid in cluster 0
                [sp()],                                         # 6: one member without peaks
                [sp(150.0, 120.0)],                             # 7: one member (its medoid entry, n, is not looked at)
                [sp(100.0), sp(200.0), sp(300.0)],              # 8: nothing reaches the quorum -> its own medoid
                [sp(100.0), sp(200.0), sp(300.0)],              # 9: the same with medoid n
                [sp(100.0), sp(200.0), sp(300.0)],              # 10: the same with medoid -1
                [sp(400.0, 500.0), sp(400.0), sp(400.03125, 500.0)]]    # 11: merged, the last id
    medoids = [0, (0, 1), "lo", "hi", "lo", (0, 0), 0, "hi", 1, "hi", "lo", 2]
    nc = len(clusters)
    stray = [(lab, sp(100.0, 400.0, 500.0)) for lab in (-1, -1, nc, nc + 5, nc + 5, -2 ** 31, 2 ** 31 - 1)]
    part = assemble(clusters, medoids, stray, rng=np.random.default_rng(108))

    def witness(ref):
        assert np.diff(ref[0]).tolist() == [3, 2, 0, 0, 0, 2, 0, 2, 1, 0, 0, 2]
        assert ref[3].tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0]
        assert cluster_out(ref, 1)[0].tolist() == [100.03125, 300.0] and cluster_out(ref, 5)[0].tolist() == [100.0, 200.0]
        assert cluster_out(ref, 8)[0].tolist() == [200.0] and cluster_out(ref, 11)[0].tolist() == [float(F32(1200.03125 / 3.0)), 500.0]
    return _case(part, 0.05, 0.5, witness)


def case_no_rows():
    """n = 0 with three clusters: every cluster falls back to a medoid that is no row"""
    part = dict(mz=np.zeros(0, F32), intensity=np.zeros(0, F32), indptr=np.zeros(1, np.int64), labels=np.zeros(0, np.int32),
                medoids=np.array([0, -1, 5], np.int32))

    def witness(ref):
        assert ref[0].tolist() == [0, 0, 0, 0] and ref[3].tolist() == [FALLBACK] * 3
    return _case(part, 0.05, 0.25, witness)


def case_no_clusters():
    part = assemble([], stray=[(0, ([100.0], [1.0])), (-1, ([], [])), (2, ([100.0, 200.0], [1.0, 1.0]))])

    def witness(ref):
        assert ref[0].tolist() == [0] and len(ref[1]) == 0 and len(ref[3]) == 0
    return _case(part, 0.05, 0.25, witness)


def tied_members(rng, m, size, n_template=6, empty_last=False, even=False):
    """m members that pool exactly `size` peaks on a grid of n_template m/z x 5 jitter steps: heavy m/z ties (even: every
    member holds size / m peaks, rounded up or down)"""
    t_mz = np.sort(rng.uniform(150.0, 1400.0, n_template))
    x = (t_mz[rng.integers(0, n_template, size)] + rng.integers(-2, 3, size) * 0.01).astype(F32)
    y = rng.uniform(0.1, 1.0, size).astype(F32)
    who = rng.permutation(np.arange(size) % m) if even else rng.integers(0, m - 1 if empty_last and m > 1 else m, size)
    members = []
    for k in range(m):
        o = np.argsort(x[who == k], kind="stable")
        members.append((x[who == k][o], y[who == k][o]))
    return members


LDS_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]


def case_lds_sizes(cut=CUT):
    """clusters of 2 .. 4 members whose pools hold exactly the bitonic padding sizes and the 256-thread strides, +- 1"""
    rng = np.random.default_rng(109)
    clusters = [tied_members(rng, 2 + i % 3, s, empty_last=(i % 4 == 1)) for i, s in enumerate(LDS_SIZES)]
    part = assemble(clusters, rng=rng)

    def witness(ref):
        pooled, members = pooled_sizes(part)
        assert pooled.tolist() == LDS_SIZES and (members >= 2).all() and pooled.max() == cut
        for c in (5, 12, 18):
            assert len(np.unique(pooled_walk(part, c, 0.05)[0])) <= 30                # ties
        assert (ref[3] == 0).sum() >= len(LDS_SIZES) - 3
    return _case(part, 0.05, 0.25, witness)


def _layout_cluster(layout):
    """'L': a lone peak, 'G': two peaks within the tolerance, one per member; 1 m/z from unit to unit -> (members, group starts)"""
    mem, starts, pos = [([], []), ([], [])], [], 0
    for i, unit in enumerate(layout):
        x = 200.0 + i
        if unit == "G":
            starts.append(pos)
            mem[i % 2][0].append(x)
            mem[1 - i % 2][0].append(x + 0.03125)
            mem[0][1].append(0.25 + (i % 7) / 8.0)
            mem[1][1].append(0.5)
            pos += 2
        else:
            mem[i % 2][0].append(x)
            mem[i % 2][1].append(0.75)
            pos += 1
    return mem, starts


EMIT_LAYOUTS = [["L"] * s + ["G"] + ["L"] * 3 for s in (0, 63, 64, 65, 127, 128)] + [
    ["G"] + ["L"] * 61 + ["G"] + ["L"] * 62 + ["G"] + ["L"] * 2,                # starts 0, 63, 127
    ["L"] * 64 + ["G"] + ["L"] * 62 + ["G"] + ["L"],                            # starts 64, 128
    ["G"] * 64, ["G"] * 65, ["G", "L"] * 64, ["L", "G"] * 65,                  # 64 and 65 kept groups
    ["L"] * 70 + ["G", "L"],                                                    # kept only in the last, partial chunk
    ["L"] * 126 + ["G"], ["L"] * 127 + ["G"], ["L"] * 128 + ["G"]]              # the last group ends at / straddles / follows a chunk


def case_emit_chunks():
    """m = 2, q = 1: a group needs two peaks, a lone peak is dropped; the kept groups start at designed pooled positions around
    the 64-lane chunks of the emit kernel's compaction"""
    built = [_layout_cluster(layout) for layout in EMIT_LAYOUTS]
    part = assemble([b[0] for b in built], rng=np.random.default_rng(110))

    def witness(ref):
        for c, (_, want) in enumerate(built):
            xs, starts, sizes = pooled_walk(part, c, 0.05)
            assert starts[sizes >= 2].tolist() == want and sizes.max() == 2, c
            assert ref[0][c + 1] - ref[0][c] == len(want) and ref[3][c] == 0, c
        assert [b[1] for b in built[:8]] == [[0], [63], [64], [65], [127], [128], [0, 63, 127], [64, 128]]
        assert [len(b[1]) for b in built[8:12]] == [64, 65, 64, 65] and built[12][1] == [70]
    return _case(part, 0.05, 1.0, witness)


BIG_IDS = (1, 2, 3, 256, 257)


def case_big_ids(nc, cut=CUT):
    """clusters above the cut (two members of cut / 2 + 1 or more peaks) at id 0 and id nc - 1, two of them side by side, and
    one next to a cluster of exactly `cut` peaks"""
    rng = np.random.default_rng(111 + nc)
    big = lambda extra: tied_members(rng, 2, cut + 2 + extra, n_template=40, even=True)
    exact = lambda: tied_members(rng, 2, cut, n_template=40, even=True)
    if nc == 1:
        clusters, bigs, exacts = [big(0)], [0], []
    elif nc == 2:
        clusters, bigs, exacts = [big(0), big(1)], [0, 1], []
    elif nc == 3:
        clusters, bigs, exacts = [big(0), exact(), big(3)], [0, 2], [1]
    else:
        bigs, exacts = [0, 1, nc // 2, nc - 1], [2, nc - 2]
        clusters = [big(c % 5) if c in bigs else exact() if c in exacts else tied_members(rng, 1 + c % 3, 1 + c % 9)
                    for c in range(nc)]
    part = assemble(clusters, rng=rng)

    def witness(ref):
        pooled, members = pooled_sizes(part)
        assert np.flatnonzero((pooled > cut) & (members > 1)).tolist() == bigs
        assert np.flatnonzero(pooled == cut).tolist() == exacts
        assert all(np.diff(part["indptr"])[part["labels"] == c].min() >= cut // 2 + 1 for c in bigs)
        assert (ref[3][bigs] == 0).all()
    return _case(part, 0.05, 0.25, witness)


DECISION_CASES = {
    "gap_dyadic": case_gap_dyadic, "gap_0.05": case_gap_005, "gap_zero": case_gap_zero,
    **{f"quorum_q{q}": (lambda q=q: case_quorum(q)) for q in QUORUM_PAIRS},
    "zero_weight": case_zero_weight, "intensity_range": case_intensity_range, "chain_order": case_chain_order,
    "labels_and_medoids": case_labels_and_medoids, "no_rows": case_no_rows, "no_clusters": case_no_clusters,
    "lds_sizes": case_lds_sizes, "emit_chunks": case_emit_chunks,
    **{f"big_ids_{nc}": (lambda nc=nc: case_big_ids(nc)) for nc in BIG_IDS},
}


# ---- grid-turn cases -----------------------------------------------------------------------------------------------------------
# Sizes follow from the device's CU count, restated from fal_consensus_spectra's host code:
#   cons_sort_lds_kernel  min(n_clusters, cus * 40) workgroups, one cluster per workgroup and turn
#   cons_emit_kernel      min(ceil(n_clusters / 4), cus * 16) blocks of four waves, one cluster per wave and turn: cus * 64
#   every flat kernel     min(ceil(items / 256), cus * 16) blocks of 256: cus * 4096 items per turn
# The restatement runs on a small LIBRARY of clusters; a case draws its clusters from the library and gathers its expected
# output from the library's the same way.
def csr_gather(indptr, pick, *arrays):
    """segments `pick` (any order, repeats allowed) of a CSR -> (new indptr, the arrays' gathered values)"""
    indptr, pick = np.asarray(indptr, np.int64), np.asarray(pick, np.int64)
    counts = np.diff(indptr)[pick]
    ip = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos = np.repeat(indptr[:-1][pick] - ip[:-1], counts) + np.arange(ip[-1])
    return (ip,) + tuple(np.asarray(a)[pos] for a in arrays)


def gather_partition(lib, pick, rng):
    """the partition whose cluster j is a copy of library cluster pick[j] (members in the library's order, rows of all
    clusters interleaved at random).  A library medoid outside its own cluster points to the copy inside the first cluster of
    the case drawn from the medoid's cluster."""
    pick = np.asarray(pick, np.int64)
    lab, n_lib = np.asarray(lib["labels"], np.int64), len(lib["labels"])
    l_order = np.argsort(lab, kind="stable")
    l_start = np.searchsorted(lab[l_order], np.arange(len(lib["medoids"]) + 1))
    rank = np.empty(n_lib, np.int64)
    rank[l_order] = np.arange(n_lib) - l_start[lab[l_order]]                 # library row -> its place among its cluster's members
    sizes = np.diff(l_start)[pick]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(start[-1])
    labels_cm = np.repeat(np.arange(len(pick)), sizes)
    src = l_order[np.repeat(l_start[pick] - start[:-1], sizes) + np.arange(n)]     # cluster-major: the library row copied
    drawn = rng.permutation(n)
    place = drawn[np.lexsort((drawn, labels_cm))]                            # cluster-major index -> dataset row
    at = np.empty(n, np.int64)
    at[place] = np.arange(n)
    indptr, mz, it = csr_gather(lib["indptr"], src[at], lib["mz"], lib["intensity"])
    first_use = np.full(len(lib["medoids"]), -1, np.int64)
    first_use[pick[::-1]] = np.arange(len(pick))[::-1]
    med = np.asarray(lib["medoids"], np.int64)[pick]
    inside = (med >= 0) & (med < n_lib)
    owner = lab[np.where(inside, med, 0)]
    home = np.where(owner == pick, np.arange(len(pick)), first_use[owner])
    assert (home[inside] >= 0).all(), "a medoid's cluster is not part of the case"
    medoids = np.where(inside, place[np.minimum(start[:-1][home] + rank[np.where(inside, med, 0)], max(n - 1, 0))],
                       np.where(med < 0, -1, n))
    return dict(mz=mz.astype(F32), intensity=it.astype(F32), indptr=indptr, labels=labels_cm[at].astype(np.int32),
                medoids=medoids.astype(np.int32))


def gather_expected(lib_ref, pick):
    """the case's expected output from the restatement's on the library"""
    ptr, mz, it = csr_gather(lib_ref[0], pick, lib_ref[1], lib_ref[2])
    return ptr, mz.astype(F32), it.astype(F32), lib_ref[3][np.asarray(pick, np.int64)].astype(np.int32)


def _library(kinds, medoids=None, seed=0):
    """kinds: name -> list of clusters (member lists) -> (the library partition, name -> library cluster ids)"""
    clusters, ids, med = [], {}, []
    for name, group in kinds.items():
        ids[name] = list(range(len(clusters), len(clusters) + len(group)))
        clusters += group
        med += (medoids or {}).get(name, [None] * len(group))
    return assemble(clusters, med, rng=np.random.default_rng(seed)), ids


@functools.lru_cache(maxsize=None)
def lds_turns_library():
    rng = np.random.default_rng(201)
    kinds = {
        "single": [tied_members(rng, 1, 5), tied_members(rng, 1, 1)],
        "large": [tied_members(rng, 2 + i % 2, s) for i, s in enumerate((300, 301, 320, 513))],
        "tiny": [tied_members(rng, 2, 2), tied_members(rng, 2, 3), tied_members(rng, 3, 3, empty_last=True)],
        "medium": [tied_members(rng, 2 + i % 3, s) for i, s in enumerate((40, 64, 65, 100))],
        "nomember": [[], []],
        "nopeaks": [[([], []), ([], [])], [([], []), ([], []), ([], [])]],
    }
    return _library(kinds, {"nomember": [(0, 0), (1, 0)]}, seed=202)


def lds_turns(num_cus):
    """-> (partition, library cluster of every cluster, conditions): more than two turns of cons_sort_lds_kernel's workgroups
    (and more than one of the emit waves).  Workgroup b sorts clusters b, b + wgs, b + 2 wgs: a large pool, then a tiny one, then
    a medium one for the workgroups that reach a third, with skipped clusters (one member, no member, no peaks) in between and
    at every place of the sequence for the others"""
    lib, ids = lds_turns_library()
    wgs, nc = num_cus * 40, 2 * num_cus * 40 + 13
    turn0 = ["large", "single", "nomember", "medium", "medium", "nopeaks", "tiny", "medium"]
    turn1 = ["tiny", "medium", "tiny", "nopeaks", "large", "medium", "medium", "tiny"]
    kind = []
    for c in range(nc):
        b, turn = c % wgs, c // wgs
        if b < 13:                      # the workgroups with three turns: large, tiny / skipped, medium / tiny
            kind.append(("large", ("tiny", "single", "tiny", "nomember", "tiny", "nopeaks")[b % 6], ("medium", "tiny")[b % 2])[turn])
        else:
            kind.append((turn0, turn1)[turn][b % 8])
    pick = np.array([ids[k][(c // 8 + c // wgs) % len(ids[k])] for c, k in enumerate(kind)], np.int64)
    pick[:2] = ids["single"]                                    # (the medoids of the clusters without a member live here)
    part = gather_partition(lib, pick, np.random.default_rng(203))
    pooled, members = pooled_sizes(part)
    sorts = (members >= 2) & (pooled >= 1)
    cond = dict(lds_turns=nc > 2 * wgs, emit_turns=nc > num_cus * 64, pooled_under_2M=int(pooled.sum()) < 2_000_000,
                no_big=int(pooled.max()) <= CUT,
                large_tiny_medium=all(pooled[b] >= 300 and 2 <= pooled[b + wgs] <= 3 and 40 <= pooled[b + 2 * wgs] <= 100
                                      and sorts[[b, b + wgs, b + 2 * wgs]].all() for b in (2, 4, 6, 8, 10, 12)),
                skipped_between=all(pooled[b] >= 300 and not sorts[b + wgs] and sorts[b + 2 * wgs] for b in (3, 5, 7, 9, 11)),
                second_sorts=int((sorts[:wgs] & sorts[wgs:2 * wgs]).sum()) > wgs // 4,
                skip_then_sort=int((~sorts[:wgs] & sorts[wgs:2 * wgs]).sum()) > wgs // 8)
    return part, pick, cond


@functools.lru_cache(maxsize=None)
def flat_turns_library(cut=CUT):
    rng = np.random.default_rng(301)
    kinds = {
        "peak": [([(x, y)]) for x, y in [([200.0], [1.0]), ([300.5], [0.25]), ([-0.0], [0.5]), ([1400.0], [0.0]), ([700.25], [3.0])]],
        "empty": [[([], [])]],
        "three": [tied_members(rng, 1, 3)],
        "pair": [tied_members(rng, 2, 3), tied_members(rng, 2, 7)],
        "nomember": [[]],
        "big": [tied_members(rng, 2, cut + 2 + e, n_template=40, even=True) for e in (0, 1, 5)],
    }
    return _library(kinds, {"nomember": [(0, 0)]}, seed=302)


def flat_turns(num_cus, cut=CUT):
    """-> (partition, library cluster of every cluster, conditions): more than one turn of every flat kernel's grid -- over the
    rows, the clusters, the pooled peaks and the peaks of the device-wide sort"""
    lib, ids = flat_turns_library(cut)
    T = num_cus * 4096
    nc = T + 37
    n_big = T // (cut + 2) + 2
    c = np.arange(nc)
    pick = np.asarray(ids["peak"], np.int64)[c % len(ids["peak"])]
    for slot, name in ((0, "pair"), (1, "empty"), (2, "nomember"), (3, "three")):
        sel = c[c % 64 == slot]
        pick[sel] = np.asarray(ids[name], np.int64)[(sel // 64) % len(ids[name])]
    at = np.unique(np.concatenate([[1, nc - 1], np.linspace(5, nc - 2, n_big - 2).astype(np.int64)]))
    pick[at] = np.asarray(ids["big"], np.int64)[np.arange(len(at)) % len(ids["big"])]
    pick[0] = ids["peak"][0]                                    # (the medoid of the clusters without a member lives here)
    part = gather_partition(lib, pick, np.random.default_rng(303))
    pooled, members = pooled_sizes(part)
    big = (pooled > cut) & (members > 1)
    cond = dict(rows=len(part["labels"]) > T, clusters=nc > T, pooled=int(pooled.sum()) > T, big_peaks=int(pooled[big].sum()) > T,
                big_at_the_end=bool(big[nc - 1]), peaks_31_bits=len(part["mz"]) < 2 ** 31)
    return part, pick, cond
