"""Consensus representatives: the numpy restatement of the definition (DESIGN.md "Consensus representatives") and the case
generators of the CPU and GPU tests.  The restatement is a plain loop over clusters, groups and peaks: float64 sums in pooled
order (m/z, dataset row, peak index), one peak after the other, for every cluster size."""
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
