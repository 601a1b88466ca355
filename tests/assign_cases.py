"""Nearest-representative search (`fal_assign_nearest`, DESIGN.md "Assigning to representatives"): the numpy restatement of the
rule -- the only oracle of tests/test_assign_cpu.py and tests/test_gpu_assign.py -- and the generators of their cases.

A side (queries or library) is a dict: mz f32[nnz], intensity f32[nnz], indptr i64[n+1], precursor_mz f32[n], retention_time
f32[n]."""
import numpy as np

from oracle import falcon_oracle as fo
from tests import peakmatch_cases as pc

f32, f64 = np.float32, np.float64


def side(mzs, its, pmz, rt=None):
    """lists of per-spectrum peak arrays -> a side"""
    n = len(mzs)
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in mzs])]).astype(np.int64)
    cat = lambda xs: np.concatenate([np.asarray(x, f32) for x in xs]).astype(f32) if n else np.zeros(0, f32)
    return dict(mz=cat(mzs), intensity=cat(its), indptr=indptr, precursor_mz=np.asarray(pmz, f32).reshape(n),
                retention_time=np.zeros(n, f32) if rt is None else np.asarray(rt, f32).reshape(n))


def take(d, rows):
    rows = np.asarray(rows, np.int64)
    return side([peaks(d, r)[0] for r in rows], [peaks(d, r)[1] for r in rows], d["precursor_mz"][rows], d["retention_time"][rows])


def concat(a, b):
    na, nb = len(a["precursor_mz"]), len(b["precursor_mz"])
    return side([peaks(a, r)[0] for r in range(na)] + [peaks(b, r)[0] for r in range(nb)],
                [peaks(a, r)[1] for r in range(na)] + [peaks(b, r)[1] for r in range(nb)],
                np.concatenate([a["precursor_mz"], b["precursor_mz"]]), np.concatenate([a["retention_time"], b["retention_time"]]))


def peaks(d, r):
    a, b = d["indptr"][r], d["indptr"][r + 1]
    return d["mz"][a:b], d["intensity"][a:b]


def is_candidate(q_pmz, l_pmz, tol, mode, rt_tol=None, q_rt=None, l_rt=None):
    """the per-pair test: mass_diff(query, library) against the tolerance, the float32 RT difference against rt_tol"""
    ok = abs(float(fo.mass_diff(f32(q_pmz), f32(l_pmz), mode == "Da"))) <= tol
    if ok and rt_tol is not None:
        ok = f64(abs(f32(f32(q_rt) - f32(l_rt)))) <= rt_tol
    return bool(ok)


def pair_dist(q, i, l, j, fragment_tol, min_matches):
    """float32(1 - cosine_fast(query, library)), 1 below min_matches"""
    sim, nm = fo.cosine_fast(*peaks(q, i), *peaks(l, j), fragment_tol)
    if nm < min_matches:
        sim = 0.0
    return f32(1.0 - sim)


def assign_ref(q, l, tol, mode, rt_tol, fragment_tol, min_matches, stats=None):
    """brute force over all (query, library) pairs -> best_row i32[nq], best_dist f32[nq], n_cand i32[nq].
    `stats` (a dict) receives: pairs (candidates), solver_pairs (candidates with a component of two or more query peaks),
    solver_winners (queries whose winner is such a pair), max_component."""
    nq, nl = len(q["precursor_mz"]), len(l["precursor_mz"])
    best_row, best_dist, n_cand = np.full(nq, -1, np.int32), np.ones(nq, f32), np.zeros(nq, np.int32)
    pairs = solver_pairs = solver_winners = max_comp = 0
    for i in range(nq):
        rows, dist, multi = [], [], []
        for j in range(nl):
            if not is_candidate(q["precursor_mz"][i], l["precursor_mz"][j], tol, mode, rt_tol, q["retention_time"][i],
                                l["retention_time"][j]):
                continue
            rows.append(j)
            dist.append(pair_dist(q, i, l, j, fragment_tol, min_matches))
            if stats is not None:
                comps = pc.components(peaks(q, i)[0], peaks(l, j)[0], fragment_tol)
                multi.append(any(a >= 2 for a, _ in comps))
                max_comp = max([max_comp] + [max(a, b) for a, b in comps])
        n_cand[i] = len(rows)
        if rows:
            rows, dist = np.asarray(rows), np.asarray(dist, f32)
            w = np.lexsort((rows, l["precursor_mz"][rows], dist))[0]
            best_row[i], best_dist[i] = rows[w], dist[w]
            if stats is not None:
                pairs += len(rows)
                solver_pairs += int(np.sum(multi))
                solver_winners += int(multi[w])
    if stats is not None:
        stats.update(pairs=pairs, solver_pairs=solver_pairs, solver_winners=solver_winners, max_component=max_comp)
    return best_row, best_dist, n_cand


# ---- generators --------------------------------------------------------------------------------------------------------------
def template_spectra(n_templates=6, per=110, pmz_centres=(500, 520, 640, 700), seed=3, jitter=0.002, chained=8, n_peaks=40,
                     drop=0.15, it_noise=0.2):
    """the generator of tests/test_gpu_exact.py `_spectra`, restated: spectra drawn around peak templates (jittered m/z, a `drop`
    share of the peaks left out, the template's intensities times 1 +- it_noise, L2-normalised) + `chained` spectra per bucket
    whose peaks sit closer than the fragment tolerance (components of several peaks: the solver)"""
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
            mz.append(m[o].astype(f32))
            if it_noise is None:
                it.append(rng.uniform(0.1, 1.0, len(m)).astype(f32))
            else:
                it.append((t_it[ti][keep] * rng.uniform(1 - it_noise, 1 + it_noise, len(m)))[o].astype(f32))
            pmz.append(centre + rng.uniform(-0.002, 0.002))
        for _ in range(chained):
            base = rng.uniform(300, 900)
            m = np.sort(np.concatenate([base + 0.03 * np.arange(6) + rng.normal(0, 0.002, 6), rng.uniform(150, 1400, 10)]))
            mz.append(m.astype(f32))
            it.append(rng.uniform(0.1, 1.0, len(m)).astype(f32))
            pmz.append(centre + rng.uniform(-0.002, 0.002))
    it = [x / np.sqrt(np.sum(x.astype(f64) ** 2)).astype(f32) for x in it]
    perm = rng.permutation(len(mz))                          # dataset order != precursor order
    mz, it, pmz = [mz[i] for i in perm], [it[i] for i in perm], np.asarray(pmz, f32)[perm]
    return side(mz, it, pmz, rng.uniform(0, 100, len(pmz)).astype(f32))


def template_split():
    """the 472 template spectra split into 236 queries and 236 library rows -> (queries, library)"""
    d = template_spectra()
    perm = np.random.default_rng(1).permutation(len(d["precursor_mz"]))
    half = len(perm) // 2
    return take(d, perm[:half]), take(d, perm[half:])


TEMPLATE_PARAMS = {            # name -> (tol, mode, rt_tol, fragment_tol, min_matches)
    "ppm20": (20.0, "ppm", None, 0.05, 0),
    "da005": (0.05, "Da", None, 0.5, 3),
    "ppm20_rt50": (20.0, "ppm", 50.0, 0.05, 0),
}


def small_templates(rng, n_peaks=8):
    return [(np.sort(rng.uniform(150, 1400, n_peaks)), rng.uniform(0.1, 1.0, n_peaks)) for _ in range(4)]


def small_spectra(n, rng, temps=None, n_peaks=8):
    """n spectra of `n_peaks` peaks drawn from 4 templates (jittered m/z, intensities times 1 +- 0.3: distances differ, few
    are 1), L2-normalised"""
    temps = temps or small_templates(rng, n_peaks)
    mzs, its = [], []
    for _ in range(n):
        t_mz, t_it = temps[rng.integers(4)]
        m = np.sort(t_mz + rng.normal(0, 0.002, n_peaks)).astype(f32)
        x = t_it * rng.uniform(0.7, 1.3, n_peaks)
        mzs.append(m)
        its.append((x / np.sqrt(np.sum(x ** 2))).astype(f32))
    return mzs, its


def ulp_bounds(l_pmz, tol, mode):
    """the four float32 precursors at the edges of the candidate range of library precursor l_pmz: (below: last outside, first
    inside; above: last inside, first outside), found by stepping float32 values against the per-pair test itself"""
    l_pmz = f32(l_pmz)

    def edge(direction):
        x = l_pmz
        while is_candidate(x, l_pmz, tol, mode):
            x = np.nextafter(x, f32(direction), dtype=f32)
        return np.nextafter(x, l_pmz, dtype=f32), x            # (last inside, first outside)
    lo_in, lo_out = edge(-np.inf)
    hi_in, hi_out = edge(np.inf)
    return lo_out, lo_in, hi_in, hi_out


def ladder_case(nq, nl, seed=0, tol=20.0, mode="ppm"):
    """library precursors on a 5 ppm ladder from m/z 600 (a 20 ppm window holds about 8 rows), shuffled rows; queries spread
    over the ladder, plus (when there is room) queries below the first rung, above the last rung and exactly on the +- 1 ulp
    bounds of a rung -> (queries, library)"""
    rng = np.random.default_rng(1000 * nq + nl + seed)
    l_pmz = (600.0 * (1.0 + 5e-6) ** np.arange(nl)).astype(f32)
    temps = small_templates(rng)
    lm, li = small_spectra(nl, rng, temps)
    perm = rng.permutation(nl)
    lib = side([lm[i] for i in perm], [li[i] for i in perm], l_pmz[perm], rng.uniform(0, 100, nl).astype(f32))
    q_pmz = rng.uniform(l_pmz[0] * (1 - 30e-6), l_pmz[-1] * (1 + 30e-6), nq).astype(f32) if nl else \
        rng.uniform(599.9, 600.1, nq).astype(f32)
    if nl:
        special = [l_pmz[0] * f32(1 - 100e-6), l_pmz[-1] * f32(1 + 100e-6), *ulp_bounds(l_pmz[nl // 2], tol, mode)]
        for k, v in enumerate(special[:max(0, nq - 1)]):
            q_pmz[k] = v
    qm, qi = small_spectra(nq, rng, temps)
    if nl and nq:
        qm[-1], qi[-1] = lm[0], li[0]                       # one exact copy of a library spectrum
    return side(qm, qi, q_pmz, rng.uniform(0, 100, nq).astype(f32)), lib


def tie_case(seed=5):
    """the library holds three byte-identical copies of 20 spectra -- one group of copies at equal precursors, one at precursors
    a few ppm apart -- in shuffled row order; the queries are copies of those 20 -> (queries, library)"""
    rng = np.random.default_rng(seed)
    m, it = small_spectra(20, rng)
    base = (600.0 + 0.5 * np.arange(20)).astype(f32)
    mzs, its, pmz = [], [], []
    for s in range(20):
        for c in range(3):
            mzs.append(m[s])
            its.append(it[s])
            pmz.append(base[s] if s % 2 == 0 else f32(base[s] * (1 + (c - 1) * 3e-6)))
    perm = rng.permutation(len(mzs))
    lib = side([mzs[i] for i in perm], [its[i] for i in perm], np.asarray(pmz, f32)[perm])
    return side(m, it, base), lib


def overflow_case(q_peaks, l_peaks, n=64, seed=9):
    """n + n spectra of q_peaks / l_peaks peaks each around shared templates (more than 3,200 staged peaks a side at 64 x 120:
    that side is read from global memory) -> (queries, library)"""
    rng = np.random.default_rng(seed)
    temps = [np.sort(rng.uniform(150, 1400, 120)) for _ in range(3)]

    def draw(k):
        mzs, its = [], []
        for _ in range(n):
            t = temps[rng.integers(3)]
            keep = np.sort(rng.choice(120, k, replace=False))
            mzs.append(np.sort(t[keep] + rng.normal(0, 0.002, k)).astype(f32))
            x = rng.uniform(0.1, 1.0, k)
            its.append((x / np.sqrt(np.sum(x ** 2))).astype(f32))
        return mzs, its
    qm, qi = draw(q_peaks)
    lm, li = draw(l_peaks)
    return (side(qm, qi, rng.uniform(700.0, 700.004, n).astype(f32)), side(lm, li, rng.uniform(700.0, 700.004, n).astype(f32)))


def unsupported_case(inside):
    """peakmatch_cases.exact_pair(33) (a 33 x 33 component: beyond the solver) as query and library spectrum among ordinary ones,
    inside one precursor window or far outside every window -> (queries, library, fragment_tol)"""
    rng = np.random.default_rng(33)
    mz_a, it_a, mz_b, it_b, tol = pc.exact_pair(33)
    qm, qi = small_spectra(5, rng)
    lm, li = small_spectra(5, rng)
    q = side(qm + [mz_a], qi + [it_a], [600.0] * 5 + [650.0])
    lib = side(lm + [mz_b], li + [it_b], [600.0] * 5 + [650.0 if inside else 800.0])
    return q, lib, tol
