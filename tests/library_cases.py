"""Library search (`fal_library_search`; DESIGN.md "Library search"): the numpy restatement of the rule -- scope in its two modes,
orientation, candidates, greedy matching, score, hit rule, top-n -- and the case generators of the CPU and GPU tests.

A side (queries or library) is a dict as tests/network_cases.py's nodes: mz, intensity f32[nnz], indptr i64[n_rows + 1], rows
i32[n], precursor_mz f32[n]; the two sides have peak CSRs of their own.  A rule is a dict: analog, precursor_tol, tol_is_da,
max_shift.  Everything behind the orientation is network_cases' (`pair_ref`, `greedy`, `similarity`, `is_edge`)."""
import functools

import numpy as np

from tests import network_cases as nc

f32, f64 = np.float32, np.float64


def rule(analog, precursor_tol=20.0, tol_is_da=False, max_shift=200.0):
    return dict(analog=bool(analog), precursor_tol=float(precursor_tol), tol_is_da=bool(tol_is_da), max_shift=float(max_shift))


def as_candidate(pq, pl, tol, is_da):
    """csrc/assignrep.h as_candidate without a retention-time rule: float32 difference and division, float64 product"""
    diff = f32(f32(pq) - f32(pl))
    md = f64(diff) if is_da else f64(f32(diff / f32(pl))) * 1e6
    return bool(abs(md) <= tol)


def in_scope(pq, pl, r):
    return nc.in_scope(pq, pl, r["max_shift"]) if r["analog"] else as_candidate(pq, pl, r["precursor_tol"], r["tol_is_da"])


def query_is_a(pq, pl):
    return bool(f32(pq) <= f32(pl))


# ---- the search ----------------------------------------------------------------------------------------------------------------
def score_pairs(q, l, fragment_tol, r):
    """every (query, library) pair in scope, scored in its orientation -> list of nc.pair_ref dicts with q, l (indices), qa (the
    query is the pair's a) and delta = float32(pmz_query - pmz_library)"""
    pq, pl = np.asarray(q["precursor_mz"], f32), np.asarray(l["precursor_mz"], f32)
    out = []
    for x in range(len(pq)):
        for y in range(len(pl)):
            if not in_scope(pq[x], pl[y], r):
                continue
            sq, sl = nc.peaks(q, x), nc.peaks(l, y)
            if len(sq[0]) > nc.MAX_PEAKS or len(sl[0]) > nc.MAX_PEAKS:
                raise nc.Unsupported((x, y))
            qa = query_is_a(pq[x], pl[y])
            (a, pa), (b, pb) = ((sq, pq[x]), (sl, pl[y])) if qa else ((sl, pl[y]), (sq, pq[x]))
            shift = f32(pa - pb) if r["analog"] else f32(0.0)
            assert shift <= 0
            p = nc.pair_ref(*a, *b, shift, fragment_tol)
            p.update(q=x, l=y, qa=qa, delta=f32(pq[x] - pl[y]))
            out.append(p)
    return out


def hits_from(scored, min_cosine, min_matched, top_n, stats=None):
    """the thresholds and the top-n over `score_pairs`' records -> (query i32, library i32, sim f32, matched i32) in (query, rank)
    order: a query's hits by (sim descending, library ascending), the first top_n of them (0: all)"""
    hits = [p for p in scored if nc.is_edge(p["sim"], p["matched"], min_cosine, min_matched)]
    hits.sort(key=lambda p: (p["q"], -float(p["sim"]), p["l"]))
    kept, seen = [], {}
    for p in hits:
        rank = seen.get(p["q"], 0)
        seen[p["q"]] = rank + 1
        if top_n <= 0 or rank < top_n:
            kept.append(p)
    if stats is not None:
        kinds = [nc.classify(p, min_matched) for p in scored]
        stats.update(in_scope=len(scored), rejected_cardinality=kinds.count(nc.REJECT), greedy_pairs=kinds.count(nc.GREEDY),
                     refused_pairs=sum(bool(p["refused"]) for p in scored), hits_before_top_n=len(hits), hits=len(kept),
                     query_is_a=sum(p["qa"] for p in scored), library_is_a=sum(not p["qa"] for p in scored),
                     hits_below=sum(p["delta"] < -1.0 for p in kept), hits_above=sum(p["delta"] > 1.0 for p in kept),
                     hits_near=sum(abs(p["delta"]) <= 1.0 for p in kept))
    col = lambda k, t: np.array([p[k] for p in kept], t)
    return col("q", np.int32), col("l", np.int32), col("sim", f32), col("matched", np.int32)


def search_ref(q, l, fragment_tol, r, min_cosine, min_matched, top_n, stats=None):
    return hits_from(score_pairs(q, l, fragment_tol, r), min_cosine, min_matched, top_n, stats)


def same_hits(got, want):
    return len(got) == 4 and all(nc.same(g, w) for g, w in zip(got, want))


def permute_side(side, perm):
    """the same CSR, new entry v = old entry perm[v]"""
    return nc.permute_nodes(side, perm)


def map_back(hits, q_perm, l_perm):
    """hits of (permute_side(q, q_perm), permute_side(l, l_perm)) in the indices of (q, l), in (query, rank) order again: the rank
    inside a query is (sim descending, library ascending)"""
    qq, ll = q_perm[hits[0]].astype(np.int32), l_perm[hits[1]].astype(np.int32)
    o = np.lexsort((ll, -hits[2].astype(f64), qq))
    return qq[o], ll[o], hits[2][o], hits[3][o]


# ---- generators ----------------------------------------------------------------------------------------------------------------
def repack(nodes, idx, seed):
    """the entries `idx` of `nodes` as a side with a peak CSR of its own (shuffled rows between spare ones)"""
    idx = np.asarray(idx)
    return nc.make_nodes([nc.peaks(nodes, int(v)) for v in idx], np.asarray(nodes["precursor_mz"], f32)[idx], np.random.default_rng(seed))


ANALOGUE = dict(nc.ANALOGUE)


@functools.lru_cache(maxsize=None)
def analogue_case():
    """nc.analogue_case() split by node parity: the library's precursors lie below and above the queries' -> (queries, library)"""
    nodes = nc.analogue_case()
    n = len(nodes["rows"])
    return repack(nodes, np.arange(0, n, 2), 21), repack(nodes, np.arange(1, n, 2), 22)


TILE_NQ, TILE_NL = (1, 63, 64, 65, 130), (1, 64, 65, 130)
TILE_BANDS = nc.TILE_BANDS


@functools.lru_cache(maxsize=None)
def tile_case(nq, nl, band):
    """nq queries against nl library spectra out of one nc.tile_case (one pool of m/z values; thresholds 0 / 0 make every pair
    with a common peak a hit), dealt to the sides at random -> (queries, library, max_shift)"""
    nodes, max_shift = nc.tile_case(nq + nl, band, seed=3 + nq)
    perm = np.random.default_rng(1000 * nq + nl).permutation(nq + nl)
    return repack(nodes, perm[:nq], 31), repack(nodes, perm[nq:], 32), max_shift


def scope_ends(pq, r):
    """the float32 library precursors at the ends of a query precursor's scope: (first outside below, first inside, last inside,
    first outside above), by stepping against the test"""
    width = r["max_shift"] if r["analog"] else (r["precursor_tol"] if r["tol_is_da"] else float(pq) * r["precursor_tol"] * 1e-6)
    out = []
    for sign in (-1.0, 1.0):
        away = f32(sign * np.inf)
        x = f32(f64(pq) + sign * width)
        while in_scope(pq, x, r):
            x = np.nextafter(x, away, dtype=f32)
        while not in_scope(pq, x, r):
            x = np.nextafter(x, -away, dtype=f32)
        out.append((x, np.nextafter(x, away, dtype=f32)))
    (lo_in, lo_out), (hi_in, hi_out) = out
    assert in_scope(pq, lo_in, r) and in_scope(pq, hi_in, r) and not in_scope(pq, lo_out, r) and not in_scope(pq, hi_out, r)
    return lo_out, lo_in, hi_in, hi_out


ULP_RULES = dict(analog=rule(True, max_shift=37.3), ppm=rule(False, 20.0, False), da=rule(False, 0.731, True))


@functools.lru_cache(maxsize=None)
def ulp_case(mode, seed=5):
    """three queries at one precursor p0 and one a float32 step below it; the library: 70 entries at p0, three each at the last
    precursor inside p0's scope and at the first outside, on both sides, and ten each far below and far above.  In sorted order
    the range of the queries' tile begins behind the far-below entries and ends, 82 or so positions on, inside its second chunk.
    Every spectrum is the same: every pair in scope is a hit at thresholds 0 / 0 -> (queries, library, rule)"""
    r = ULP_RULES[mode]
    rng = np.random.default_rng(seed)
    p0 = f32(500.0)
    lo_out, lo_in, hi_in, hi_out = scope_ends(p0, r)
    s = nc.spectrum(np.sort(rng.uniform(150.0, 450.0, 8)), rng.uniform(0.2, 1.0, 8))
    lp = np.array([300.0] * 10 + [lo_out] * 3 + [lo_in] * 3 + [p0] * 70 + [hi_in] * 3 + [hi_out] * 3 + [800.0] * 10, f32)
    qp = np.array([p0] * 3 + [np.nextafter(p0, f32(0))], f32)
    l = nc.make_nodes([s] * len(lp), lp, rng)
    q = nc.make_nodes([s] * len(qp), qp, rng)
    return q, permute_side(l, rng.permutation(len(lp))), r


@functools.lru_cache(maxsize=None)
def tie_case():
    """nc.tie_case()'s spectra on both sides (six byte-identical ones at one precursor among others): equal similarities (the rank
    goes to the lower library index) and equal precursors (the query is a) -> (queries, library)"""
    nodes = nc.tie_case()
    n = len(nodes["rows"])
    return repack(nodes, np.arange(n), 41), repack(nodes, np.random.default_rng(42).permutation(n), 43)


@functools.lru_cache(maxsize=None)
def strip_case():
    """nc.strip_case() (sides of 200 peaks, conflicts in every pair) split by parity -> (queries, library)"""
    nodes = nc.strip_case()
    n = len(nodes["rows"])
    return repack(nodes, np.arange(0, n, 2), 51), repack(nodes, np.arange(1, n, 2), 52)


LDS_SIDES = ("query", "library", "both")


@functools.lru_cache(maxsize=None)
def lds_case(which):
    """nc.lds_case()'s 70 spectra of 60 peaks (a tile side of 64 of them is above the 3,200 staged peaks) on the query side, on
    the library side, or on both; the other side has 20 of them -> (queries, library)"""
    nodes = nc.lds_case()
    big, few = np.arange(70), np.arange(5, 25)
    return (repack(nodes, big if which in ("query", "both") else few, 61),
            repack(nodes, big if which in ("library", "both") else few[::-1], 62))


def limit_case(in_scope_of_others):
    """nc.limit_case on the library side (one entry of 4,097 peaks, within max_shift of the queries or far away); the queries are
    its spectra of 300 and 20 peaks -> (queries, library, max_shift)"""
    nodes, max_shift = nc.limit_case(in_scope_of_others)
    return repack(nodes, [1, 2, 3], 71), nodes, max_shift
