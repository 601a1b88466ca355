"""Representative network (`fal_network_edges`; DESIGN.md "Representative network"): the numpy restatement of the rule -- scope,
candidates, greedy matching, score, edge rule, mutual top-k -- and the case generators of the CPU and GPU tests.

Nodes are a dict: mz, intensity f32[nnz], indptr i64[n_rows + 1] (a peak CSR, m/z ascending in a row), rows i32[n] (node v is
CSR row rows[v]), precursor_mz f32[n].  The restatement works on whole candidate matrices per pair; csrc/netmatch.h walks
windows.  They agree on bits."""
import numpy as np

f32, f64 = np.float32, np.float64
MAX_PEAKS = 4096            # include/falcon_hip.h FAL_NET_MAX_PEAKS
REJECT, INLINE, GREEDY = 0, 1, 2


class Unsupported(Exception):
    """a pair in scope has a side of more than MAX_PEAKS peaks"""


def peaks(nodes, v):
    r = int(nodes["rows"][v])
    a, b = nodes["indptr"][r], nodes["indptr"][r + 1]
    return nodes["mz"][a:b], nodes["intensity"][a:b]


def in_scope(pmz_a, pmz_b, max_shift):
    return bool(abs(f64(f32(f32(pmz_b) - f32(pmz_a)))) <= max_shift)


# ---- one pair ------------------------------------------------------------------------------------------------------------------
def greedy(cand, w):
    """candidates (bool [na, nb]) with weights w taken by (w descending, i ascending, j ascending), accepted when neither peak was
    accepted before -> (score f64: the accepted w added in ascending i, matched, a candidate was refused)"""
    ii, jj = np.nonzero(cand)
    ww = w[ii, jj]
    used_a, used_b, got = set(), set(), {}
    for k in np.lexsort((jj, ii, -ww)):
        i, j = int(ii[k]), int(jj[k])
        if i in used_a or j in used_b:
            continue
        used_a.add(i), used_b.add(j)
        got[i] = ww[k]
    score = 0.0
    for i in sorted(got):
        score += float(got[i])
    return score, len(got), len(got) < len(ii)


def similarity(score):
    return f32(max(0.0, min(score, 1.0)))


def pair_ref(amz, ait, bmz, bit, shift, tol):
    """a in front of b in sorted order, shift = f32(pmz_a - pmz_b) -> dict of the pair's score and of what the kernels decide on:
    hit_a / hit_b (peaks with a partner in a window, weights ignored), widest_a / widest_b (the most partners of one peak)"""
    shift = f32(shift)
    zero = np.abs(amz[:, None] - bmz[None, :]).astype(f64) <= tol
    moved = np.abs((amz - shift)[:, None] - bmz[None, :]).astype(f64) <= tol
    w = ait[:, None] * bit[None, :]
    assert w.dtype == f32 and (amz - shift).dtype == f32
    win = zero | moved
    score, matched, refused = greedy(win & (w > 0), w)
    score0, matched0, _ = greedy(zero & (w > 0), w)
    per_a, per_b = win.sum(axis=1), win.sum(axis=0)
    return dict(sim=similarity(score), matched=matched, refused=refused, sim_zero=similarity(score0), matched_zero=matched0,
                hit_a=int((per_a > 0).sum()), hit_b=int((per_b > 0).sum()), widest_a=int(per_a.max(initial=0)),
                widest_b=int(per_b.max(initial=0)))


def need(min_matched):
    return max(int(min_matched), 1)


def classify(p, min_matched):
    """what the tile kernel does with a scored pair: REJECT by cardinality, sum it INLINE, or list it for the GREEDY kernel"""
    if p["hit_a"] < need(min_matched) or p["hit_b"] < need(min_matched):
        return REJECT
    return INLINE if p["widest_a"] <= 1 and p["widest_b"] <= 1 else GREEDY


def is_edge(sim, matched, min_cosine, min_matched):
    return matched >= need(min_matched) and f32(sim) >= f32(min_cosine)


# ---- the network -----------------------------------------------------------------------------------------------------------------
def score_pairs(nodes, fragment_tol, max_shift):
    """every pair in scope, scored -> list of pair_ref dicts with u < v (node indices) and a, b (the pair in sorted order)"""
    pmz = np.asarray(nodes["precursor_mz"], f32)
    order = np.argsort(pmz, kind="stable")                    # (precursor m/z, node index)
    out = []
    for x in range(len(order)):
        a = int(order[x])
        for y in range(x + 1, len(order)):
            b = int(order[y])
            if not in_scope(pmz[a], pmz[b], max_shift):
                continue
            pa, pb = peaks(nodes, a), peaks(nodes, b)
            if len(pa[0]) > MAX_PEAKS or len(pb[0]) > MAX_PEAKS:
                raise Unsupported((a, b))
            p = pair_ref(*pa, *pb, f32(pmz[a] - pmz[b]), fragment_tol)
            p.update(a=a, b=b, u=min(a, b), v=max(a, b))
            out.append(p)
    return out


def top_k_filter(edges, top_k):
    """edges (u, v, sim, matched) -> those among the first top_k of both ends by (sim descending, other node ascending)"""
    if top_k <= 0:
        return list(edges)
    inc = {}
    for e in edges:
        inc.setdefault(e[0], []).append((-float(e[2]), e[1], e))
        inc.setdefault(e[1], []).append((-float(e[2]), e[0], e))
    first = {n: {id(t[2]) for t in sorted(l, key=lambda t: t[:2])[:top_k]} for n, l in inc.items()}
    return [e for e in edges if id(e) in first[e[0]] and id(e) in first[e[1]]]


def network_from(scored, min_cosine, min_matched, top_k, stats=None):
    """the thresholds and the mutual top-k over `score_pairs`' records -> (u i32, v i32, sim f32, matched i32) in (u, v) order"""
    edges = sorted((p["u"], p["v"], p["sim"], p["matched"]) for p in scored if is_edge(p["sim"], p["matched"], min_cosine, min_matched))
    kept = top_k_filter(edges, top_k)
    if stats is not None:
        kinds = [classify(p, min_matched) for p in scored]
        stats.update(in_scope=len(scored), rejected_cardinality=kinds.count(REJECT), greedy_pairs=kinds.count(GREEDY),
                     refused_pairs=sum(bool(p["refused"]) for p in scored), edges_before_top_k=len(edges), edges=len(kept),
                     shift_only_edges=sum(is_edge(p["sim"], p["matched"], min_cosine, min_matched) and
                                          not is_edge(p["sim_zero"], p["matched_zero"], min_cosine, min_matched) for p in scored))
    return (np.array([e[0] for e in kept], np.int32), np.array([e[1] for e in kept], np.int32), np.array([e[2] for e in kept], f32),
            np.array([e[3] for e in kept], np.int32))


def network_ref(nodes, fragment_tol, max_shift, min_cosine, min_matched, top_k, stats=None):
    return network_from(score_pairs(nodes, fragment_tol, max_shift), min_cosine, min_matched, top_k, stats)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_edges(got, want):
    return len(got) == 4 and all(same(g, w) for g, w in zip(got, want))


# ---- generators ----------------------------------------------------------------------------------------------------------------
def make_nodes(spectra, pmz, rng=None, spare_rows=2):
    """spectra [(mz, intensity)] -> nodes; with `rng` the CSR holds them in a shuffled row order between `spare_rows` rows no node
    names"""
    n = len(spectra)
    n_rows = n + (spare_rows if rng is not None else 0)
    rows = (rng.permutation(n_rows)[:n] if rng is not None else np.arange(n)).astype(np.int32)
    by_row = [(np.zeros(0, f32), np.zeros(0, f32))] * n_rows
    for v, r in enumerate(rows):
        by_row[r] = spectra[v]
    if rng is not None:
        for r in set(range(n_rows)) - set(rows.tolist()):
            by_row[r] = (np.sort(rng.uniform(100.0, 900.0, 7)).astype(f32), rng.uniform(0.1, 1.0, 7).astype(f32))
    indptr = np.zeros(n_rows + 1, np.int64)
    indptr[1:] = np.cumsum([len(s[0]) for s in by_row])
    cat = lambda k: (np.concatenate([s[k] for s in by_row]) if n_rows else np.zeros(0)).astype(f32)
    return dict(mz=cat(0), intensity=cat(1), indptr=indptr, rows=rows, precursor_mz=np.asarray(pmz, f32))


def permute_nodes(nodes, perm):
    """the same CSR, new node v = old node perm[v]"""
    return dict(nodes, rows=nodes["rows"][perm], precursor_mz=nodes["precursor_mz"][perm])


def map_back(edges, perm):
    """edges of `permute_nodes(nodes, perm)` in the indices of `nodes`, in (u, v) order again"""
    u, v = perm[edges[0]], perm[edges[1]]
    lo, hi = np.minimum(u, v).astype(np.int32), np.maximum(u, v).astype(np.int32)
    o = np.lexsort((hi, lo))
    return lo[o], hi[o], edges[2][o], edges[3][o]


def unit(it):
    it = np.asarray(it, f64)
    return (it / np.sqrt(np.sum(it ** 2))).astype(f32)


def spectrum(mz, it):
    o = np.argsort(mz, kind="stable")
    return np.asarray(mz, f32)[o], unit(np.asarray(it)[o])


ANALOGUE_SHIFTS = (0.0, 14.0157, 15.9949, 28.0313, 42.0106)
ANALOGUE = dict(fragment_tol=0.05, max_shift=50.0, min_cosine=0.7, min_matched=6)


def analogue_case(seed=1, n_templates=8, copies=3, shifts=ANALOGUE_SHIFTS, wrap=None):
    """families of analogues: per template 24 peaks (20 apart from each other, two doublets 0.03 apart: two partners in one
    window), about half of which move with the precursor shift; per shift `copies` noisy copies.  Distinct precursors.
    `wrap` (tools/network_rate.py's scaled form): template t starts at the precursor of template t mod wrap, a little above"""
    rng = np.random.default_rng(seed)
    spectra, pmz = [], []
    for t in range(n_templates):
        base = np.sort(rng.choice(np.arange(120.0, 380.0, 1.7), 22, replace=False) + rng.uniform(-0.3, 0.3, 22))
        mz = np.concatenate([base, base[[3, 15]] + 0.03])
        it = rng.uniform(0.2, 1.0, 24)
        moves = rng.permutation(24) < 12
        moves[[22, 23]] = moves[[3, 15]]                      # a doublet moves, or stays, as one
        for s in shifts:
            for c in range(copies):
                spectra.append(spectrum(mz + moves * s + rng.normal(0.0, 0.004, 24), it * rng.uniform(0.85, 1.15, 24)))
                pmz.append(400.0 + 31.0 * (t if wrap is None else t % wrap) + s + 0.0113 * c + 0.0007 * (t if wrap is None else t // wrap))
    assert wrap is not None or len(set(np.asarray(pmz, f32).tolist())) == len(pmz)
    return make_nodes(spectra, pmz, rng)


TILE_SIZES = (1, 2, 63, 64, 65, 130)
TILE_BANDS = ("equal", "mid", "all")


def pool_spectrum(rng, pool, lo=6, hi=12, p_empty=0.05):
    if rng.random() < p_empty:
        return np.zeros(0, f32), np.zeros(0, f32)
    k = int(rng.integers(lo, hi + 1))
    pick = np.sort(rng.choice(len(pool), k, replace=False))
    return spectrum(pool[pick] + rng.normal(0.0, 0.01, k), rng.uniform(0.1, 1.0, k))


def tile_case(n, band, seed=0):
    """n small spectra over one pool of 30 m/z values (most pairs share a peak; thresholds 0 / 0 make every such pair an edge).
    band "equal": five precursor values, max_shift 0 (only equal precursors are in scope: the node index orders them);
    "mid": precursors 0.5 apart, max_shift 20.25 (a band of 40 positions: it ends inside a chunk); "all": every pair in scope
    -> (nodes, max_shift)"""
    rng = np.random.default_rng(100 * n + TILE_BANDS.index(band) + 1000 * seed)
    pool = np.sort(rng.uniform(150.0, 450.0, 30))
    spectra = [pool_spectrum(rng, pool) for _ in range(n)]
    if band == "equal":
        pmz, max_shift = rng.choice([500.0, 500.25, 501.5, 503.0, 510.0], n), 0.0
    elif band == "mid":
        pmz, max_shift = 500.0 + 0.5 * rng.permutation(n), 20.25
    else:
        pmz, max_shift = rng.uniform(300.0, 900.0, n), 1e6
    return make_nodes(spectra, pmz, rng), max_shift


def scope_edges(pmz, max_shift):
    """the float32 precursors above pmz at the end of its scope: (last inside, first outside), by stepping against the test"""
    x = f32(pmz) + f32(max_shift)
    while in_scope(pmz, x, max_shift):
        x = np.nextafter(x, f32(np.inf), dtype=f32)
    while not in_scope(pmz, x, max_shift):
        x = np.nextafter(x, f32(-np.inf), dtype=f32)
    return x, np.nextafter(x, f32(np.inf), dtype=f32)


def ulp_case(max_shift=37.3, seed=5):
    """64 nodes at one precursor, three nodes each at the last float32 precursor inside their scope and at the first outside,
    and three nodes one float32 step below the precursor.  In sorted order the first tile row ends among the 64 equal precursors:
    the binary-searched end of its band lies between the two groups of three, inside the second chunk.  Every spectrum is the
    same, so every pair in scope is an edge at thresholds 0 / 0 -> (nodes, max_shift)"""
    rng = np.random.default_rng(seed)
    p0 = f32(500.0)
    inside, outside = scope_edges(p0, max_shift)
    assert in_scope(p0, inside, max_shift) and not in_scope(p0, outside, max_shift) and np.nextafter(inside, f32(np.inf)) == outside
    below = np.nextafter(p0, f32(0))
    pmz = np.array([p0] * 64 + [inside] * 3 + [outside] * 3 + [below] * 3, f32)
    s = spectrum(np.sort(rng.uniform(150.0, 450.0, 8)), rng.uniform(0.2, 1.0, 8))
    nodes = make_nodes([s] * len(pmz), pmz, rng)
    return permute_nodes(nodes, rng.permutation(len(pmz))), max_shift


def tie_case(seed=9):
    """six byte-identical spectra with flat intensities and two doublets (equal weights inside every pair: the lower i, then the
    lower j, is taken; equal similarities between the pairs: the ranks go to the lower node), at one precursor, among other
    spectra -> nodes"""
    rng = np.random.default_rng(seed)
    base = np.sort(rng.choice(np.arange(150.0, 400.0, 2.1), 10, replace=False))
    mz = np.concatenate([base, base[[2, 7]] + 0.03])
    flat = spectrum(mz, np.ones(12))
    pool = np.sort(rng.uniform(150.0, 450.0, 30))
    spectra = [flat] * 6 + [pool_spectrum(rng, np.concatenate([pool, base]), p_empty=0.0) for _ in range(10)]
    pmz = [600.0] * 6 + list(rng.uniform(590.0, 610.0, 10))
    return permute_nodes(make_nodes(spectra, pmz, rng), rng.permutation(16))


def dense_spectrum(rng, k, lo=150.0, hi=1400.0):
    """k peaks, many of them closer than the fragment tolerance of 0.05"""
    return spectrum(rng.uniform(lo, hi, k), rng.uniform(0.1, 1.0, k))


def strip_case(seed=4, n=40, k=200):
    """n nodes of k = 200 peaks in one family (noisy copies of one spectrum with peaks closer than the tolerance: conflicts in
    every pair, sides above one strip of 64), two nodes without peaks -> nodes"""
    rng = np.random.default_rng(seed)
    mz, it = rng.uniform(150.0, 600.0, k), rng.uniform(0.1, 1.0, k)
    spectra = [spectrum(mz + rng.normal(0.0, 0.01, k), it * rng.uniform(0.8, 1.2, k)) for _ in range(n - 2)]
    spectra += [(np.zeros(0, f32), np.zeros(0, f32))] * 2
    return make_nodes(spectra, 700.0 + rng.uniform(0.0, 5.0, n), rng)


def lds_case(seed=6, n=70, k=60):
    """70 nodes of 60 peaks: a tile side of 64 rows holds 3,840 peaks, above the 3,200 that are staged -> nodes"""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.uniform(150.0, 900.0, 90))
    spectra = [pool_spectrum(rng, pool, k, k, p_empty=0.0) for _ in range(n)]
    return make_nodes(spectra, 800.0 + rng.uniform(0.0, 3.0, n), rng)


def limit_case(in_scope_of_others, seed=8, big=MAX_PEAKS + 1):
    """a few spectra of 4,096 peaks and fewer, and one of 4,097: at a precursor within max_shift of theirs, or far away
    -> (nodes, max_shift)"""
    rng = np.random.default_rng(seed)
    spectra = [dense_spectrum(rng, k) for k in (MAX_PEAKS, 300, 20, 20)] + [dense_spectrum(rng, big)]
    pmz = [700.0, 701.0, 702.0, 703.0, 704.0 if in_scope_of_others else 900.0]
    return make_nodes(spectra, pmz, rng), 10.0
