"""References and input builders shared by the linkage tie tests (test_linkage_cpu.py, test_gpu_linkage_ties.py).

`fo.linkage_clusters` and tests/golden/linkage.npz go through scipy, whose order between equal merge heights is not
specified.  The kernels of csrc/linkage.hip state their own: always the pair with the smallest height, ties -> lowest
(a, b) in the group's ascending-row numbering, Lance-Williams updates in float64, stop at the first height > t.  The
references here restate exactly that in plain numpy, so inputs made of ties (lattices, matrices of five values) have ONE
answer the kernels can be held to, integer for integer.  Plain numpy: no torch, no GPU, no import of the library."""
import functools

import numpy as np

WAVE_MAX = 256                   # csrc/linkage.hip kLinkageWaveMax: groups above it take lk_agglomerate_big_kernel
NO_PARTNER = 0x7fffffff


# --------------------------------------------------------------------------- references
def agglomerate_ref(D, t, method, tie="lowest", stats=None):
    """Naive agglomeration of one group.  D: symmetric float64 [m, m].  Every step takes the argmin of D over the active
    pairs a < b in row-major order (smallest value, then lowest a, then lowest b), stops when `not (v <= t)`, gives every
    other active c the height max(D[a,c], D[b,c]) (complete) or (sa*D[a,c] + sb*D[b,c]) / (sa + sb) (average) in float64 and
    retires b.  -> int64[m]: the lowest local index of every member's cluster, -1 for clusters of one.
    `tie="highest"` is the OPPOSITE rule (highest (a, b) among the ties): only to show that an input tells the two apart.
    `stats` (a dict) receives `steps` (merges made) and `tied` (merges whose minimum was held by more than one pair)."""
    assert method in ("complete", "average") and tie in ("lowest", "highest")
    D = np.array(D, np.float64)
    m = len(D)
    assert D.shape == (m, m)
    W = np.where(np.triu(np.ones((m, m), bool), 1), D, np.inf)     # the active pairs a < b; everything else +inf
    flat = W.reshape(-1)
    act = np.ones(m, bool)
    sz = np.ones(m, np.float64)
    cl = np.arange(m)
    steps = tied = 0
    for _ in range(m - 1):
        i = int(np.argmin(flat)) if tie == "lowest" else m * m - 1 - int(np.argmin(flat[::-1]))
        v = flat[i]
        if not (v <= t):
            break
        a, b = divmod(i, m)
        steps += 1
        if stats is not None:
            tied += int(np.count_nonzero(flat == v) > 1)
        other = act.copy()
        other[a] = other[b] = False
        c = np.flatnonzero(other)
        sa, sb = sz[a], sz[b]
        nv = np.maximum(D[a, c], D[b, c]) if method == "complete" else (sa * D[a, c] + sb * D[b, c]) / (sa + sb)
        D[a, c] = nv
        D[c, a] = nv
        W[np.minimum(a, c), np.maximum(a, c)] = nv
        W[b, :] = np.inf
        W[:, b] = np.inf
        act[b] = False
        sz[a] = sa + sb
        cl[cl == b] = a
    if stats is not None:
        stats["steps"], stats["tied"] = steps, tied
    return np.where(sz[cl] >= 2, cl, -1).astype(np.int64)


def agglomerate_cached_ref(D, t, method):
    """A sequential port of lk_agglomerate_big_kernel's bookkeeping: every active row a keeps its nearest active partner
    b > a (`nnv`, `nni`: smallest value, ties -> lowest b); the merge is the smallest cached value, ties -> lowest a; after a
    merge of (ba, bb) the rows c < bb whose partner was bb, or was ba with c < ba, are searched again (`todo`), as is ba; any
    other c < ba takes ba in place when `nv < nnv[c] or (nv == nnv[c] and ba < nni[c])`.
    In exact arithmetic the in-place rule cannot fire (before the merge D[c][ba] > nnv[c] or nni[c] < ba, the same for bb, and
    a reducible update stays at or above the smaller of the two); in float64 the mean (sa*x + sb*x) / (sa + sb) of two EQUAL
    heights can round below x, and then it does (`two_values_matrix`).
    -> (representatives as `agglomerate_ref`, how often the in-place rule replaced an entry)"""
    assert method in ("complete", "average")
    D = np.array(D, np.float64)
    m = len(D)
    act = np.ones(m, bool)
    sz = np.ones(m, np.float64)
    cl = np.arange(m)
    nnv = np.full(m, np.inf)
    nni = np.full(m, NO_PARTNER, np.int64)

    def search_row(a):
        b = a + 1 + np.flatnonzero(act[a + 1:])
        if len(b) == 0:
            nnv[a], nni[a] = np.inf, NO_PARTNER
            return
        j = int(np.argmin(D[a, b]))                                 # the first minimum: the lowest b
        nnv[a], nni[a] = D[a, b[j]], b[j]

    for a in range(m):
        search_row(a)
    replaced = 0
    for _ in range(m - 1):
        cand = np.where(act, nnv, np.inf)
        ba = int(np.argmin(cand))                                   # the first minimum: the lowest a
        bv = cand[ba]
        if not (bv <= t):
            break
        bb = int(nni[ba])
        sa, sb = sz[ba], sz[bb]
        cl[cl == bb] = ba
        todo = []
        for c in range(m):
            if not act[c] or c == ba or c == bb:
                continue
            dac, dbc = D[ba, c], D[bb, c]
            nv = max(dac, dbc) if method == "complete" else (sa * dac + sb * dbc) / (sa + sb)
            D[ba, c] = nv
            D[c, ba] = nv
            if c < bb:
                p = nni[c]
                if p == bb or (p == ba and c < ba):
                    todo.append(c)
                elif c < ba and (nv < nnv[c] or (nv == nnv[c] and ba < p)):
                    nnv[c], nni[c] = nv, ba
                    replaced += 1
        act[bb] = False
        sz[ba] = sa + sb
        todo.append(ba)
        for a in todo:
            search_row(a)
    return np.where(sz[cl] >= 2, cl, -1).astype(np.int64), replaced


def _components(n, ei, ej):
    """connected components of the undirected edges (ei[x], ej[x]) -> the lowest row of every row's component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(ei.tolist(), ej.tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)                           # the lower root stays: root = lowest row
    return np.array([find(x) for x in range(n)], np.int64)


def _linkage_from_slots(n, rows, cols, dist64, t, method, tie="lowest", stats=None):
    """the shared body of `linkage_ref` / `linkage_ref_csr`: stored slots (rows[x] -> cols[x], float64 distance), cut t"""
    assert t < 1.0 and method in ("single", "complete", "average")
    ok = (cols >= 0) & (cols < n) & (cols != rows)
    rows, cols, dist64 = rows[ok], cols[ok], dist64[ok]
    e = dist64 <= t
    comp = _components(n, rows[e], cols[e])
    rep = np.full(n, -1, np.int64)
    lidx = np.zeros(n, np.int64)
    inside = comp[rows] == comp[cols]
    rows, cols, dist64 = rows[inside], cols[inside], dist64[inside]
    slot_comp = comp[rows]
    steps = tied = 0
    for root in np.flatnonzero(comp == np.arange(n)):
        members = np.flatnonzero(comp == root)                      # ascending rows
        m = len(members)
        if m < 2:
            continue
        if method == "single":
            rep[members] = root
            continue
        lidx[members] = np.arange(m)
        D = np.ones((m, m), np.float64)
        s = slot_comp == root
        D[lidx[rows[s]], lidx[cols[s]]] = dist64[s]                 # slots with d > t included
        D = np.minimum(D, D.T)
        st = {} if stats is not None else None
        loc = agglomerate_ref(D, t, method, tie, st)
        if st is not None:
            steps, tied = steps + st["steps"], tied + st["tied"]
        rep[members] = np.where(loc >= 0, members[np.maximum(loc, 0)], -1)
    if stats is not None:
        stats["steps"], stats["tied"] = steps, tied
    labels = np.full(n, -1, np.int32)
    reps = np.unique(rep[rep >= 0])                                 # clusters numbered by their lowest row
    has = rep >= 0
    labels[has] = np.searchsorted(reps, rep[has]).astype(np.int32)
    return labels


def linkage_ref(nb_idx, nb_dist, t, method, tie="lowest", stats=None):
    """The contract of `fo.linkage_clusters` / `fal_linkage_cluster` with the kernels' tie rule.  t32 = float32(t); an edge
    i - j exists where 0 <= j < n, j != i and nb_dist <= t32 (either direction); connected components, members in ascending
    row order; single: the component is the cluster; complete / average: D = 1.0, filled from the stored slots of the members
    whose neighbour is in the same component (slots with d > t included), D = minimum(D, D.T), `agglomerate_ref` at
    float(t32).  -> labels int32[n] numbered by lowest row, clusters of one = -1."""
    nb_idx = np.asarray(nb_idx)
    n, k = nb_idx.shape
    t32 = np.float32(t)
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    return _linkage_from_slots(n, rows, nb_idx.reshape(-1).astype(np.int64),
                               np.asarray(nb_dist, np.float32).reshape(-1).astype(np.float64), float(t32), method, tie, stats)


def linkage_ref_csr(ptr, idx, dist, t, method, tie="lowest", stats=None):
    """the same over a CSR of float64 distances (`fal_linkage_cluster_csr`, single / complete): the cut stays a float64"""
    ptr = np.asarray(ptr, np.int64)
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    return _linkage_from_slots(n, rows, np.asarray(idx).astype(np.int64), np.asarray(dist, np.float64), float(t), method, tie,
                               stats)


def component_sizes(labels_single):
    """sizes of the clusters of a `single` labelling, ascending"""
    lab = np.asarray(labels_single)
    return sorted(np.bincount(lab[lab >= 0]).tolist())


# --------------------------------------------------------------------------- input builders
def points_graph(pos, k):
    """every row's k nearest OTHER rows by float32 Euclidean distance clipped to 0.99 (stable argsort: ties -> lowest row);
    unused slots are -1 / inf.  -> nb_idx int32[n, k], nb_dist float32[n, k]"""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    nb_idx = np.full((n, k), -1, np.int32)
    nb_dist = np.full((n, k), np.inf, np.float32)
    for i0 in range(0, n, 512):
        blk = np.sqrt(((pos[i0:i0 + 512, None] - pos[None]) ** 2).sum(-1)).astype(np.float32)
        blk = np.clip(blk, 0, np.float32(0.99))
        order = np.argsort(blk, axis=1, kind="stable")
        for r in range(len(blk)):
            i = i0 + r
            o = order[r][:k + 1]
            o = o[o != i][:k]
            nb_idx[i, :len(o)] = o
            nb_dist[i, :len(o)] = blk[r][o]
    return nb_idx, nb_dist


def lattice_points(sizes, n_isolated=0):
    """each (w, h): a w x h grid with spacing 1/64 (row-major: x fastest), the groups 100 apart; then `n_isolated` single
    points far from everything and from each other.  Coordinates are exact binary fractions: equal offsets give equal
    distances, bit for bit."""
    pts = []
    for g, (w, h) in enumerate(sizes):
        y, x = np.divmod(np.arange(w * h), w)
        pts.append(np.stack([100.0 * g + x / 64.0, y / 64.0], 1))
    for i in range(n_isolated):
        pts.append(np.array([[-1000.0 - 100.0 * i, 500.0]]))
    return np.concatenate(pts)


def lattice_graph(sizes, k, seed, n_isolated=0):
    """`lattice_points` shuffled with the seed (seed None: left in order) -> `points_graph`"""
    pos = lattice_points(sizes, n_isolated)
    if seed is not None:
        pos = pos[np.random.default_rng(seed).permutation(len(pos))]
    return points_graph(pos, k)


def few_values_matrix(m, seed):
    """symmetric [m, m]: entries drawn from {1..5}/64, half of them set to 1.0 (a missing pair), symmetrised by `minimum`,
    zero diagonal"""
    rng = np.random.default_rng(seed)
    D = rng.integers(1, 6, size=(m, m)).astype(np.float64) / 64.0
    D[rng.random((m, m)) < 0.5] = 1.0
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return D


def two_values_matrix(m, seed, share=0.15, f32=False):
    """symmetric [m, m] of two heights that are no binary fractions: 0.05 * two uniform draws (rounded to float32 first with
    `f32`, so that neighbour lists hold them exactly); `share` of the cells drawn the smaller, symmetrised by `minimum`, zero
    diagonal.  Average linkage of clusters at EQUAL heights x gives (sa*x + sb*x) / (sa + sb), which float64 rounds below x for
    some sizes: the inputs on which the big kernel's in-place replacement fires."""
    rng = np.random.default_rng(seed)
    vals = np.sort(rng.random(2)) * 0.05
    if f32:
        vals = vals.astype(np.float32).astype(np.float64)
    D = np.where(rng.random((m, m)) < share, vals[0], vals[1])
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return D


def to_neighbour_lists(D):
    """every off-diagonal cell below 1 becomes a stored slot (ascending neighbour), k = the largest degree; the padding is
    -1 / inf.  -> nb_idx int32[m, k], nb_dist float32[m, k]"""
    D = np.asarray(D, np.float64)
    m = len(D)
    stored = D < 1.0
    np.fill_diagonal(stored, False)
    k = max(int(stored.sum(1).max()), 1)
    nb_idx = np.full((m, k), -1, np.int32)
    nb_dist = np.full((m, k), np.inf, np.float32)
    for i in range(m):
        j = np.flatnonzero(stored[i])
        nb_idx[i, :len(j)] = j
        nb_dist[i, :len(j)] = D[i, j]
    return nb_idx, nb_dist


def to_matrix(nb_idx, nb_dist):
    """the float64 matrix of ONE group given as neighbour lists: 1.0 where no direction is stored, the smaller direction else"""
    n = len(nb_idx)
    D = np.ones((n, n), np.float64)
    for i in range(n):
        ok = (nb_idx[i] >= 0) & (nb_idx[i] < n) & (nb_idx[i] != i)
        D[i, nb_idx[i][ok]] = nb_dist[i][ok]
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return D


def pairs_to_csr(n, rows, cols, d):
    """The layout exact mode hands to `fal_linkage_cluster_csr`, stated once (test_gpu_exact_paths.py's `_hand_csr` builds its
    three rows through it): indptr int64[n+1], idx int32, dist float64, SYMMETRIC -- every pair (rows[x], cols[x], d[x]) and its
    mirror -- with rows and columns ascending; a pair given more than once keeps the smallest distance"""
    rows, cols, d = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(d, np.float64)
    r2, c2, d2 = np.concatenate([rows, cols]), np.concatenate([cols, rows]), np.concatenate([d, d])
    o = np.lexsort((d2, c2, r2))
    r2, c2, d2 = r2[o], c2[o], d2[o]
    first = np.ones(len(r2), bool)
    first[1:] = (r2[1:] != r2[:-1]) | (c2[1:] != c2[:-1])
    r2, c2, d2 = r2[first], c2[first], d2[first]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.int64)
    return ptr, c2.astype(np.int32), d2


def neighbour_lists_to_csr(nb_idx, nb_dist):
    """`pairs_to_csr` of every stored slot (ids outside the table and self ids dropped)"""
    n, k = nb_idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = nb_idx.reshape(-1).astype(np.int64)
    ok = (cols >= 0) & (cols < n) & (cols != rows)
    return pairs_to_csr(n, rows[ok], cols[ok], nb_dist.reshape(-1)[ok])


def curve_graph(m, k):
    """the distinct-height input of test_gpu_linkage.py::test_linkage_of_a_group_of_thousands_of_rows_equals_scipy: a noisy
    curve of m rows (one connected group at the cuts 0.05 / 0.04) next to 20 groups of 30 rows"""
    rng = np.random.default_rng(m)
    s = np.arange(m) * 0.006
    pos = np.stack([s, 0.008 * rng.normal(size=m)], 1)
    small = np.concatenate([rng.normal(size=(30, 2)) * 0.01 + np.array([0.0, 50.0 + 5 * g]) for g in range(20)])
    return points_graph(np.concatenate([pos, small]), k)


def pairs_and_triples_graph():
    """k = 1: one stored neighbour a row.  Rows 0-1 a pair stored both ways, 2-3 a pair stored one way (3 points outside the
    table), 4-5-6 a chain 4 -> 5 -> 6 -> 5 (the pair (4, 6) is missing: distance 1), 7 a row pointing at itself, 8 -> 9 above
    the cut (no edge), 9 an empty slot, 10-11-12 a chain with equal distances."""
    idx = np.array([1, 0, 3, 13, 5, 6, 5, 7, 9, -1, 11, 12, 11], np.int32)[:, None]
    dist = np.array([.25, .25, .125, .0625, .125, .25, .25, 0., .75, np.inf, .25, .25, .25], np.float32)[:, None]
    return idx, dist


# --------------------------------------------------------------------------- the inputs of the tie tests, by name
COMPOSITE_SIZES = [(2, 1), (3, 1), (5, 1), (9, 7), (8, 8), (13, 5), (17, 15), (16, 16), (257, 1), (32, 32), (41, 25)]
COMPOSITE_ISOLATED = 7
LATTICE_K = 24
CUT = {"complete": 3 / 64, "average": 2.5 / 64, "single": 3 / 64}
CSR_SIZES = [(2, 1), (17, 15), (3, 1), (16, 16), (5, 4), (257, 1)]


@functools.lru_cache(maxsize=None)
def tie_input(name):
    """neighbour lists of a named input (cached: the CPU and the GPU tests of one run share them; treat as read-only)
      composite   groups of 2, 3, 5, 63, 64, 65, 255, 256, 257, 1,024 and 1,025 rows + 7 isolated rows, shuffled
      grid256     a 16 x 16 lattice, shuffled;  grid257: the same rows + one that continues the first grid row (row 256, the
                  highest-numbered member): one row apart, the two take different kernels
      few150 / few300   `few_values_matrix` as neighbour lists: one group, degree above 64
      csr         groups of 2, 255, 3, 256, 20 and 257 rows, shuffled"""
    if name == "composite":
        return lattice_graph(COMPOSITE_SIZES, LATTICE_K, 2024, COMPOSITE_ISOLATED)
    if name in ("grid256", "grid257"):
        pos = lattice_points([(16, 16)])[np.random.default_rng(5).permutation(256)]
        if name == "grid257":
            pos = np.concatenate([pos, [[16 / 64.0, 0.0]]])
        return points_graph(pos, LATTICE_K)
    if name == "few150":
        return to_neighbour_lists(few_values_matrix(150, 150))
    if name == "few300":
        return to_neighbour_lists(few_values_matrix(300, 300))
    if name == "csr":
        return lattice_graph(CSR_SIZES, LATTICE_K, 77, 3)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def rounding_input():
    """-> (nb_idx, nb_dist, cut): `two_values_matrix(300, 20, 0.05, f32=True)` as neighbour lists (one group of 300 rows, 299
    slots a row: the big kernel) and a cut at 0.9 of the larger height, as a float32.  Average linkage up to that cut makes
    251 merges, leaves 49 clusters, and the in-place rule of the cached-partner bookkeeping fires twice on the way."""
    D = two_values_matrix(300, 20, 0.05, f32=True)
    idx, dist = to_neighbour_lists(D)
    return idx, dist, float(np.float32(D.max() * 0.9))


@functools.lru_cache(maxsize=None)
def tie_reference(name, method, tie="lowest"):
    """-> (`linkage_ref` labels of `tie_input(name)` at CUT[method], merge steps, merge steps with a tied minimum)"""
    idx, dist = tie_input(name)
    st = {}
    lab = linkage_ref(idx, dist, CUT[method], method, tie, st)
    lab.setflags(write=False)
    return lab, st["steps"], st["tied"]
