"""References and input builders of the graph-tail tests (test_tail_cpu.py, test_gpu_tail.py): a8 filter, a9 DBSCAN,
a10 refinement, a11 medoids, a12 global labels.

The references restate DESIGN section 3 and include/falcon_hip.h in plain numpy / Python, independent of the oracle's
vectorised forms (test_tail_cpu.py holds the two against each other), of the kernels and of the wrappers.  Each takes
`variant=`: exactly one rule replaced by its neighbour (`<` for `<=`, highest for lowest, ...).  The variants are never
right; they exist so that every input can be shown to tell the rule from its neighbour -- an input on which a variant
gives the reference's result says nothing about that rule.  Every builder is seeded and returns numpy arrays only:
no torch, no GPU, no import of the library."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
EPS = 0.1                                      # a9's eps of every G input
EPS32 = f32(EPS)
EPS_UP, EPS_DOWN = np.nextafter(EPS32, f32(1)), np.nextafter(EPS32, f32(0))
M_EPS = 0.6                                    # the eps the M graphs are clustered with when they go through the fused calls
WIDE = dict(tol=1.0, mode="Da", rt_tol=None)   # with one m/z for every row: a10 keeps every cluster of two or more rows

FILTER_VARIANTS = ("lt", "noclamp", "last")
DBSCAN_VARIANTS = ("lt", "self_core", "highest", "lowest_cluster", "past_count")
REFINE_VARIANTS = ("rightmost", "lt", "unstable", "by_value", "pairs")
MEDOID_VARIANTS = ("tie_highest", "tie_dataset", "f64", "ascending", "missing0")
LABEL_VARIANTS = ("noise_sorted",)


def mass_diff(a, b, is_da):
    """float32 difference, float32 division, float64 product with 10^6 ("tolerance arithmetic")"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    diff = (a - b).astype(f32)
    if is_da:
        return diff.astype(f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (diff / b).astype(f32).astype(f64) * 1e6


# =========================================================================== a8 filter
def filter_ref(sim, idx, mz, rt, tol, mode, rt_tol, n_neighbors, variant=None):
    """Row by row: drop empty slots, the row itself, candidates outside the precursor tolerance |mass_diff(query, candidate)|
    <= tol and (with `rt_tol`) outside |rt_q - rt_c| <= rt_tol (float32 difference); keep the first `n_neighbors` survivors in
    slot order with dist = 1 - sim clamped to [0, 1]; pad with (-1, +inf).
    variants: "lt" (< at both tolerances), "noclamp", "last" (the last n_neighbors survivors)."""
    assert variant in (None,) + FILTER_VARIANTS
    n, ka = idx.shape
    out_idx = np.full((n, n_neighbors), -1, np.int32)
    out_dist = np.full((n, n_neighbors), np.inf, f32)
    mz = np.asarray(mz, f32)
    for i in range(n):
        cand = np.flatnonzero((idx[i] >= 0) & (idx[i] != i))
        j = idx[i, cand]
        md = np.abs(mass_diff(np.full(len(j), mz[i], f32), mz[j], mode == "Da"))
        ok = md < tol if variant == "lt" else md <= tol
        if rt_tol is not None:
            rd = np.abs((f32(rt[i]) - np.asarray(rt, f32)[j]).astype(f32)).astype(f64)
            ok &= rd < rt_tol if variant == "lt" else rd <= rt_tol
        surv = cand[ok]
        surv = surv[-n_neighbors:] if variant == "last" else surv[:n_neighbors]
        d = (f32(1.0) - sim[i, surv].astype(f32)).astype(f32)
        if variant != "noclamp":
            d = np.minimum(np.maximum(d, f32(0)), f32(1))
        out_idx[i, :len(surv)] = idx[i, surv]
        out_dist[i, :len(surv)] = d
    return out_idx, out_dist


F_N = 259
F_K_ANN = (1, 63, 64, 65, 200)
F_N_NEIGHBORS = (1, 5, 64, 70)
F_GROUPS = ((500.0, 90), (500.125, 40), (500.25, 40), (500.5, 83))      # multiples of 0.125; exactly 0.25 Da: groups 0-2 and 2-3
F_CONFIGS = {                                   # name -> (tol, mode, rt_tol, RT handed in)
    "da": (0.25, "Da", None, False),
    "da_rt": (0.25, "Da", 8.0, True),
    "da_rt_unused": (0.25, "Da", None, True),   # RT given, rt_tol None: the column must not be read
    "ppm": (20.0, "ppm", None, False),
}


def ppm_pair(lo, tol=20.0, query_is_hi=True):
    """the largest float32 `hi` above `lo` whose ppm difference is still <= tol, and the next float32 (the first beyond it),
    found by stepping np.nextafter under `mass_diff` -- (hi - lo) / lo when the query is `hi` (a8 at the row of `hi`; a10's
    link distance), (lo - hi) / hi otherwise"""
    lo = f32(lo)
    md = (lambda h: abs(float(mass_diff(h, lo, False)))) if query_is_hi else (lambda h: abs(float(mass_diff(lo, h, False))))
    hi = f32(lo * f32(1.0 + tol * 1e-6))
    while md(hi) <= tol:
        hi = np.nextafter(hi, f32(np.inf))
    while md(hi) > tol:
        hi = np.nextafter(hi, f32(0))
    up = np.nextafter(hi, f32(np.inf))
    assert md(hi) <= tol < md(up)
    return hi, up


@functools.lru_cache(maxsize=None)
def filter_rows():
    """precursor m/z (ascending) and RT of the 259 rows every F input shares.  Rows 0..252: four groups at multiples of
    0.125 (0.25 Da = the tolerance between groups 0 and 2, 0.125 between neighbours, 0.5 between 0 and 3).  Rows 253..255:
    700, 700.25 and the next float32 above it.  Rows 256..258: 800, the last float32 within 20 ppm of it, the first beyond.
    RT is 8 on every fourth row (the "full" rows below) and on the six special rows, else 0 / 8 / 16 by row: differences of
    exactly rt_tol = 8 everywhere, 16 between some."""
    mz = np.concatenate([np.full(c, v, f32) for v, c in F_GROUPS])
    hi, up = ppm_pair(800.0)
    mz = np.concatenate([mz, np.array([700.0, 700.25, np.nextafter(f32(700.25), f32(np.inf)), 800.0, hi, up], f32)])
    assert len(mz) == F_N and np.all(np.diff(mz) >= 0)
    i = np.arange(F_N)
    rt = np.where((i % 4 == 1) | (i >= 253), 8.0, 8.0 * (i % 3)).astype(f32)
    return mz, rt


@functools.lru_cache(maxsize=None)
def filter_input(k_ann, n_neighbors):
    """sim / idx [259, k_ann] of one (k_ann, n_neighbors) case.  By row % 4 (rows 0..252):
      1  "full": candidates are other rows of the row's own m/z group first -- no self, no hole (65 survivors at k_ann 65)
         but for one at slot 10 on rows % 8 == 5 (the 64th survivor then sits in slot 64);
      0  "late": 64 rows of a group out of tolerance first, then the own group: `kept` starts to count in the second
         64-candidate chunk, so n_neighbors 1 and 5 are reached there too (group 2 is within 0.25 Da of every group:
         its late rows are ordinary ones under Da);
      3  "edge": slot 0 holds a row exactly 0.25 Da away where the groups have one, then a random order;
      2  "mixed": a random order;
    all but "full" with -1 holes (one slot in nine) and the row's own id.  The special rows name their two partners first.
    sim rows descend over {1.0000001, 1, 0.3, 0, -0.2} (both clamps of 1 - sim); odd rows start at 1.0000001,
    rows % 4 == 2 start at -0.2 (all of the row, then)."""
    rng = np.random.default_rng(1000 * k_ann + n_neighbors)
    mz, _ = filter_rows()
    n = F_N
    group = np.searchsorted(np.cumsum([c for _, c in F_GROUPS]), np.arange(n), side="right")     # specials: group 4
    far_of = {0: 3, 1: 3, 2: 3, 3: 0}
    edge_of = {0: 2, 2: 0, 1: 3, 3: 1}          # 1 <-> 3 are 0.375 apart: out of tolerance in slot 0
    idx = np.empty((n, k_ann), np.int32)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        own = rng.permutation(others[group[others] == group[i]])
        if i >= 253:
            base = 253 + 3 * ((i - 253) // 3)
            p = [base + (i - base + 1) % 3, base + (i - base + 2) % 3]
            cand = np.concatenate([p, rng.permutation(np.setdiff1d(others, p))])
            kind = 2
        else:
            kind = i % 4
            if kind == 1:
                cand = np.concatenate([own, rng.permutation(np.setdiff1d(others, own))])
            elif kind == 0:
                far = rng.permutation(others[group[others] == far_of[group[i]]])[:64]
                cand = np.concatenate([far, own, rng.permutation(np.setdiff1d(others, np.concatenate([far, own])))])
            else:
                cand = rng.permutation(others)
                if kind == 3:
                    first = rng.choice(others[group[others] == edge_of[group[i]]])
                    cand = np.concatenate([[first], cand[cand != first]])
        row = cand[:k_ann].astype(np.int32)
        if kind != 1 and k_ann > 2 and i < 253:
            holes = np.flatnonzero(rng.random(k_ann) < 1 / 9)
            holes = holes[(holes > 0) & (holes < k_ann - 1)]          # in the middle of the row
            row[holes] = -1
            row[rng.integers(1, k_ann - 1)] = i                       # the row's own id
        if kind == 1 and i % 8 == 5 and k_ann > 11:
            row[10] = -1
        idx[i] = row
    vals = np.array([1.0000001, 1.0, 0.3, 0.0, -0.2], f32)
    sim = np.empty((n, k_ann), f32)
    for i in range(n):
        cuts = np.sort(rng.integers(0, k_ann + 1, 4))
        row = vals[np.searchsorted(cuts, np.arange(k_ann), side="right")]
        if i % 2 == 1:
            row[0] = vals[0]
        if i % 4 == 2:
            row[:] = vals[4]
        sim[i] = row
    assert np.all(np.diff(sim, axis=1) <= 0)
    return sim, idx


def filter_cases():
    """-> [(k_ann, n_neighbors, config name)], every combination"""
    return [(ka, nn, c) for ka in F_K_ANN for nn in F_N_NEIGHBORS for c in F_CONFIGS]


def filter_args(k_ann, n_neighbors, config):
    """-> sim, idx, mz, rt or None, tol, mode, rt_tol, n_neighbors: the arguments of `filter_ref` / `fo.filter_neighbors`"""
    sim, idx = filter_input(k_ann, n_neighbors)
    mz, rt = filter_rows()
    tol, mode, rt_tol, with_rt = F_CONFIGS[config]
    return sim, idx, mz, (rt if with_rt else None), tol, mode, rt_tol, n_neighbors


def filter_catches(k_ann, n_neighbors, config):
    """the variants the case is built to tell from the rule: the clamps everywhere (a survivor with sim 1.0000001 or -0.2 in
    a kept slot); "last" where a row has more survivors than n_neighbors (the full rows: k_ann survivors); "lt" where a
    difference equals the tolerance: 0.25 Da (not under ppm: no pair of the rows is at 20 ppm to the bit, the ppm pair brackets it)"""
    c = ["noclamp"]
    if k_ann > n_neighbors:
        c.append("last")
    if config != "ppm":
        c.append("lt")
    return tuple(c)


@functools.lru_cache(maxsize=None)
def filter_reference(k_ann, n_neighbors, config):
    return filter_ref(*filter_args(k_ann, n_neighbors, config))


# =========================================================================== a9 DBSCAN
def cut_at_count(idx, dist, nb_count):
    """the graph a counted call sees: slots at and behind min(nb_count, k) hold nothing"""
    if nb_count is None:
        return idx, dist
    behind = np.arange(idx.shape[1])[None, :] >= np.asarray(nb_count)[:, None]
    return np.where(behind, -1, idx).astype(np.int32), np.where(behind, np.inf, dist).astype(f32)


def dbscan_ref(idx, dist, eps, nb_count=None, variant=None):
    """DBSCAN(min_samples = 2) as DESIGN section 3 states it: an eps-edge i -> j is a stored slot (below nb_count[i] where
    counts are given) with j != i and float32 dist <= float32 eps; core(i) <=> row i has an eps-edge; clusters = components
    of the cores under core -> core edges taken as undirected, numbered by their lowest core; a non-core j with in-edges
    from cores joins the cluster of the LOWEST-INDEX such core; everything else -1.  -> labels int32[n], cluster count.
    variants: "lt" (dist < eps), "self_core" (a self slot within eps makes the row core), "highest" (border -> highest-index
    core in-neighbour), "lowest_cluster" (border -> the in-neighbour of the lowest cluster), "past_count" (nb_count ignored)."""
    assert variant in (None,) + DBSCAN_VARIANTS
    n, k = idx.shape
    e32 = f32(eps)
    if nb_count is not None and variant != "past_count":
        idx, dist = cut_at_count(idx, dist, nb_count)
    rows = np.arange(n)[:, None]
    near = (dist < e32) if variant == "lt" else (dist <= e32)
    edge = (idx >= 0) & (idx < n) & (idx != rows) & near
    core = edge.any(1)
    if variant == "self_core":
        core |= ((idx == rows) & near).any(1)
    src, slot = np.nonzero(edge)
    dst = idx[src, slot]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(src.tolist(), dst.tolist()):
        if core[a] and core[b]:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)          # the root is the component's lowest core
    labels = np.full(n, -1, np.int32)
    number = {}
    for i in np.flatnonzero(core).tolist():
        labels[i] = number.setdefault(find(i), len(number))
    votes = {}
    for a, b in zip(src.tolist(), dst.tolist()):
        if core[a] and not core[b]:
            votes.setdefault(b, []).append(a)
    for b, cores in votes.items():
        if variant == "highest":
            labels[b] = labels[max(cores)]
        elif variant == "lowest_cluster":
            labels[b] = min(int(labels[a]) for a in cores)
        else:
            labels[b] = labels[min(cores)]
    return labels, len(number)


def single_linkage_ref(idx, dist, t):
    """components of the undirected edges with dist <= t, numbered by lowest row, components of one row -1 (the contract of
    `fal_linkage_cluster` for method single)"""
    n = len(idx)
    rows = np.arange(n)[:, None]
    src, slot = np.nonzero((idx >= 0) & (idx != rows) & (dist <= f32(t)))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(src.tolist(), idx[src, slot].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(n)])
    size = np.bincount(root, minlength=n)
    keep = size[root] >= 2
    _, inv = np.unique(root[keep], return_inverse=True)
    labels = np.full(n, -1, np.int32)
    labels[keep] = inv
    return labels


def drop_single_member_clusters(labels):
    """labels with every cluster of one row set to -1 and the others renumbered in their order: what a10 makes of DBSCAN
    labels when the tolerance splits nothing"""
    labels = np.asarray(labels)
    out = np.full(len(labels), -1, np.int32)
    if (labels >= 0).any():
        size = np.bincount(labels[labels >= 0])
        new = np.cumsum(size >= 2) - 1
        keep = (labels >= 0) & (size[np.where(labels >= 0, labels, 0)] >= 2)
        out[keep] = new[labels[keep]]
    return out


G_SLOT_K = (1, 7, 8, 9, 63, 64, 65, 130)
G_SLOT_N = 1003
G_BORDER_LABELS = np.array([0, 1, 0, 1, 1, 0, 2, -1, 3, 1, 0, 3], np.int32)    # worked out by hand, see g_border()


def g_slots(k, packed):
    """1,003 rows in blocks of 11 (coprime with every k): the block's rows 2..10 name its row 0, rows 0 and 1 name each other
    (the last two rows of the array are such a pair as well); every row stores exactly ONE neighbour within eps (at eps to
    the bit) and stores it at slot `row mod k`.  Nobody names rows 2..10 of a block: a row whose slot is missed is noise.
    packed = False: the other slots are -1.  packed = True: they hold other rows at distance 0.5, nb_count = k.
    -> idx, dist, nb_count or None"""
    n = G_SLOT_N
    rng = np.random.default_rng(77 + k)
    i = np.arange(n)
    r = i % 11
    target = np.where(r == 0, i + 1, np.where(r == 1, i - 1, i - r))
    target[n - 2:] = [n - 1, n - 2]
    if packed:
        idx = np.empty((n, k), np.int32)
        for a in range(n):
            pool = np.setdiff1d(np.arange(n), [a, target[a]])
            idx[a] = rng.choice(pool, k, replace=False)
        dist = np.full((n, k), 0.5, f32)
    else:
        idx = np.full((n, k), -1, np.int32)
        dist = np.full((n, k), np.inf, f32)
    idx[i, i % k] = target
    dist[i, i % k] = EPS32
    return idx, dist, (np.full(n, k, np.int32) if packed else None)


def g_slot_leaf_slots(k):
    """the slots at which the rows nobody names (block rows 2..10) keep their neighbour: must be every slot of the row"""
    i = np.arange(G_SLOT_N - 2)
    return np.unique(i[i % 11 >= 2] % k)


def g_eps():
    """307 rows, k = 5, random neighbours, every distance one of float32(0.1), the float32 above, the float32 below"""
    rng = np.random.default_rng(5)
    n, k = 307, 5
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    for i in range(n):
        c = rng.integers(0, 3)                                 # most rows store little: many small clusters
        pool = np.setdiff1d(np.arange(max(0, i - 6), min(n, i + 7)), [i])
        idx[i, :c] = rng.choice(pool, c, replace=False)
        dist[i, :c] = rng.choice(np.array([EPS32, EPS_UP, EPS_DOWN], f32), c)
    return idx, dist, None


def g_border():
    """12 rows, k = 3, by hand (-> expected labels G_BORDER_LABELS, 4 clusters):
       0 -> 2            core                     cluster 0 = {0, 2, 5}: 5 -> 0 is one-directional
       1 -> 3, 9         core                     cluster 1 = {1, 3, 4}: 1 -> 3 is one-directional
       2 -> 0, 10        core
       3 -> 4            core
       4 -> 3 (at eps)   core
       5 -> 0, 9         core
       6 -> 10           core, its only eps-neighbour is the border 10: cluster 2 = {6}, one member
       7 -> 7 (0.05)     a self slot within eps and nothing else: not core, noise
       8 -> 7 (0.5), 11 (one float32 above eps): not core; the border of core 11 -> label 3
       9 -> 0 (0.3)      border of cores 1 (cluster 1) and 5 (cluster 0): the lowest-index core is 1 -> label 1, the HIGHER cluster
      10                 border of cores 2 (cluster 0) and 6 (cluster 2): lowest core 2 -> label 0
      11 -> 8 (at eps)  core: cluster 3 = {11} + its border 8 (nothing at all under dist < eps)"""
    idx = np.full((12, 3), -1, np.int32)
    dist = np.full((12, 3), np.inf, f32)
    rows = {0: [(2, 0.05)], 1: [(3, 0.05), (9, 0.02)], 2: [(0, 0.05), (10, 0.07)], 3: [(4, 0.01)], 4: [(3, EPS32)],
            5: [(0, 0.03), (9, 0.05)], 6: [(10, 0.05)], 7: [(7, 0.05)], 8: [(7, 0.5), (11, EPS_UP)], 9: [(0, 0.3)], 11: [(8, EPS32)]}
    for i, nb in rows.items():
        s0 = 1 if i in (6, 7) else 0                           # (a hole in front on two rows)
        for s, (j, d) in enumerate(nb):
            idx[i, s0 + s], dist[i, s0 + s] = j, f32(d)
    return idx, dist, None


def g_border_random():
    """the motifs of g_border at random: 20,000 rows, k = 9; two rows in five store nothing within eps (borders or noise),
    the others one or two eps-neighbours among the 8 rows to either side (many small clusters that share borders) plus
    far neighbours, holes and self slots, at random slots"""
    rng = np.random.default_rng(9)
    n, k = 20000, 9
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    near_d = np.array([0.05, EPS32, EPS_DOWN, 0.01], f32)
    far_d = np.array([0.5, EPS_UP, 0.11], f32)
    for i in range(n):
        lo, hi = max(0, i - 8), min(n, i + 9)
        pool = rng.permutation(np.setdiff1d(np.arange(lo, hi), [i]))
        n_near = 0 if i % 5 < 2 else (1 if rng.random() < 0.7 else 2)
        n_far = int(rng.integers(0, 3))
        slots = rng.permutation(k)
        c = n_near + n_far
        idx[i, slots[:c]] = pool[:c]
        dist[i, slots[:n_near]] = rng.choice(near_d, n_near)
        dist[i, slots[n_near:c]] = rng.choice(far_d, n_far)
        if i % 7 == 3:                                         # a self slot within eps
            idx[i, slots[c]], dist[i, slots[c]] = i, f32(0.05)
    return idx, dist, None


def g_hub(core0):
    """50,001 rows, k = 4; every row >= 1 names row 0 at eps (slot row mod 4).  core0: row 0 names row 1 -> one component of
    50,001 cores.  Else row 0 stores nothing -> a border with 50,000 votes; the rows also chain i -> i + 1 in runs of 50
    (1,000 clusters), so the votes come from 1,000 clusters and the lowest-index core, row 1, gives label 0."""
    n, k = 50001, 4
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    i = np.arange(1, n)
    idx[i, i % 4] = 0
    dist[i, i % 4] = EPS32
    if core0:
        idx[0, 3], dist[0, 3] = 1, EPS32
    else:
        link = i[(i % 50 != 0) & (i + 1 < n)]
        idx[link, (link + 1) % 4] = link + 1
        dist[link, (link + 1) % 4] = f32(0.05)
    return idx, dist, None


def g_count():
    """4,099 rows (not a multiple of 8), k = 16, rows front-packed with 0..16 stored neighbours among the 10 rows to either
    side, one in fourteen of them within eps (hundreds of clusters).  nb_count: on every third row BELOW the stored length (the slots behind it hold
    stored neighbours, every second within eps, that must not count); 0 on rows % 3 == 0 and % 5 == 0; k + 3 on full rows
    % 3 == 1; else the stored length."""
    rng = np.random.default_rng(16)
    n, k = 4099, 16
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    count = np.zeros(n, np.int32)
    for i in range(n):
        L = int(rng.integers(0, k + 1)) if i % 4 else k
        pool = np.setdiff1d(np.arange(max(0, min(i - 10, n - 21)), min(n, max(i + 11, 21))), [i])
        idx[i, :L] = rng.choice(pool, L, replace=False)
        dist[i, :L] = np.where(rng.random(L) < 0.07, rng.choice(np.array([0.05, EPS32, EPS_DOWN], f32), L),
                               rng.choice(np.array([0.5, EPS_UP], f32), L))
        count[i] = L
        if i % 3 == 0 and L > 0:
            count[i] = 0 if i % 5 == 0 else int(rng.integers(0, L))
            dist[i, count[i]:L:2] = f32(0.05)
        elif i % 3 == 1 and L == k:
            count[i] = k + 3
    return idx, dist, count


def graph_names():
    return ([f"slots{k}" for k in G_SLOT_K] + [f"slots{k}p" for k in G_SLOT_K]
            + ["eps", "border", "border_random", "hub_core", "hub_border", "count"])


@functools.lru_cache(maxsize=None)
def graph_input(name):
    """-> idx, dist, nb_count or None of the G input `name`"""
    if name.startswith("slots"):
        return g_slots(int(name[5:].rstrip("p")), name.endswith("p"))
    return {"eps": g_eps, "border": g_border, "border_random": g_border_random, "hub_core": lambda: g_hub(True),
            "hub_border": lambda: g_hub(False), "count": g_count}[name]()


def graph_catches(name):
    """the DBSCAN variants the G input is built to tell from the rule"""
    if name.startswith("slots") or name in ("eps", "hub_core"):
        return ("lt",)                                        # every edge of the slot inputs and of hub_core is AT eps
    return {"border": ("lt", "self_core", "highest", "lowest_cluster"),
            "border_random": ("lt", "self_core", "highest", "lowest_cluster"),
            "hub_border": ("lt", "highest"),
            "count": ("lt", "past_count", "highest", "lowest_cluster")}[name]


def tile_table(sizes, tile_rows):
    """row offsets of the bucket tiles of `fal_cluster_graph_tiled` for buckets of these sizes, none beyond the library's
    largest tile: consecutive whole buckets; a bucket that would take the open tile over `tile_rows` closes it, unless the
    tile is empty (test_tiles_cpu.py holds this against the library's builder)"""
    rows, start, pos = [0], 0, 0
    for s in sizes:
        if pos + s - start > tile_rows and pos > start:
            rows.append(pos)
            start = pos
        pos += int(s)
    if pos > start:
        rows.append(pos)
    return np.array(rows, np.int64)


def tile_eps_edges(idx, dist, nb_count, tile_rows, eps):
    """eps-edges per tile as `tile_dbscan_kernel` counts them for its edge list: a slot below min(nb_count, k) that holds a row
    of the row's own tile other than the row itself at float32 dist <= float32 eps; the same id twice in a row counts per slot"""
    n, k = idx.shape
    tile_rows = np.asarray(tile_rows, np.int64)
    tile = np.searchsorted(tile_rows, np.arange(n), side="right") - 1
    lo, hi = tile_rows[tile][:, None], tile_rows[tile + 1][:, None]
    stored = np.arange(k)[None, :] < np.minimum(np.asarray(nb_count), k)[:, None]
    j = idx.astype(np.int64)
    edge = stored & (j >= lo) & (j < hi) & (j != np.arange(n)[:, None]) & (dist <= f32(eps))
    return np.bincount(tile, weights=edge.sum(1), minlength=len(tile_rows) - 1).astype(np.int64)


_NEAR = np.array([0.05, EPS32, EPS_DOWN, 0.01], f32)
_FAR = np.array([0.5, EPS_UP, 0.11], f32)


def _store_row(rng, idx, dist, i, lo, m, e, f):
    """row i of a bucket [lo, lo + m): e + f distinct other rows of the bucket front-packed in random order, e of them within
    EPS and f beyond -> the stored length"""
    c = e + f
    t = rng.choice(m - 1, c, replace=False) if c else np.zeros(0, np.int64)
    idx[i, :c] = lo + t + (t >= i - lo)
    d = rng.choice(_FAR, c)
    d[rng.permutation(c)[:e]] = rng.choice(_NEAR, e)
    dist[i, :c] = d
    return c


def density_graph(sizes, k, per_row, seed, hide=True):
    """front-packed random rows, a row's neighbours drawn from its WHOLE bucket; bucket b holds round(per_row[b] * rows)
    eps-edges at EPS the counts leave visible (fewer where its rows cannot store that many), unequally spread over the rows,
    next to up to three neighbours beyond eps a row.  hide: rows % 11 == 0 have nb_count 0 in front of stored neighbours (any
    number of them within eps) and full odd rows k + 2, as test_gpu_graph_tiled.bucket_graph has them.
    -> idx, dist, nb_count, splits"""
    rng = np.random.default_rng(seed)
    per_row = np.broadcast_to(np.asarray(per_row, f64), (len(sizes),))
    splits = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(splits[-1])
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    count = np.zeros(n, np.int32)
    for b, m in enumerate(sizes):
        lo, most = int(splits[b]), min(k, m - 1)
        rows = np.arange(lo, lo + m)
        hidden = (rows % 11 == 0) if hide else np.zeros(m, bool)
        vis = np.flatnonzero(~hidden)
        e = np.zeros(m, np.int64)
        if len(vis) and most > 0:
            E = min(int(round(per_row[b] * m)), len(vis) * most)
            e[vis] = E // len(vis)
            e[rng.choice(vis, E % len(vis), replace=False)] += 1
            for a, c in rng.choice(vis, (m, 2)):                # one edge from row a to row c: the total stays
                if e[a] > 0 and e[c] < most:
                    e[a] -= 1
                    e[c] += 1
        e[hidden] = rng.integers(0, most + 1, int(hidden.sum()))
        for li in range(m):
            i = lo + li
            c = _store_row(rng, idx, dist, i, lo, m, int(e[li]), int(min(most - e[li], rng.integers(0, 4))))
            count[i] = 0 if hidden[li] else (k + 2 if c == k and i % 2 else c)
    return idx, dist, count, splits


def cut_graph(m, k, n_core, n_border, n_edges, seed):
    """one bucket of m rows with EXACTLY n_edges eps-edges at EPS: n_core rows (rows 0 and m - 1 among them, the others
    anywhere) store them, as evenly as n_edges divides, to rows drawn from the core rows and n_border further rows (core ->
    core and core -> border edges); every other row is noise.  Rows % 3 == 0 with room keep one more row within eps BEHIND their
    count; neighbours beyond eps fill some of the slots left.  -> idx, dist, nb_count"""
    rng = np.random.default_rng(seed)
    chosen = np.concatenate([[0, m - 1], 1 + rng.choice(m - 2, n_core + n_border - 2, replace=False)])
    chosen[2:] = rng.permutation(chosen[2:])
    core = chosen[:n_core]
    idx = np.full((m, k), -1, np.int32)
    dist = np.full((m, k), np.inf, f32)
    count = np.zeros(m, np.int32)
    e = np.full(n_core, n_edges // n_core)
    e[rng.choice(n_core, n_edges % n_core, replace=False)] += 1
    assert e.min() >= 1 and e.max() <= min(k, len(chosen) - 1)
    for i, ei in zip(core.tolist(), e.tolist()):
        pool = chosen[chosen != i]
        f = int(min(k - ei, rng.integers(0, 3)))
        near = rng.choice(pool, ei, replace=False)
        t = np.concatenate([near, rng.choice(np.setdiff1d(np.arange(m), np.append(near, i)), f, replace=False)])
        d = np.concatenate([rng.choice(_NEAR, ei), rng.choice(_FAR, f)])
        o = rng.permutation(ei + f)
        idx[i, :ei + f], dist[i, :ei + f], count[i] = t[o], d[o], ei + f
        if i % 3 == 0 and ei + f < k:
            idx[i, ei + f], dist[i, ei + f] = rng.choice(pool), f32(0.05)
    return idx, dist, count


# =========================================================================== a10 refinement
def linkage_1d_ref(values, ppm, variant=None):
    """complete linkage of 1-D values: sort (stable), then m - 1 times merge the adjacent pair of segments with the smallest
    max(right) - min(left) (float32 difference; ppm: float32 division by min(left), float64 product with 10^6), the LEFTMOST
    of equal ones.  -> [(left node, right node, height)], leaves 0..m-1 are members, merge `it` makes node m + it.
    variants: "rightmost" (the rightmost of equal minima), "unstable" (equal values in reversed member order)."""
    v = np.asarray(values, f32)
    m = len(v)
    order = np.lexsort((-np.arange(m), v)) if variant == "unstable" else np.argsort(v, kind="stable")
    lo = [v[i] for i in order]
    hi = list(lo)
    node = [int(i) for i in order]
    Z = []
    for it in range(m - 1):
        best, bs = None, -1
        for s in range(len(node) - 1):
            d = f32(hi[s + 1] - lo[s])
            d = f64(f32(d / lo[s])) * 1e6 if ppm else f64(d)
            if best is None or d < best or (variant == "rightmost" and d == best):
                best, bs = d, s
        Z.append((node[bs], node[bs + 1], float(best)))
        hi[bs], node[bs] = hi[bs + 1], m + it
        del lo[bs + 1], hi[bs + 1], node[bs + 1]
    return Z


def fcluster_ref(Z, m, t, variant=None):
    """scipy's fcluster(Z, t, "distance") - 1 restated: depth-first from the root; a subtree whose largest height is <= t is
    one flat cluster; flat clusters are numbered in the order the walk meets them, and the walk of a node goes into its
    left child if that is a merge, then into its right child if that is a merge, and only then numbers the children that
    are leaves, left before right.  variant "lt": < t."""
    T = np.zeros(m, np.int32)
    if m == 1:
        return T
    top = [0.0] * len(Z)
    for i, (l, r, h) in enumerate(Z):
        top[i] = max(h, top[l - m] if l >= m else 0.0, top[r - m] if r >= m else 0.0)
    count = [0]

    def walk(node, number):
        l, r, _ = Z[node - m]
        if number is None and (top[node - m] < t if variant == "lt" else top[node - m] <= t):
            number = count[0]
            count[0] += 1
        for c in (l, r):
            if c >= m:
                walk(c, number)
        for c in (l, r):
            if c < m:
                if number is None:
                    T[c] = count[0]
                    count[0] += 1
                else:
                    T[c] = number
    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * m + 100))
    try:
        walk(2 * m - 2, None)
    finally:
        sys.setrecursionlimit(old)
    return T


def postprocess_ref(mz, rt, tol, mode, rt_tol, variant=None):
    """`_postprocess_cluster` on the members of ONE DBSCAN cluster (ascending row order) -> (sub labels int32[m]: -1 or
    0.., number of clusters kept).  Fewer than 2 members: noise.  a = flat cut of the m/z linkage at tol; with rt_tol: b = flat
    cut of the RT linkage, a = rank of 2 a + 3 b among its distinct values (the reference's combination: it COLLIDES, e.g.
    (3, 0) and (0, 2), on purpose here).  One flat cluster: all 0.  As many as members: all noise.  Else groups of one
    member are noise and the others are numbered by first occurrence.
    variants: linkage_1d_ref's and fcluster_ref's, "pairs" (true (a, b) pairs), "by_value" (kept groups numbered by ascending a)."""
    assert variant in (None,) + REFINE_VARIANTS
    m = len(mz)
    if m < 2:
        return np.full(m, -1, np.int32), 0
    a = fcluster_ref(linkage_1d_ref(mz, mode == "ppm", variant), m, tol, variant)
    if rt_tol is not None:
        b = fcluster_ref(linkage_1d_ref(rt, False, variant), m, rt_tol, variant)
        if variant == "pairs":
            a = np.unique(np.stack([a, b], 1), axis=0, return_inverse=True)[1].reshape(-1).astype(np.int32)
        else:
            a = np.unique(a * 2 + b * 3, return_inverse=True)[1].reshape(-1).astype(np.int32)
    n_flat = int(a.max()) + 1
    if n_flat == 1:
        return np.zeros(m, np.int32), 1
    if n_flat == m:
        return np.full(m, -1, np.int32), 0
    size = np.bincount(a, minlength=n_flat)
    number = {}
    for g in (sorted(a.tolist()) if variant == "by_value" else a.tolist()):
        if size[g] >= 2 and g not in number:
            number[g] = len(number)
    return np.array([number.get(g, -1) for g in a.tolist()], np.int32), len(number)


def refine_ref(db_labels, mz, rt, tol, mode, rt_tol, variant=None):
    """a10 over every DBSCAN cluster in id order (ids without members pass), members in ascending row order; kept clusters
    are numbered in (DBSCAN id, first occurrence) order.  -> labels int32[n], cluster count"""
    db_labels = np.asarray(db_labels)
    out = np.full(len(db_labels), -1, np.int32)
    total = 0
    for c in np.unique(db_labels[db_labels >= 0]).tolist():
        rows = np.flatnonzero(db_labels == c)
        sub, kept = postprocess_ref(mz[rows], None if rt is None else rt[rows], tol, mode, rt_tol, variant)
        out[rows] = np.where(sub >= 0, sub + total, -1)
        total += kept
    return out, total


def tie_share(Z):
    """share of the merges whose height equals another merge's height in the same dendrogram"""
    h = np.array([z[2] for z in Z])
    if len(h) == 0:
        return 0.0
    _, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
    return float(np.mean(cnt[inv.reshape(-1)] > 1))


R_SIZES = (2, 3, 63, 64, 65, 129, 200)
R_RUNS = {                                      # name -> (tol, mode, rt_tol): Da with the lattice's tolerances, ppm with the collision's
    "da": (0.5, "Da", None), "da_rt": (0.5, "Da", 8.0), "ppm": (20.0, "ppm", None), "ppm_rt": (20.0, "ppm", 5.0)}
LATTICE_J = np.array([0, 2, 4, 7, 9, 11, 14, 16, 18, 21, 22, 25, 27, 29, 32, 33])
"""the lattice's 16 distinct m/z steps of 0.25: four triples two steps apart (0.5 = the tolerance: two equal heights AT the
tolerance, where the leftmost minimum keeps {a, a + 2} and the rightmost {a + 2, a + 4}), two pairs one step apart, gaps of three"""
COLLISION_MZ = np.array([500, 500, 501, 501, 502, 502, 503, 503, 500, 500, 501, 501], f32)
COLLISION_RT = np.array([0, 0, 0, 0, 0, 0, 0, 0, 20, 20, 10, 10], f32)
COLLISION_LABELS = np.array([0, 0, 1, 1, 2, 2, 3, 3, 3, 3, 4, 4], np.int32)
"""`postprocess_ref(COLLISION_MZ, COLLISION_RT, 20, "ppm", 5)` by hand, members in the order written.  m/z: the equal values
merge first, then 502 | 503 (1,992 ppm, the smallest), 500 | 501 (2,000), the root (6,000); the walk goes left first:
500 -> 0, 501 -> 1, 502 -> 2, 503 -> 3, a = 0 0 1 1 2 2 3 3 0 0 1 1.  RT: 0 | 10 and 10 | 20 are both 10 apart, the leftmost
merges, the root is 20 high; the walk numbers RT 0 -> 0, RT 10 -> 1, RT 20 -> 2, b = 0 0 0 0 0 0 0 0 2 2 1 1.
2a + 3b = 0 0 2 2 4 4 6 6 6 6 5 5: (m/z 503, RT 0) and (m/z 500, RT 20) share the value 6.  Five groups, all of two or more
members, numbered by first occurrence."""


def _r_patterns(rng):
    """-> [(pattern name, m/z, RT)] one entry per DBSCAN cluster"""
    out = []
    hi_da = f32(510.0) + f32(0.5)
    hi_ppm, up_ppm = ppm_pair(600.0)
    for m in R_SIZES:
        out.append(("lattice", (500 + 0.25 * rng.choice(LATTICE_J, m)).astype(f32), (8.0 * rng.integers(0, 5, m)).astype(f32)))
        out.append(("dup_one", np.full(m, 501.0, f32), rng.choice(np.array([0, 8, 16, 40, 41], f32), m)))
        out.append(("dup_30ppm", rng.choice(np.array([502.0, 502.0 * (1 + 30e-6)], f32), m),
                    (8.0 * rng.integers(0, 3, m)).astype(f32)))
        inner = lambda lo, hi: np.concatenate([[lo, hi], rng.uniform(lo, hi, m - 2).astype(f32)]).astype(f32)
        rt_flat = np.full(m, 3.0, f32)
        out.append(("cut_da_at", inner(f32(510.0), hi_da), rt_flat))
        out.append(("cut_da_above", inner(f32(510.0), np.nextafter(hi_da, f32(np.inf))), rt_flat))
        out.append(("cut_ppm_at", inner(f32(600.0), hi_ppm), rt_flat))
        out.append(("cut_ppm_above", inner(f32(600.0), up_ppm), rt_flat))
    for m in (65, 129):
        apart = (520.0 + 1.0 * np.arange(m)).astype(f32)
        out.append(("apart", apart, (8.0 * rng.integers(0, 3, m)).astype(f32)))
        pair = apart.copy()
        pair[m // 2] = pair[m // 2 - 1]                       # one close pair: one survivor
        out.append(("apart_pair", pair, np.full(m, 1.0, f32)))
    out.append(("collision", COLLISION_MZ.copy(), COLLISION_RT.copy()))
    reps = 11                                                  # 130 members: the 12-member pattern tiled, two rows short
    out.append(("collision", np.tile(COLLISION_MZ, reps)[:130].copy(), np.tile(COLLISION_RT, reps)[:130].copy()))
    for _ in range(6):
        out.append(("single", np.array([505.0], f32), np.array([0.0], f32)))
    return out


@functools.lru_cache(maxsize=None)
def refine_input():
    """the ONE a10 call: every pattern of `_r_patterns` as a DBSCAN cluster, ids shuffled with every seventh id left
    without members and `n_clusters_in` four above the highest id, 40 noise rows, all rows sorted by m/z (ties at random:
    the clusters interleave).  -> labels int32[n], mz, rt, n_clusters_in, {cluster id: pattern name}"""
    rng = np.random.default_rng(10)
    pats = _r_patterns(rng)
    ids = [i for i in range(2 * len(pats)) if i % 7 != 3][:len(pats)]
    ids = rng.permutation(ids)
    lab = np.concatenate([np.full(len(p[1]), c, np.int32) for c, p in zip(ids, pats)] + [np.full(40, -1, np.int32)])
    mz = np.concatenate([p[1] for p in pats] + [rng.uniform(499, 650, 40).astype(f32)])
    rt = np.concatenate([p[2] for p in pats] + [np.zeros(40, f32)])
    o = np.lexsort((rng.random(len(mz)), mz))
    names = {int(c): p[0] for c, p in zip(ids, pats)}
    return lab[o], mz[o], rt[o], int(max(ids)) + 5, names


R_CATCHES = {
    # pattern -> variants it is built to catch (under at least one of the four run settings)
    "lattice": ("rightmost", "lt", "by_value", "pairs"),
    "dup_one": ("rightmost", "lt", "by_value"),        # RT 0 / 8 / 16: two heights AT rt_tol; 40 / 41 apart from them
    "dup_30ppm": ("rightmost", "lt", "by_value"),
    "cut_da_at": ("lt",),                 # max - min == tol: one cluster by the shortcut, none under <
    "cut_da_above": (),                   # exempt: the other side of the shortcut, it splits under every variant alike
    "cut_ppm_at": (),                     # exempt: the ppm pair BRACKETS 20 ppm, no height equals it
    "cut_ppm_above": (),
    "apart": ("lt", "pairs"),             # (through RT steps of rt_tol; without RT: n_flat == m above 64 members, under every variant)
    "apart_pair": (),
    "collision": ("by_value", "pairs"),
    "single": (),
}


@functools.lru_cache(maxsize=None)
def refine_reference(run):
    lab, mz, rt, _, _ = refine_input()
    tol, mode, rt_tol = R_RUNS[run]
    return refine_ref(lab, mz, rt, tol, mode, rt_tol)


# =========================================================================== a11 medoids, a12 labels
def medoid_scores_ref(labels, idx, dist, variant=None):
    """score of row i of cluster c = float32 sum, in slot order, of the stored distances to other rows of c, plus 1.0 for
    every other member of c the row does not store; noise rows +inf.
    variants: "f64" (the sum in float64, rounded once), "ascending" (summed by ascending distance), "missing0"."""
    labels = np.asarray(labels)
    n, k = idx.shape
    rows = np.arange(n)[:, None]
    member = labels >= 0
    same = (idx >= 0) & (idx != rows) & member[:, None] & (labels[np.where(idx < 0, 0, idx)] == labels[:, None])
    d = np.where(same, dist, 0).astype(f32)
    if variant == "ascending":
        d = np.sort(np.where(same, dist, np.inf).astype(f32), axis=1)
        d = np.where(np.isinf(d), f32(0), d)
    acc = np.zeros(n, f64 if variant == "f64" else f32)
    for s in range(k):
        acc = (acc + d[:, s]).astype(acc.dtype)                # adding 0.0 for the other slots changes no sum
    acc = acc.astype(f32)
    size = np.bincount(labels[member], minlength=1)[np.where(member, labels, 0)]
    missing = (size - 1 - same.sum(1)).astype(f32)
    if variant != "missing0":
        acc = (acc + missing).astype(f32)
    return np.where(member, acc, f32(np.inf)).astype(f32)


def labels_and_medoids(labels_sorted, score, order):
    """a11 / a12 from the per-row scores: medoid of cluster c = its member of the lowest (score, SORTED row), reported as a
    dataset row; labels by dataset row, the noise rows numbered n_clusters.. in dataset-row order and their own medoids.
    (the rule `test_gpu_pipeline._check_stages` states)  -> labels int32[n], medoids int32[n_labels]"""
    lab = np.asarray(labels_sorted)
    N = len(lab)
    n_cl = int(lab.max()) + 1 if N else 0
    member = lab >= 0
    safe = np.where(member, lab, 0)
    o = np.lexsort((np.arange(N), score, safe))
    o = o[member[o]]
    first = np.concatenate([[True], safe[o][1:] != safe[o][:-1]]) if len(o) else np.zeros(0, bool)
    ref_labels = np.empty(N, np.int32)
    ref_labels[order] = lab
    noise = ref_labels == -1
    ref_labels[noise] = np.arange(n_cl, n_cl + noise.sum())
    ref_med = np.concatenate([np.asarray(order)[o[first]], np.flatnonzero(noise)]).astype(np.int32)
    return ref_labels, ref_med


def finalize_ref(labels_sorted, n_clusters, order, idx, dist, variant=None):
    """a11 + a12, sequentially.  variants: medoid_scores_ref's, "tie_highest" (equal scores -> highest sorted row),
    "tie_dataset" (-> lowest DATASET row), "noise_sorted" (noise numbered in sorted-row order)."""
    assert variant in (None,) + MEDOID_VARIANTS + LABEL_VARIANTS
    lab = np.asarray(labels_sorted)
    n = len(lab)
    score = medoid_scores_ref(lab, idx, dist, variant)
    best = [None] * n_clusters
    for i in range(n):
        c = int(lab[i])
        if c < 0:
            continue
        tie = -i if variant == "tie_highest" else (int(order[i]) if variant == "tie_dataset" else i)
        key = (float(score[i]), tie, i)
        if best[c] is None or key < best[c]:
            best[c] = key
    labels = np.empty(n, np.int32)
    noise_rows = []
    for i in range(n):
        if lab[i] >= 0:
            labels[order[i]] = lab[i]
        else:
            noise_rows.append(int(order[i]))
    if variant != "noise_sorted":
        noise_rows.sort()
    for r, ds in enumerate(noise_rows):
        labels[ds] = n_clusters + r
    medoids = np.array([int(order[b[2]]) for b in best] + noise_rows, np.int32).reshape(-1)
    return labels, medoids


def _scatter_clusters(rng, sizes, n_noise):
    """rows dealt to clusters of the given sizes at random; clusters numbered by their lowest row (the contract of a9/a10)"""
    n = sum(sizes) + n_noise
    lab = np.concatenate([np.full(s, c, np.int32) for c, s in enumerate(sizes)] + [np.full(n_noise, -1, np.int32)])
    lab = lab[rng.permutation(n)]
    first = {}
    for v in lab.tolist():
        if v >= 0:
            first.setdefault(v, len(first))
    return np.array([first.get(v, -1) for v in lab.tolist()], np.int32)


def m_cliques():
    """cliques of 2..40 rows, rows interleaved, k = 40: every member stores every other at 0.25 -> all scores of a cluster
    are equal ((m - 1) / 4, exact); 9 noise rows"""
    rng = np.random.default_rng(40)
    lab = _scatter_clusters(rng, list(range(2, 41)), 9)
    n, k = len(lab), 40
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    for c in range(int(lab.max()) + 1):
        rows = np.flatnonzero(lab == c)
        for i in rows:
            nb = rng.permutation(rows[rows != i])
            idx[i, :len(nb)], dist[i, :len(nb)] = nb, f32(0.25)
    return lab, idx, dist


def m_float_order():
    """60 clusters {B, A, C, D} on ascending rows B < A, k = 8.  A stores (B 0.5, C 2^-25, D 2^-25): in float32 and slot
    order 0.5 + 2^-25 + 2^-25 = 0.5 (each addend is half an ulp, ties to even).  B stores (C 2^-25, D 2^-25, A 0.5):
    2^-24 + 0.5 = 0.5 + 2^-24.  C and D store nothing (score 3).  A is the medoid; a float64 sum or an ascending sum gives
    A and B the same score and the lower row B."""
    rng = np.random.default_rng(25)
    lab = _scatter_clusters(rng, [4] * 60, 5)
    n, k = len(lab), 8
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    t = f32(2.0 ** -25)
    for c in range(60):
        B, A, C, D = np.flatnonzero(lab == c)
        idx[A, :3], dist[A, :3] = [B, C, D], [0.5, t, t]
        idx[B, 1:4], dist[B, 1:4] = [C, D, A], [t, t, 0.5]
    return lab, idx, dist


def m_wide(k):
    """k = 65 / 130: 301 rows, clusters of 2..7 rows; slots 0..63 of every member hold rows of OTHER clusters, noise rows
    and the row itself (none of which count); its cluster's other members sit in slots 64.. with random distances"""
    rng = np.random.default_rng(k)
    sizes = [int(s) for s in rng.integers(2, 8, 60)]
    lab = _scatter_clusters(rng, sizes, 301 - sum(sizes))
    n = len(lab)
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    for i in range(n):
        foreign = np.flatnonzero((lab != lab[i]) | (lab < 0))
        foreign = foreign[foreign != i]
        front = rng.choice(foreign, 64, replace=False)
        front[rng.integers(0, 64)] = i
        idx[i, :64], dist[i, :64] = front, rng.random(64).astype(f32)
        if lab[i] >= 0:
            mates = np.flatnonzero(lab == lab[i])
            mates = rng.permutation(mates[mates != i])[:k - 64]
            if i % 3 == 0:
                mates = mates[:-1]                             # one member not stored (at k = 65: none stored): + 1.0
            idx[i, 64:64 + len(mates)], dist[i, 64:64 + len(mates)] = mates, rng.random(len(mates)).astype(f32)
    return lab, idx, dist


def m_big():
    """one cluster of 5,000 rows and 37 noise rows, k = 8: every member stores 8 others at random distances, so every score
    is 4,991 + a sum of eight distances from {0.25, 0.5}: the 1.0-per-missing-member term dominates and about twenty rows
    share the lowest score, 4,993; every fifth row stores seven"""
    rng = np.random.default_rng(5000)
    lab = _scatter_clusters(rng, [5000], 37)
    n, k = len(lab), 8
    rows = np.flatnonzero(lab == 0)
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    for i in rows:
        nb = rng.choice(rows, k + 1, replace=False)
        idx[i], dist[i] = nb[nb != i][:k], rng.choice(np.array([0.25, 0.5], f32), k)
        if i % 5 == 0:
            idx[i, k - 1], dist[i, k - 1] = -1, np.inf         # seven stored: 1.75 + 4,992 loses to 2.0 + 4,991
    return lab, idx, dist


def m_all_noise():
    rng = np.random.default_rng(3)
    n, k = 300, 4
    idx = rng.integers(0, n, (n, k)).astype(np.int32)
    idx[idx == np.arange(n)[:, None]] = -1
    for i in range(n):                                          # distinct ids within a row
        _, firsts = np.unique(idx[i], return_index=True)
        dup = np.setdiff1d(np.arange(k), firsts)
        idx[i, dup] = -1
    dist = np.where(idx >= 0, f32(0.9), f32(np.inf)).astype(f32)
    return np.full(n, -1, np.int32), idx, dist


def m_one_cluster():
    rng = np.random.default_rng(257)
    n, k = 257, 6
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, f32)
    for i in range(n):
        c = k - 1 if i % 9 == 0 else k
        idx[i, :c] = rng.choice(np.delete(np.arange(n), i), c, replace=False)
        dist[i, :c] = rng.choice(np.array([0.125, 0.25], f32), c)      # a handful of rows share the lowest score
    return np.zeros(n, np.int32), idx, dist


def m_one_row(noise):
    return (np.array([-1 if noise else 0], np.int32), np.full((1, 3), -1, np.int32), np.full((1, 3), np.inf, f32))


M_BUILDERS = {"cliques": m_cliques, "float_order": m_float_order, "wide65": lambda: m_wide(65), "wide130": lambda: m_wide(130),
              "big": m_big, "all_noise": m_all_noise, "one_cluster": m_one_cluster,
              "one_row_noise": lambda: m_one_row(True), "one_row_cluster": lambda: m_one_row(False)}
M_CATCHES = {
    "cliques": ("tie_highest", "tie_dataset", "noise_sorted"),
    "float_order": ("f64", "ascending", "missing0", "noise_sorted"),
    "wide65": ("missing0", "noise_sorted"),
    "wide130": ("missing0", "noise_sorted"),
    "big": ("tie_highest", "tie_dataset", "missing0", "noise_sorted"),
    "all_noise": ("noise_sorted",),
    "one_cluster": ("missing0",),
    "one_row_noise": (),                  # exempt: one row is the shape itself, it separates no rule
    "one_row_cluster": (),
}


def medoid_names():
    return list(M_BUILDERS)


@functools.lru_cache(maxsize=None)
def medoid_input(name):
    """-> labels_sorted int32[n] (dense ids, every id with a member), n_clusters, row_order int64[n] (a random permutation),
    idx, dist"""
    lab, idx, dist = M_BUILDERS[name]()
    order = np.random.default_rng(len(lab)).permutation(len(lab)).astype(np.int64)
    return lab, int(lab.max()) + 1 if len(lab) else 0, order, idx, dist


@functools.lru_cache(maxsize=None)
def medoid_reference(name):
    lab, n_cl, order, idx, dist = medoid_input(name)
    return finalize_ref(lab, n_cl, order, idx, dist)


# =========================================================================== the chain a9 -> a10 -> a11 / a12
def chain_names():
    return ["G:" + g for g in graph_names()] + ["M:" + m for m in medoid_names()]


@functools.lru_cache(maxsize=None)
def chain_input(name):
    """a G or M graph as the fused calls take it -> idx, dist, nb_count (the input's own, or k on every row: nothing cut),
    own_count (whether the counts cut anything), eps, mz (one value: a10 splits nothing under WIDE), row_order"""
    if name.startswith("G:"):
        idx, dist, count = graph_input(name[2:])
        eps = EPS
    else:
        _, _, _, idx, dist = medoid_input(name[2:])
        count, eps = None, M_EPS
    n, k = idx.shape
    own = count is not None and bool(np.any(np.minimum(count, k) < k))
    if count is None:
        count = np.full(n, k, np.int32)
    order = np.random.default_rng(n + 1).permutation(n).astype(np.int64)
    return idx, dist, count, own, eps, np.full(n, 500.0, f32), order


@functools.lru_cache(maxsize=None)
def chain_reference(name, counted):
    """-> labels, medoids, labels_sorted, n_clusters, (db labels, db count) of the whole tail on `chain_input(name)`;
    counted: on the graph cut at nb_count"""
    idx, dist, count, _, eps, mz, order = chain_input(name)
    if counted:
        idx, dist = cut_at_count(idx, dist, count)
    db, n_db = dbscan_ref(idx, dist, eps)
    # one m/z under WIDE: a10 splits nothing and drops the clusters of one row (test_tail_cpu.py holds this against
    # `refine_ref` wherever the clusters are small enough for its quadratic loops)
    lab = drop_single_member_clusters(db)
    n_cl = int(lab.max()) + 1
    labels, medoids = finalize_ref(lab, n_cl, order, idx, dist)
    return labels, medoids, lab, n_cl, (db, n_db)


@functools.lru_cache(maxsize=None)
def single_linkage_agrees(name):
    """whether single linkage at eps gives the labels DBSCAN + a10 give on this graph (no border joins two clusters, no
    border below its cluster's lowest core): only then may `cluster_graph(linkage="single")` be held to `chain_reference`"""
    idx, dist, _, _, eps, _, _ = chain_input(name)
    return bool(np.array_equal(single_linkage_ref(idx, dist, eps), chain_reference(name, False)[2]))
