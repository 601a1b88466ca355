"""Molecular families (`fal_network_families`, csrc/netfamily.h; DESIGN.md "Molecular families"): the rule restated in numpy, and
the graphs the CPU and GPU tests share.

The rule.  n nodes, m edges (u, v, sim float32 >= 0, finite); every edge starts alive (round 0).  A pass takes the components of
the alive edges; root(x) is the smallest node of x's component, size(x) its node count.  With max_size 0, or no component above
max_size, the passes end.  Otherwise the pass is cutting round r = 1, 2, ...: for every oversized component, lo = the smallest
sim among its alive edges, and its alive edges with float64(sim) <= float64(lo) + delta get round r.  Components of two or more
nodes are numbered 0, 1, ... by ascending root; every other node has family -1 and size 1."""
import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32


def components(n, u, v):
    """-> root i32[n]: the smallest node of every node's component (hooking under the smaller label, then pointer jumping)"""
    lab = np.arange(n, dtype=np.int64)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    while len(u):
        new = lab.copy()
        low = np.minimum(lab[u], lab[v])
        for at in (u, v, lab[u], lab[v]):
            np.minimum.at(new, at, low)
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    return lab.astype(i32)


def valid(n, u, v, sim, max_size, delta):
    u, v, sim = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(sim, f32)
    return bool(max_size >= 0 and delta >= 0 and ((u >= 0) & (u < n) & (v >= 0) & (v < n) & (u != v)).all()
                and (np.isfinite(sim) & (sim >= 0)).all())


def families(n, u, v, sim, max_size=100, delta=0.02):
    """-> dict(family i32[n], size i32[n], round i32[m], n_families, n_rounds, n_cut, largest_before (the largest component of
    all the edges), largest (of the surviving ones), cut_per_round)"""
    assert valid(n, u, v, sim, max_size, delta)
    u, v, sim = np.asarray(u, i32), np.asarray(v, i32), np.asarray(sim, f32)
    rnd = np.zeros(len(u), i32)
    r, largest_before, cuts = 0, None, []
    while True:
        alive = rnd == 0
        root = components(n, u[alive], v[alive])
        size = np.bincount(root, minlength=n).astype(i32)[root] if n else np.zeros(0, i32)
        if largest_before is None:
            largest_before = int(size.max()) if n else 0
        over = (size > max_size) if max_size > 0 else np.zeros(n, bool)
        if not over.any():
            break
        r += 1
        e = np.flatnonzero(alive & over[u])
        lo = np.full(n, np.inf, f32)
        np.minimum.at(lo, root[u[e]], sim[e])
        cut = e[sim[e].astype(f64) <= lo[root[u[e]]].astype(f64) + f64(delta)]
        assert len(cut)
        rnd[cut] = r
        cuts.append(len(cut))
    is_family = (root == np.arange(n)) & (size >= 2)
    rank = np.cumsum(is_family) - is_family
    family = np.where(size >= 2, rank[root], -1).astype(i32)
    return dict(family=family, size=size, round=rnd, n_families=int(is_family.sum()), n_rounds=r, n_cut=int((rnd > 0).sum()),
                largest_before=largest_before, largest=int(size.max()) if n else 0, cut_per_round=cuts)


def same(got, want):
    """bit equality of the three arrays and the two counts"""
    return (all(np.asarray(got[k]).dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in ("family", "size", "round"))
            and got["n_families"] == want["n_families"] and got["n_rounds"] == want["n_rounds"])


def family_sets(res):
    """the families as a set of frozensets of nodes"""
    fam = res["family"]
    return {frozenset(np.flatnonzero(fam == f).tolist()) for f in range(res["n_families"])}


# ---- graphs: dict(n, u, v, sim) ------------------------------------------------------------------------------------------------
def graph(n, u, v, sim):
    return dict(n=int(n), u=np.asarray(u, i32), v=np.asarray(v, i32), sim=np.asarray(sim, f32))


def empty(n):
    return graph(n, [], [], [])


def random_graph(n, m, seed, grid=None):
    """m distinct pairs, sims uniform in [0.7, 1); `grid`: rounded to multiples of 1 / grid (many ties)"""
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < m:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    uv = np.array(sorted(pairs), i32)
    sim = rng.uniform(0.7, 1.0, m).astype(f32)
    if grid:
        sim = (np.round(sim * grid) / grid).astype(f32)
    return graph(n, uv[:, 0], uv[:, 1], sim)


def chain(n, seed=3):
    """node i -- node i + 1 with random sims: the union-find's trees are deep"""
    rng = np.random.default_rng(seed)
    return graph(n, np.arange(n - 1), np.arange(1, n), rng.uniform(0.7, 1.0, n - 1).astype(f32))


def star(leaves, seed=4, hub=0, strong=60):
    """every leaf hooks under one root; `strong` leaves hold on at 0.95 and above, the others lie below 0.9"""
    rng = np.random.default_rng(seed)
    other = np.array([x for x in range(leaves + 1) if x != hub], i32)
    sim = np.concatenate([rng.uniform(0.7, 0.9, leaves - strong), rng.uniform(0.95, 1.0, strong)])[rng.permutation(leaves)]
    return graph(leaves + 1, np.minimum(other, hub), np.maximum(other, hub), sim.astype(f32))


def two_cliques(k=10, inside=0.9, bridge=0.71):
    """two k-cliques joined by one weaker edge"""
    u, v, s = [], [], []
    for base in (0, k):
        for a in range(k):
            for b in range(a + 1, k):
                u.append(base + a), v.append(base + b), s.append(inside)
    u.append(k - 1), v.append(k), s.append(bridge)
    return graph(2 * k, u, v, s)


def equal_sims(n=30, sim=0.8, seed=6):
    """one connected component of n nodes (a random tree and some more edges) whose edges all share one sim, and a pair beside it"""
    rng = np.random.default_rng(seed)
    u = [int(rng.integers(0, b)) for b in range(1, n)] + [0, 3, 5]
    v = list(range(1, n)) + [7, 11, 13]
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    return graph(n + 2, np.append(lo, n), np.append(hi, n + 1), [sim] * len(u) + [0.75])


def shuffled(g, seed=7, duplicates=0):
    """the same graph with its edges in another order, the first `duplicates` of them twice, some with their ends swapped"""
    rng = np.random.default_rng(seed)
    pick = np.concatenate([np.arange(len(g["u"])), np.arange(duplicates)])
    pick = pick[rng.permutation(len(pick))]
    swap = rng.random(len(pick)) < 0.5
    u, v = g["u"][pick], g["v"][pick]
    return graph(g["n"], np.where(swap, v, u), np.where(swap, u, v), g["sim"][pick]), pick


def permuted(g, seed=8):
    """node x of `g` becomes node perm[x] -> (graph, perm)"""
    perm = np.random.default_rng(seed).permutation(g["n"]).astype(i32)
    return graph(g["n"], perm[g["u"]], perm[g["v"]], g["sim"]), perm


def edge_cases():
    """what the rule accepts at its edges, for cap 3 and delta 0: a chain of four nodes (max_size + 1: cut) with sims -0.0 (the key
    of +0), 0 and a subnormal -- both zeros go, the subnormal stays; a chain of three (max_size: untouched) with the largest
    float32; a chain of four with equal sims (dissolves); a node without an edge"""
    sims = [-0.0, 0.0, 1e-45, 3.4028235e38, 0.5, 0.5, 0.5, 0.5]
    return graph(12, [0, 1, 2, 4, 5, 7, 8, 9], [1, 2, 3, 5, 6, 8, 9, 10], sims)


# name -> (graph, max_size, delta, expectations on the restatement's result); the GPU and CPU tests run every one
def _cases():
    r300, r5000, ch, st, cl, eq = random_graph(300, 450, 1), random_graph(5000, 7000, 2), chain(3000), star(2000), two_cliques(), equal_sims()
    out = {f"empty-{n}": (empty(n), 100, 0.02, lambda s: s["n_families"] == 0 and s["n_rounds"] == 0) for n in (1, 2, 255, 256, 257)}
    out.update({
        "one-edge": (graph(2, [0], [1], [0.9]), 100, 0.02, lambda s: s["n_families"] == 1 and s["n_cut"] == 0),
        "one-edge-cap-1": (graph(5, [3], [1], [0.9]), 1, 0.02, lambda s: s["n_families"] == 0 and s["n_cut"] == 1),
        "random-300": (r300, 20, 0.02, lambda s: s["n_rounds"] >= 5 and s["largest_before"] >= 200 and s["largest"] <= 20),
        "random-300-delta-0": (r300, 20, 0.0, lambda s: s["n_rounds"] >= 200 and s["largest"] <= 20),
        "random-300-grid": (random_graph(300, 450, 1, grid=20), 20, 0.0,
                            lambda s: 2 <= s["n_rounds"] <= 7 and max(s["cut_per_round"]) >= 30),
        "random-5000": (r5000, 100, 0.02, lambda s: s["n_rounds"] >= 5 and s["largest_before"] >= 1000 and s["n_families"] >= 100),
        "chain-cap-0": (ch, 0, 0.02, lambda s: s["n_families"] == 1 and s["largest"] == 3000 and s["n_rounds"] == 0),
        "chain-cap-3000": (ch, 3000, 0.0, lambda s: s["n_cut"] == 0 and s["largest"] == 3000),
        "chain-cap-2999": (ch, 2999, 0.0, lambda s: s["n_cut"] == 1 and s["n_rounds"] == 1),
        "chain-cap-64": (ch, 64, 0.0, lambda s: s["n_rounds"] >= 8 and s["largest"] <= 64 and s["n_families"] >= 40),
        "star-cap-0": (st, 0, 0.02, lambda s: s["n_families"] == 1 and s["largest"] == 2001),
        "star-cap-100": (st, 100, 0.02, lambda s: s["n_rounds"] >= 5 and s["largest"] == 61 and s["n_families"] == 1),
        "cliques-cap-10": (cl, 10, 0.02, lambda s: s["n_cut"] == 1 and s["n_families"] == 2 and s["n_rounds"] == 1),
        "cliques-cap-19": (cl, 19, 0.02, lambda s: s["n_cut"] == 1 and s["n_families"] == 2),
        "cliques-cap-20": (cl, 20, 0.02, lambda s: s["n_cut"] == 0 and s["n_families"] == 1),
        "equal-sims": (eq, 10, 0.0, lambda s: s["n_rounds"] == 1 and s["n_cut"] == len(eq["u"]) - 1 and s["n_families"] == 1
                       and s["largest_before"] == 30),
        "duplicates-shuffled": (shuffled(r300, duplicates=40)[0], 20, 0.02, lambda s: s["n_rounds"] >= 5),
        "permuted": (permuted(r300)[0], 20, 0.02, lambda s: s["n_rounds"] >= 5),
        "edge-values": (edge_cases(), 3, 0.0, lambda s: s["n_cut"] == 5 and s["n_rounds"] == 1 and s["n_families"] == 2
                        and s["round"].tolist() == [1, 1, 0, 0, 0, 1, 1, 1] and s["size"][4:7].tolist() == [3, 3, 3]),
    })
    return out


CASES = _cases()
_results = {}


def expected(name):
    """the restatement's result for a case, computed once and shared (nobody writes into it)"""
    if name not in _results:
        g, max_size, delta, holds = CASES[name]
        res = families(g["n"], g["u"], g["v"], g["sim"], max_size, delta)
        assert holds(res), (name, {k: v for k, v in res.items() if not isinstance(v, np.ndarray)})
        for k in ("family", "size", "round"):
            res[k].setflags(write=False)
        _results[name] = res
    return _results[name]


# every input the call refuses: name -> (graph, max_size, delta)
def invalid_cases():
    g = random_graph(40, 60, 11)

    def with_edge(e, u=None, v=None, sim=None):
        h = graph(g["n"], g["u"].copy(), g["v"].copy(), g["sim"].copy())
        for k, x in (("u", u), ("v", v), ("sim", sim)):
            if x is not None:
                h[k][e] = x
        return h
    return {"u-negative": (with_edge(5, u=-1), 100, 0.02), "v-is-n": (with_edge(59, v=40), 100, 0.02),
            "u-far-outside": (with_edge(0, u=2 ** 31 - 1), 100, 0.02), "loop": (with_edge(17, u=9, v=9), 100, 0.02),
            "sim-nan": (with_edge(3, sim=np.nan), 100, 0.02), "sim-inf": (with_edge(3, sim=np.inf), 100, 0.02),
            "sim-negative": (with_edge(30, sim=-0.25), 100, 0.02), "max-size-negative": (g, -1, 0.02),
            "delta-negative": (g, 100, -0.01), "delta-nan": (g, 100, float("nan"))}
