"""Annotation propagation (`fal_network_propagate`, csrc/netpropagate.h; DESIGN.md "Annotation propagation"): the rule restated in
numpy, and the graphs the CPU and GPU tests share.

The rule.  n nodes, m undirected links (u, v, sim float32 >= 0, finite), seed int32[n] (>= 0: annotated, -1: not), max_hops in
[1, 64], min_score in [0, 1].  Level 0: every annotated node has hops 0, source itself, parent -1, score 1.  Level d = 1 ..
max_hops in this order: a link {a, b} with hops[a] == d - 1 and b not yet reached offers b the candidate (a, c = float32(score[a]
* sim)); it counts when c >= float32(min_score); a node with a counting candidate takes the greatest c, equal c the lowest a, and
has hops d, parent a, source source[a], score c (a zero of either sign is +0).  A node never reached: source, hops, parent -1,
score 0."""
import numpy as np

from tests import family_cases as fc

f32, f64, i32 = np.float32, np.float64, np.int32
graph = fc.graph


def valid(n, u, v, sim, seed, max_hops, min_score):
    u, v, sim = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(sim, f32)
    return bool(1 <= max_hops <= 64 and 0.0 <= min_score <= 1.0 and (np.asarray(seed, np.int64) >= -1).all()
                and ((u >= 0) & (u < n) & (v >= 0) & (v < n) & (u != v)).all() and (np.isfinite(sim) & (sim >= 0)).all())


def propagate(n, u, v, sim, seed, max_hops=3, min_score=0.0, stats=True):
    """-> dict(source, hops, parent i32[n], score f32[n], n_reached, n_levels; and the statistics tied (nodes whose best score
    two parents offered), tied_sources (those whose two best parents carry different sources); stats=False leaves both 0)"""
    assert valid(n, u, v, sim, seed, max_hops, min_score)
    u, v, sim, seed = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(sim, f32), np.asarray(seed, i32)
    assert len(seed) == n
    annotated = seed >= 0
    hops = np.where(annotated, 0, -1).astype(i32)
    source = np.where(annotated, np.arange(n), -1).astype(i32)
    parent = np.full(n, -1, i32)
    score = np.where(annotated, 1, 0).astype(f32)
    ends_a, ends_b, sims = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([sim, sim])     # both directions
    floor = f32(min_score)
    n_levels = tied = tied_sources = 0
    for d in range(1, max_hops + 1):
        pick = np.flatnonzero((hops[ends_a] == d - 1) & (hops[ends_b] == -1))
        a, b = ends_a[pick], ends_b[pick]
        with np.errstate(over="ignore", invalid="ignore"):
            c = (score[a] * sims[pick]).astype(f32)
        c = np.where(c == 0, f32(0), c)                    # -0 -> +0
        ok = c >= floor                                    # (a NaN fails)
        a, b, c = a[ok], b[ok], c[ok]
        if len(b) == 0:
            break
        with np.errstate(invalid="ignore"):
            order = np.lexsort((a, -c.astype(f64), b))     # per b: greatest c first, then lowest a
        a, b, c = a[order], b[order], c[order]
        first = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
        # statistics: the first offer of another parent at the same score (duplicates of one link repeat a parent)
        last = np.r_[first[1:], len(b)]
        for lo, hi in zip(first, last) if stats else ():
            same = a[lo:hi][c[lo:hi] == c[lo]]
            others = same[same != same[0]]
            if len(others):
                tied += 1
                tied_sources += bool((source[others] != source[same[0]]).any())
        node, par = b[first], a[first]
        hops[node], parent[node], score[node] = d, par, c[first]
        source[node] = source[par]
        n_levels = d
    return dict(source=source, hops=hops, parent=parent, score=score, n_reached=int((hops >= 1).sum()), n_levels=n_levels,
                tied=tied, tied_sources=tied_sources)


ARRAYS = ("source", "hops", "parent", "score")


def same(got, want):
    """bit equality of the four arrays and the two counts"""
    return (all(np.asarray(got[k]).dtype == want[k].dtype and np.asarray(got[k]).shape == want[k].shape
                and np.array_equal(np.asarray(got[k]).view(i32), want[k].view(i32)) for k in ARRAYS)
            and got["n_reached"] == want["n_reached"] and got["n_levels"] == want["n_levels"])


def bfs_hops(n, u, v, seed, max_hops):
    """breadth-first distance from the annotated nodes, -1 beyond max_hops or out of reach"""
    hops = np.where(np.asarray(seed) >= 0, 0, -1).astype(i32)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    for d in range(1, max_hops + 1):
        nxt = np.concatenate([v[(hops[u] == d - 1) & (hops[v] == -1)], u[(hops[v] == d - 1) & (hops[u] == -1)]])
        if len(nxt) == 0:
            break
        hops[nxt] = d
    return hops


# ---- graphs and seeds ------------------------------------------------------------------------------------------------------------
def seeds(n, nodes):
    """seed[n]: node x of `nodes` carries the value 100 + x (the call does not interpret it), everything else -1"""
    s = np.full(n, -1, i32)
    nodes = np.asarray(nodes, np.int64)
    s[nodes] = 100 + nodes
    return s


def chain(n):
    """node i -- node i + 1; the sims cycle through 0.75, 0.875, 1.0 (every running product is exact in float32 up to 9 nodes)"""
    return graph(n, np.arange(n - 1), np.arange(1, n), np.array([0.75, 0.875, 1.0], f32)[np.arange(n - 1) % 3])


def triangle(sv, sa, av):
    """s = 0, a = 1, v = 2"""
    return graph(3, [0, 0, 1], [2, 1, 2], [sv, sa, av])


def star(n, hub=0, sim=0.75):
    other = np.array([x for x in range(n) if x != hub], i32)
    return graph(n, np.full(n - 1, hub), other, np.full(n - 1, sim, f32))


def ring(n, m=None):
    """a ring of n nodes; `m` > n: its links repeated in order until there are m"""
    e = np.arange(n if m is None else m) % n
    return graph(n, e, (e + 1) % n, np.array([0.875, 1.0, 0.75, 1.0], f32)[e % 4])


def random_graph(n, m, n_seeds, seed=5):
    """m drawn pairs with the self-loops dropped (duplicates stay), sims from {0.75, 0.875, 1.0}: every product is exact, and
    ties occur -> (graph, seed array)"""
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    sim = rng.choice(np.array([0.75, 0.875, 1.0], f32), m)
    keep = u != v
    return graph(n, u[keep], v[keep], sim[keep]), seeds(n, rng.choice(n, n_seeds, replace=False))


def shuffled(g, seed=7, duplicates=0):
    """family_cases.shuffled: another link order, the first `duplicates` links twice, some with their ends swapped"""
    return fc.shuffled(g, seed, duplicates)[0]


def permuted(g, s, seed=8):
    """node x becomes node perm[x] -> (graph, seed array, perm)"""
    h, perm = fc.permuted(g, seed)
    t = np.empty_like(s)
    t[perm] = s
    return h, t, perm


# name -> (graph, seed, max_hops, min_score, expectations on the restatement's result); the GPU and CPU tests run every one
def _cases():
    ch, tri = chain(9), triangle
    prod = np.cumprod(np.concatenate([[1.0], chain(9)["sim"]]).astype(f32), dtype=f32)
    detour = tri(0.5, 0.9, 0.9)
    out = {
        "chain-9": (ch, seeds(9, [0]), 8, 0.0, lambda r: r["hops"].tolist() == list(range(9)) and np.array_equal(r["score"], prod)
                    and r["parent"].tolist() == [-1] + list(range(8)) and (r["source"] == 0).all() and r["n_levels"] == 8),
        "chain-9-hops-1": (ch, seeds(9, [0]), 1, 0.0, lambda r: r["hops"].tolist() == [0, 1] + [-1] * 7 and r["n_reached"] == 1),
        "chain-9-hops-7": (ch, seeds(9, [0]), 7, 0.0, lambda r: r["hops"].tolist() == list(range(8)) + [-1] and r["n_reached"] == 7
                           and r["score"][8] == 0 and r["source"][8] == -1),
        "two-seeds-tie": (graph(3, [0, 1], [1, 2], [0.75, 0.75]), seeds(3, [0, 2]), 3, 0.0,
                          lambda r: r["parent"][1] == 0 and r["source"].tolist() == [0, 0, 2] and r["tied_sources"] == 1),
        "level-beats-score": (tri(0.75, 1.0, 1.0), seeds(3, [0]), 3, 0.0,
                              lambda r: r["hops"].tolist() == [0, 1, 1] and r["score"][2] == f32(0.75) and r["parent"][2] == 0),
        "min-score-detour": (detour, seeds(3, [0]), 3, 0.6, lambda r: r["hops"].tolist() == [0, 1, 2] and r["parent"][2] == 1
                             and r["score"][2] == f32(f32(0.9) * f32(0.9))),
        "min-score-stops": (detour, seeds(3, [0]), 3, 0.85, lambda r: r["hops"].tolist() == [0, 1, -1] and r["n_reached"] == 1),
        "duplicates": (graph(2, [0, 1, 0], [1, 0, 1], [0.75, 0.875, 0.5]), seeds(2, [0]), 3, 0.0, lambda r: r["score"][1] == f32(0.875)),
        "zero-sim": (graph(4, [0, 1, 2], [1, 2, 3], [0.0, -0.0, 1.0]), seeds(4, [0]), 3, 0.0,
                     lambda r: r["hops"].tolist() == [0, 1, 2, 3] and not r["score"][1:].any() and not np.signbit(r["score"]).any()),
        "sim-above-one": (graph(3, [0, 1], [1, 2], [1.5, 3.0e38]), seeds(3, [0]), 3, 1.0,
                          lambda r: r["score"][1] == f32(1.5) and np.isinf(r["score"][2]) and r["n_reached"] == 2),
        "no-seed": (ch, seeds(9, []), 3, 0.0, lambda r: r["n_reached"] == 0 and r["n_levels"] == 0 and (r["hops"] == -1).all()),
        "all-seeds": (ch, seeds(9, range(9)), 3, 0.0, lambda r: r["n_reached"] == 0 and (r["hops"] == 0).all()
                      and r["source"].tolist() == list(range(9))),
        "no-links": (fc.empty(5), seeds(5, [1, 3]), 3, 0.0, lambda r: r["hops"].tolist() == [-1, 0, -1, 0, -1] and r["n_levels"] == 0),
        "n-0": (fc.empty(0), seeds(0, []), 3, 0.0, lambda r: r["n_reached"] == 0 and len(r["hops"]) == 0),
        "star-300": (star(300), seeds(300, [0]), 3, 0.0, lambda r: r["n_reached"] == 299 and r["n_levels"] == 1
                     and (r["parent"][1:] == 0).all()),
        "hub-of-seeds-300": (star(300), seeds(300, range(1, 300)), 3, 0.0,
                             lambda r: r["n_reached"] == 1 and r["parent"][0] == 1 and r["source"][0] == 1 and r["tied_sources"] == 1),
    }
    for n in (63, 64, 65):
        out[f"ring-n-{n}"] = (ring(n), seeds(n, [n // 3]), 64, 0.0, lambda r, n=n: r["n_reached"] == n - 1 and r["n_levels"] == n // 2)
    for m in (255, 256, 257):
        out[f"ring-m-{m}"] = (ring(255, m), seeds(255, [7]), 64, 0.0, lambda r: r["n_reached"] == 128 and r["n_levels"] == 64)
    for n, m, k, ties, late in ((300, 420, 12, 5, 10), (5000, 7000, 150, 50, 300)):
        g, s = random_graph(n, m, k)
        out[f"random-{n}"] = (g, s, 64, 0.0, lambda r, ties=ties: r["tied_sources"] >= ties and 7 <= r["n_levels"] < 64)
        out[f"random-{n}-hops-3"] = (g, s, 3, 0.0, lambda r: r["n_levels"] == 3 and r["hops"].max() == 3)
        out[f"random-{n}-min-0.6"] = (g, s, 64, 0.6, lambda r, late=late, name=f"random-{n}": 7 <= r["n_levels"] < 64 and
                                      int(((r["hops"] > expected(name)["hops"]) & (expected(name)["hops"] >= 0)).sum()) >= late)
        out[f"random-{n}-hops-3-min-0.6"] = (g, s, 3, 0.6, lambda r: r["n_levels"] == 3)
    return out


CASES = _cases()
_results = {}


def expected(name):
    """the restatement's result for a case, computed once and shared (nobody writes into it)"""
    if name not in _results:
        g, seed, max_hops, min_score, holds = CASES[name]
        res = propagate(g["n"], g["u"], g["v"], g["sim"], seed, max_hops, min_score)
        for k in ARRAYS:
            res[k].setflags(write=False)
        _results[name] = res
        if not holds(res):
            del _results[name]
            raise AssertionError((name, {k: v for k, v in res.items() if not isinstance(v, np.ndarray)}))
    return _results[name]


# every input the call refuses: name -> (graph, seed, max_hops, min_score)
def invalid_cases():
    out = {name: (g, seeds(g["n"], [0, 7, 21]), 3, 0.0) for name, (g, _, _) in fc.invalid_cases().items()
           if name.startswith(("u-", "v-", "loop", "sim-"))}
    g = fc.random_graph(40, 60, 11)
    low = seeds(40, [0, 7, 21])
    low[13] = -2
    s = seeds(40, [0, 7, 21])
    out.update({"seed-below-minus-1": (g, low, 3, 0.0), "max-hops-0": (g, s, 0, 0.0), "max-hops-65": (g, s, 65, 0.0),
                "max-hops-negative": (g, s, -1, 0.0), "min-score-nan": (g, s, 3, float("nan")), "min-score-negative": (g, s, 3, -0.01),
                "min-score-above-1": (g, s, 3, 1.5)})
    return out
