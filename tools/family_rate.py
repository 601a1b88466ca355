"""The molecular families' rate (`fal_network_families`), medians of `--reps` calls behind `--warmup` by HIP events, in one session
with its yardsticks:

1. tests/network_cases.py's analogue families scaled to about `--families_nodes` nodes (tools/network_rate.py's workload), the
   result of `fal_network_edges` at top_k = 10 as input, left on the device: the call at cap 100 / delta 0.02 and at cap 0; the
   `fal_network_edges` call that produced the edges; the numpy restatement (tests/family_cases.py) on the same edges, checked
   against the device's bits, and scipy's `connected_components` for the uncapped case where scipy is installed.
2. a random graph of `--random_nodes` nodes and 1.4 edges a node with sims uniform in [0.7, 1) (one giant component: many rounds)
   at cap 100 / delta 0.02, with the restatement.

A call's time less its kernels' is what the per-pass synchronisations cost: the report gives the call per pass.  The report goes to
`--out`.

    python tools/family_rate.py [--families_nodes 100000] [--random_nodes 100000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def timed(fn, warmup, reps):
    """-> HIP-event ms of every steady call, the last result"""
    import torch
    ms, out = [], None
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    return np.array(ms), out


def size_histogram(size, family):
    """families by their node count: {"2": .., "3-5": .., ...} and the nodes without a family"""
    sizes = np.bincount(family[family >= 0]) if (family >= 0).any() else np.zeros(0, np.int64)
    edges = [2, 3, 6, 11, 21, 51, 101, 1001, 1 << 62]
    names = ["2", "3-5", "6-10", "11-20", "21-50", "51-100", "101-1000", "above 1000"]
    hist = {nm: int(((sizes >= lo) & (sizes < hi)).sum()) for nm, lo, hi in zip(names, edges[:-1], edges[1:])}
    return dict(families_by_size=hist, largest=int(sizes.max()) if len(sizes) else 0, nodes_without_family=int((family < 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families_nodes", type=int, default=100_000)
    ap.add_argument("--random_nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "network", "family_rate.txt"))
    a = ap.parse_args()
    import torch
    from falcon_amd.cluster.cluster import ClusterPipeline
    from tests import family_cases as fc
    from tests import network_cases as nc
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x if isinstance(x, str) else json.dumps(x))

    med = lambda v: round(float(np.median(v)), 3)
    c = ClusterPipeline(device=0).ctx
    c.plan(0)
    say(f"family_rate: medians of {a.reps} calls after {a.warmup} warm-ups, HIP events; device {torch.cuda.get_device_name(0)}")

    def measure(name, n, u, v, sim, max_size, delta, restate=True, **extra):
        ms, out = timed(lambda: c.network_families(u, v, sim, n, max_size, delta), a.warmup, a.reps)
        family, size, rnd, n_families, n_rounds = out
        got = dict(family=family.cpu().numpy(), size=size.cpu().numpy(), round=rnd.cpu().numpy(), n_families=n_families, n_rounds=n_rounds)
        rec = dict(measure=name, nodes=n, edges=int(u.numel()), max_size=max_size, delta=delta, rounds=n_rounds, passes=n_rounds + 1,
                   families=n_families, edges_cut=c.counter(13), call_ms=med(ms), call_ms_all=[round(float(x), 3) for x in ms],
                   call_ms_per_pass=round(med(ms) / (n_rounds + 1), 4), **size_histogram(got["size"], got["family"]), **extra)
        if restate:
            hu, hv, hs = u.cpu().numpy(), v.cpu().numpy(), sim.cpu().numpy()
            t0 = time.perf_counter()
            want = fc.families(n, hu, hv, hs, max_size, delta)
            rec.update(numpy_restatement_s=round(time.perf_counter() - t0, 3), equals_restatement=bool(fc.same(got, want)))
            rec["numpy_over_device"] = round(rec["numpy_restatement_s"] / (rec["call_ms"] * 1e-3))
        say(rec)
        return got

    # ---- 1. the analogue families ------------------------------------------------------------------------------------------------
    nodes = nc.analogue_case(seed=1, n_templates=max(1, a.families_nodes // 15), wrap=25)
    an = nc.ANALOGUE
    dn = {k: c.to_dev(nodes[k]) for k in ("mz", "intensity", "indptr", "rows", "precursor_mz")}
    n = len(nodes["rows"])
    ms, (u, v, sim, _) = timed(lambda: c.network_edges(dn["mz"], dn["intensity"], dn["indptr"], dn["rows"], dn["precursor_mz"],
                                                       an["fragment_tol"], an["max_shift"], an["min_cosine"], an["min_matched"], 10),
                               a.warmup, a.reps)
    hs = sim.cpu().numpy()
    say(dict(measure="network_edges", nodes=n, edges=int(u.numel()), top_k=10, call_ms=med(ms),
             sim_percentiles_0_10_50_90_100=[round(float(x), 4) for x in np.percentile(hs, [0, 10, 50, 90, 100])]))
    measure("analogue_families", n, u, v, sim, 100, 0.02)
    got = measure("analogue_families_uncapped", n, u, v, sim, 0, 0.02)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        hu, hv = u.cpu().numpy(), v.cpu().numpy()
        t0 = time.perf_counter()
        k, lab = connected_components(coo_matrix((np.ones(len(hu), np.int8), (hu, hv)), shape=(n, n)), directed=False)
        t_sp = time.perf_counter() - t0
        same = len(set(zip(lab.tolist(), got["family"].tolist()))) == k and int((np.bincount(lab) >= 2).sum()) == got["n_families"]
        say(dict(measure="scipy_connected_components", seconds=round(t_sp, 4), components=int(k), same_partition=bool(same)))
    except ImportError:
        say(dict(measure="scipy_connected_components", seconds=None, note="scipy is not installed"))

    # ---- 2. a random graph with one giant component ---------------------------------------------------------------------------------
    rng = np.random.default_rng(7)
    n, m = a.random_nodes, a.random_nodes * 7 // 5
    ru, rv = rng.integers(0, n, m), rng.integers(0, n, m)
    ok = ru != rv
    ru, rv, rs = ru[ok].astype(np.int32), rv[ok].astype(np.int32), rng.uniform(0.7, 1.0, int(ok.sum())).astype(np.float32)
    measure("random_graph", n, c.to_dev(ru), c.to_dev(rv), c.to_dev(rs), 100, 0.02)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
