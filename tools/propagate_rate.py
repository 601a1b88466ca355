"""The annotation propagation's rate (`fal_network_propagate`), medians of `--reps` calls behind `--warmup` by HIP events, beside the
numpy restatement (tests/propagate_cases.py) on the same links, checked against the device's bits:

1. tests/network_cases.py's analogue families scaled to about `--families_nodes` nodes (tools/network_rate.py's workload), the
   links `fal_network_edges` returns at top_k = 10 left on the device, every tenth node annotated: at max_hops 3 and 64, and at
   max_hops 64 with min_score 0.99.
2. a random graph of `--random_nodes` nodes and 1.4 links a node with sims uniform in [0.7, 1) (tools/family_rate.py's, at cap 0:
   every link survives; one giant component), every tenth node annotated and one node in a thousand: at max_hops 3 and 64.

A call enqueues 2 * max_hops + 3 launches whatever the graph; `levels` is how many of the relax / commit pairs had work.  The
report goes to `--out`.

    python tools/propagate_rate.py [--families_nodes 100000] [--random_nodes 100000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tools.family_rate import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families_nodes", type=int, default=100_000)
    ap.add_argument("--random_nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "network", "propagate_rate.txt"))
    a = ap.parse_args()
    import torch
    from falcon_amd.cluster.cluster import ClusterPipeline
    from tests import network_cases as nc
    from tests import propagate_cases as pc
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x if isinstance(x, str) else json.dumps(x))

    med = lambda v: round(float(np.median(v)), 3)
    c = ClusterPipeline(device=0).ctx
    c.plan(0)
    say(f"propagate_rate: medians of {a.reps} calls after {a.warmup} warm-ups, HIP events; device {torch.cuda.get_device_name(0)}")

    def measure(name, n, u, v, sim, seed, max_hops, min_score, restate=True):
        d_seed = c.to_dev(seed, torch.int32)
        ms, out = timed(lambda: c.network_propagate(u, v, sim, n, d_seed, max_hops, min_score), a.warmup, a.reps)
        source, hops, parent, score, n_reached, n_levels = out
        got = dict(source=source.cpu().numpy(), hops=hops.cpu().numpy(), parent=parent.cpu().numpy(), score=score.cpu().numpy(),
                   n_reached=n_reached, n_levels=n_levels)
        rec = dict(measure=name, nodes=n, links=int(u.numel()), seeds=int((seed >= 0).sum()), max_hops=max_hops, min_score=min_score,
                   reached=n_reached, levels=n_levels, launches=2 * max_hops + 3, call_ms=med(ms),
                   call_ms_all=[round(float(x), 3) for x in ms],
                   nodes_by_hops=np.bincount(got["hops"][got["hops"] >= 0], minlength=1).tolist()[:12])
        if restate:
            hu, hv, hs = u.cpu().numpy(), v.cpu().numpy(), sim.cpu().numpy()
            t0 = time.perf_counter()
            want = pc.propagate(n, hu, hv, hs, seed, max_hops, min_score, stats=False)
            rec.update(numpy_restatement_s=round(time.perf_counter() - t0, 3), equals_restatement=bool(pc.same(got, want)))
            rec["numpy_over_device"] = round(rec["numpy_restatement_s"] / (rec["call_ms"] * 1e-3))
        say(rec)

    # ---- 1. the analogue families ------------------------------------------------------------------------------------------------
    nodes = nc.analogue_case(seed=1, n_templates=max(1, a.families_nodes // 15), wrap=25)
    an = nc.ANALOGUE
    dn = {k: c.to_dev(nodes[k]) for k in ("mz", "intensity", "indptr", "rows", "precursor_mz")}
    n = len(nodes["rows"])
    u, v, sim, _ = c.network_edges(dn["mz"], dn["intensity"], dn["indptr"], dn["rows"], dn["precursor_mz"], an["fragment_tol"],
                                   an["max_shift"], an["min_cosine"], an["min_matched"], 10)
    seed = pc.seeds(n, np.arange(0, n, 10))
    measure("analogue_hops_3", n, u, v, sim, seed, 3, 0.0)
    measure("analogue_hops_64", n, u, v, sim, seed, 64, 0.0)
    measure("analogue_hops_64_min_0.99", n, u, v, sim, seed, 64, 0.99)

    # ---- 2. a random graph with one giant component ---------------------------------------------------------------------------------
    rng = np.random.default_rng(7)
    n, m = a.random_nodes, a.random_nodes * 7 // 5
    ru, rv = rng.integers(0, n, m), rng.integers(0, n, m)
    ok = ru != rv
    ru, rv, rs = ru[ok].astype(np.int32), rv[ok].astype(np.int32), rng.uniform(0.7, 1.0, int(ok.sum())).astype(np.float32)
    du, dv, dsim = c.to_dev(ru), c.to_dev(rv), c.to_dev(rs)
    tenth, sparse = pc.seeds(n, np.arange(0, n, 10)), pc.seeds(n, np.arange(0, n, 1000))
    measure("random_tenth_hops_3", n, du, dv, dsim, tenth, 3, 0.0)
    measure("random_tenth_hops_64", n, du, dv, dsim, tenth, 64, 0.0)
    measure("random_thousandth_hops_64", n, du, dv, dsim, sparse, 64, 0.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
