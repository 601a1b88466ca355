"""Exact mode's per-GPU share of the fixed 10 M job (bench.py --scaling strong's dataset: `synth.generate_device`, both
precursor charges), measured on ONE GPU: every simulated rank runs `ClusterPipeline.run_many(shard=(rank, world))` -- the
same deal on `distributed.exact_window_costs` as a real N-GPU run -- one after the other.  No exchange, no concurrency
between ranks: a PROJECTION of the compute side of the N-GPU run, not a measurement of it.

Prints per rank: rows, buckets, pairs scored (sum of n_b (n_b - 1) / 2), the deal's modelled load and the median wall time
of its passes; then one JSON line with the totals per world size.

    python tools/exact_shard_share.py [--n 10000000] [--worlds 1,8] [--linkage complete] [--eps 0.1] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--worlds", default="1,8")
    ap.add_argument("--linkage", default="complete", choices=["single", "complete", "average"])
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3, help="timed passes per rank (after one warm-up pass); the median is reported")
    a = ap.parse_args()
    import torch
    from falcon_amd import distributed as fdist, synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset, resolve_params
    dev = torch.device("cuda", 0)
    data = synth.generate_device(a.n, dev, seed=42)
    parts = []
    for charge in (2, 3):
        c = synth.select_charge_device(data, charge)
        parts.append(SpectrumDataset(c["precursor_mz"], c["retention_time"], c["mz"], c["intensity"], c["indptr"]))
    del data
    pipe = ClusterPipeline(device=0)
    p = resolve_params(a.linkage, a.eps, 0, AnnParams(eps=a.eps, exact=True))
    args = (20.0, "ppm", None, 0.05, 2 ** 15, p)
    counts = pipe.ctx.window_counts([ds.precursor_mz for ds in parts], p.mz_interval)
    costs = fdist.exact_window_costs(counts, args[4])

    def one_pass(rank, world):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = pipe.run_many(parts, *args, shard=(rank, world) if world > 1 else None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, outs

    out = {"tool": "exact_shard_share", "n": a.n, "linkage": a.linkage, "eps": a.eps, "worlds": {}}
    for world in [int(x) for x in a.worlds.split(",")]:
        owners = fdist.deal_job(list(costs), world)
        ranks = []
        for rank in range(world):
            pipe.trim()                                    # every simulated rank starts from the pools of a fresh process
            one_pass(rank, world)
            ts = []
            for _ in range(a.reps):
                ms, outs = one_pass(rank, world)
                ts.append(ms)
            sizes = np.concatenate([np.diff(np.asarray(l["splits"], np.int64)) for l in pipe.lasts if "splits" in l] or
                                   [np.zeros(0, np.int64)])
            row = dict(rank=rank, rows=int(sum(int(o[0].numel()) for o in outs)), buckets=int(len(sizes)),
                       max_bucket=int(sizes.max()) if len(sizes) else 0, pairs=int((sizes * (sizes - 1) // 2).sum()),
                       modelled_load=float(sum(c[o == rank].sum() for c, o in zip(costs, owners))),
                       ms=round(sorted(ts)[len(ts) // 2], 2), passes_ms=[round(t, 2) for t in ts])
            print(f"world {world} {row}", flush=True)
            ranks.append(row)
        ms = np.array([r["ms"] for r in ranks])
        load = np.array([r["modelled_load"] for r in ranks])
        out["worlds"][world] = dict(ranks=ranks, slowest_rank_ms=float(ms.max()), mean_rank_ms=round(float(ms.mean()), 2),
                                    worst_over_mean_ms=round(float(ms.max() / ms.mean()), 3),
                                    worst_over_mean_modelled=round(float(load.max() / load.mean()), 3),
                                    pairs=int(sum(r["pairs"] for r in ranks)))
    w = sorted(out["worlds"])
    if len(w) > 1:
        out["projected_speedup"] = round(out["worlds"][w[0]]["slowest_rank_ms"] / out["worlds"][w[-1]]["slowest_rank_ms"], 2)
    out["note"] = ("one GPU running every rank's share in turn: the compute side of the sharded exact job (window histograms, the "
                   "deal, the rank's sort, edges, linkage, medoids); the labels-only all-gatherv is not included. A projection: "
                   "no multi-GPU node was used")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
