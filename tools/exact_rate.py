"""Exact mode's rate on BASELINE configs[1]'s workload: 1 M synthetic spectra (`synth.generate_device`, seed 42), both
precursor charges, every pair of every bucket scored with the matched-peak cosine (`fal_cluster_exact`).

Prints per charge: spectra, buckets, pairs scored (sum of n_b (n_b - 1) / 2), the stage times of the pass (edge kernel,
edges + fallback, linkage / refinement / medoids) and pairs/s of the edge kernel, then one JSON line with the totals.

    python tools/exact_rate.py [--n 1000000] [--linkage complete] [--eps 0.1] [--reps 2]
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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--linkage", default="complete", choices=["single", "complete", "average"])
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--fragment_tol", type=float, default=0.05)
    ap.add_argument("--min_matches", type=int, default=0)
    ap.add_argument("--reps", type=int, default=2, help="passes per charge; the last one is reported (the first loads code objects)")
    a = ap.parse_args()
    import torch
    from falcon_amd import synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    dev = torch.device("cuda", 0)
    data = synth.generate_device(a.n, dev, seed=42)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.enable_timing(True)
    p = AnnParams(eps=a.eps, exact=True, clustering="hierarchical", linkage=a.linkage, min_matches=a.min_matches)
    tot = dict(spectra=0, pairs=0, edge_kernel_ms=0.0, edges_ms=0.0, tail_ms=0.0, wall_ms=0.0, clusters=0)
    for charge in (2, 3):
        d = synth.select_charge_device(data, charge)
        ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels, medoids = pipe.run(ds, 20.0, "ppm", None, a.fragment_tol, 2 ** 15, p)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        nb = np.diff(pipe.last["splits"]).astype(np.int64)
        pairs = int((nb * (nb - 1) // 2).sum())
        kern, edges, tail = c.stage_ms("kernel")[0], c.stage_ms("scan")[0], c.stage_ms("tail")[0]
        n_cl = int((torch.bincount(labels.long()) > 1).sum().item())
        row = dict(charge=charge, spectra=len(ds), buckets=len(nb), max_bucket=int(nb.max()), pairs=pairs,
                   edge_kernel_ms=round(kern, 3), edges_ms=round(edges, 3), tail_ms=round(tail, 3), wall_ms=round(wall, 3),
                   pairs_per_s_kernel=round(pairs / (kern * 1e-3)) if kern > 0 else None, clusters=n_cl)
        print(row, flush=True)
        for k in ("spectra", "pairs", "clusters"):
            tot[k] += row[k]
        for k in ("edge_kernel_ms", "edges_ms", "tail_ms", "wall_ms"):
            tot[k] += row[k]
    tot["pairs_per_s_kernel"] = round(tot["pairs"] / (tot["edge_kernel_ms"] * 1e-3)) if tot["edge_kernel_ms"] > 0 else None
    tot["pairs_per_s_wall"] = round(tot["pairs"] / (tot["wall_ms"] * 1e-3))
    print(json.dumps(dict(tool="exact_rate", n=a.n, linkage=a.linkage, eps=a.eps, **tot)), flush=True)


if __name__ == "__main__":
    main()
