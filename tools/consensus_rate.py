"""The consensus stage's rate on BASELINE configs[1]'s workload: 1 M synthetic spectra (`synth.generate_device`, seed 42), both
precursor charges, labels and medoids from the default nearest-neighbour path, then `fal_consensus_spectra` alone.

Prints per charge: spectra, clusters (all / of 2+ members), pooled peaks, the share of clusters and of pooled peaks on the
device-wide sort path, fallbacks, output peaks, the clustering pass of the same run (wall, second pass), the consensus stage
(HIP events around the call, median and minimum of `--reps` steady passes after a warm-up; the call synchronises once inside,
so the events span that host gap too) and the numpy restatement (tests/consensus_cases.py) over the same labels on the host,
timed on a uniform sample of `--sample` clusters and SCALED to all clusters.  Then one JSON line with the totals.

    python tools/consensus_rate.py [--n 1000000] [--reps 5] [--sample 20000]
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
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--fragment_tol", type=float, default=0.05)
    ap.add_argument("--min_fraction", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5, help="steady passes of the consensus stage after one warm-up pass")
    ap.add_argument("--sample", type=int, default=20000, help="clusters the numpy restatement is timed on (scaled to all)")
    a = ap.parse_args()
    import torch
    from falcon_amd import _lib, synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    from tests import consensus_cases as cc
    dev = torch.device("cuda", 0)
    data = synth.generate_device(a.n, dev, seed=42)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.plan(0)
    p = AnnParams(eps=a.eps)
    tot = dict(spectra=0, clusters=0, clusters_2plus=0, pooled_peaks=0, global_clusters=0, global_peaks=0, fallbacks=0,
               out_peaks=0, cluster_pass_ms=0.0, consensus_ms=0.0, consensus_min_ms=0.0, numpy_scaled_ms=0.0)
    for charge in (2, 3):
        d = synth.select_charge_device(data, charge)
        ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels, medoids = pipe.run(ds, 20.0, "ppm", None, a.fragment_tol, 2 ** 15, p)
            torch.cuda.synchronize()
            pass_ms = (time.perf_counter() - t0) * 1e3
        n, nc, nnz = len(ds), int(medoids.shape[0]), int(d["mz"].shape[0])
        labels, medoids = labels.to(torch.int32).contiguous(), medoids.to(torch.int32).contiguous()
        out_ptr, status = c.empty((nc + 1,), torch.int64), c.empty((nc,), torch.int32)
        out_mz, out_it = c.empty((nnz,), torch.float32), c.empty((nnz,), torch.float32)

        def stage():
            _lib.check(c.lib.fal_consensus_spectra(c._h, c._p(d["mz"]), c._p(d["intensity"]), c._p(d["indptr"]), n, c._p(labels),
                                                   c._p(medoids), nc, a.fragment_tol, a.min_fraction, nnz, c._p(out_ptr),
                                                   c._p(out_mz), c._p(out_it), c._p(status)), "fal_consensus_spectra")
        stage()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            stage()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        st = status.cpu().numpy()
        lab_h, med_h = labels.cpu().numpy(), medoids.cpu().numpy()
        mz_h, it_h, ip_h = d["mz"].cpu().numpy(), d["intensity"].cpu().numpy(), d["indptr"].cpu().numpy()
        sizes = np.bincount(lab_h, minlength=nc)
        pooled = np.bincount(lab_h, weights=np.diff(ip_h), minlength=nc).astype(np.int64)
        multi = sizes > 1
        glob = (st & _lib.CONS_GLOBAL) != 0
        # the numpy restatement over the same labels, on a uniform sample of clusters, scaled
        rng = np.random.default_rng(0)
        sample = np.sort(rng.choice(nc, size=min(a.sample, nc), replace=False))
        t0 = time.perf_counter()
        ref = cc.consensus_reference(mz_h, it_h, ip_h, lab_h, med_h, a.fragment_tol, a.min_fraction, clusters=sample.tolist())
        np_ms = (time.perf_counter() - t0) * 1e3
        got_ptr, got_mz = out_ptr.cpu().numpy(), out_mz.cpu().numpy()
        same = all(np.array_equal(got_mz[got_ptr[k]:got_ptr[k + 1]].view(np.int32), ref[1][ref[0][k]:ref[0][k + 1]].view(np.int32))
                   for k in sample[:2000])
        row = dict(charge=charge, spectra=n, clusters=nc, clusters_2plus=int(multi.sum()), max_members=int(sizes.max()),
                   pooled_peaks=int(pooled[multi].sum()), global_clusters=int(glob.sum()), global_peaks=int(pooled[glob].sum()),
                   global_cluster_share=round(float(glob.sum()) / max(int(multi.sum()), 1), 6),
                   fallbacks=int(((st & _lib.CONS_FALLBACK) != 0).sum()), out_peaks=int(got_ptr[-1]),
                   cluster_pass_ms=round(pass_ms, 3), consensus_ms=round(float(np.median(times)), 3),
                   consensus_min_ms=round(float(min(times)), 3), numpy_sample=len(sample), numpy_sample_ms=round(np_ms, 1),
                   numpy_scaled_ms=round(np_ms * nc / len(sample), 1), sample_bits_equal=bool(same))
        print(row, flush=True)
        for k in tot:
            tot[k] += row[k]
    for k in ("cluster_pass_ms", "consensus_ms", "consensus_min_ms", "numpy_scaled_ms"):
        tot[k] = round(tot[k], 3)
    tot["numpy_over_gpu"] = round(tot["numpy_scaled_ms"] / tot["consensus_ms"], 1) if tot["consensus_ms"] > 0 else None
    tot["consensus_over_cluster_pass"] = round(tot["consensus_ms"] / tot["cluster_pass_ms"], 3) if tot["cluster_pass_ms"] > 0 else None
    print(json.dumps(dict(tool="consensus_rate", n=a.n, eps=a.eps, min_fraction=a.min_fraction, reps=a.reps, **tot)), flush=True)


if __name__ == "__main__":
    main()
