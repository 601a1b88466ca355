"""The member-score stage's rate (`fal_member_scores` + `fal_cluster_summary`) on 1 M synthetic spectra (`synth.generate_device`,
seed 42), both precursor charges, labels and medoids from the unchanged default nearest-neighbour path, medoid representatives.

Per charge, by HIP events, the median of `--reps` passes behind `--warmup`: the score kernel alone (the library's stage timer),
the two calls together (sort, kernels, the one wait, the summary), and the clustering pass of the same run (events around
`ClusterPipeline.run`).  With them the cluster-size histogram, the pairs the solver finished, and how many of the score kernel's
64-member tiles hold only clusters of one member.

In the same session: the scoring kernel of `fal_assign_nearest` as `tools/assign_rate.py` times it (library = the medoids,
queries = a second draw, seed 43) -- the same per-pair code at 64 x 64 tiles, the yardstick for pairs per second -- and the
numpy restatement (tests/memberscore_cases.py) on `--sample` clusters per charge, checked against the device's bits and scaled
to all clusters.  The report goes to `--out`.

    python tools/memberscore_rate.py [--n 1000000] [--reps 5] [--warmup 2] [--sample 2000] [--out profiles/memberscore/...]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def timed(fn, warmup, reps, after=None):
    """-> (HIP-event ms of every steady pass, what `after()` returned behind each, the last result)"""
    import torch
    ms, extra, out = [], [], None
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
            if after is not None:
                extra.append(after())
    return ms, extra, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--fragment_tol", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=2000, help="clusters per charge the numpy restatement is timed on (scaled to all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from falcon_amd import synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    from tests import memberscore_cases as mc
    out_path = a.out or os.path.join("profiles", "memberscore", f"memberscore_rate_{a.n // 1_000_000}M.txt" if a.n % 1_000_000 == 0
                                     else f"memberscore_rate_{a.n}.txt")
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x if isinstance(x, str) else json.dumps(x))

    med = lambda v: round(float(np.median(v)), 3)
    dev = torch.device("cuda", 0)
    first = synth.generate_device(a.n, dev, seed=42)
    second = synth.generate_device(a.n, dev, seed=43)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.plan(0)
    c.enable_timing(True)
    p = AnnParams(eps=a.eps)
    say(f"memberscore_rate: n = {a.n}, eps = {a.eps}, 20 ppm, fragment_tol = {a.fragment_tol}, medoid representatives, median of "
        f"{a.reps} passes after {a.warmup} warm-ups, HIP events; device {torch.cuda.get_device_name(0)}")
    keys = ("spectra", "clusters", "solver_pairs", "score_kernel_ms", "stage_ms", "cluster_pass_ms", "numpy_s_scaled",
            "assign_pairs", "assign_kernel_ms")
    tot = {k: 0 for k in keys}
    hist_edges = [1, 2, 3, 5, 9, 17, 33, 65, 129, 1 << 30]
    hist_names = ["1", "2", "3-4", "5-8", "9-16", "17-32", "33-64", "65-128", "129+"]
    hist_tot = np.zeros(len(hist_names), np.int64)
    for charge in (2, 3):
        d = synth.select_charge_device(first, charge)
        ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
        pass_ms, _, (labels, medoids) = timed(lambda: pipe.run(ds, 20.0, "ppm", None, a.fragment_tol, 2 ** 15, p), a.warmup, a.reps)
        labels, medoids = labels.to(torch.int32).contiguous(), medoids.to(torch.int32).contiguous()
        n, nc = int(labels.numel()), int(medoids.numel())

        def stage():
            sim, matched = c.member_scores(d["mz"], d["intensity"], d["indptr"], labels, d["mz"], d["intensity"], d["indptr"], medoids,
                                           a.fragment_tol)
            return sim, matched, c.cluster_summary(labels, nc, sim, d["precursor_mz"], d["retention_time"])
        _, kern, _ = timed(lambda: c.member_scores(d["mz"], d["intensity"], d["indptr"], labels, d["mz"], d["intensity"], d["indptr"],
                                                   medoids, a.fragment_tol), a.warmup, a.reps, after=lambda: c.stage_ms("kernel")[0])
        solver = c.counter(9)
        stage_ms, _, (sim, matched, cols) = timed(stage, a.warmup, a.reps)
        # the yardstick: fal_assign_nearest's scoring kernel, library = the medoids, queries = a second draw
        lib = pipe._take_rows(c, ds, medoids.long())
        l_pmz = d["precursor_mz"][medoids.long()].contiguous()
        q = synth.select_charge_device(second, charge)
        _, a_kern, (_, _, cand) = timed(lambda: c.assign_nearest(q["mz"], q["intensity"], q["indptr"], q["precursor_mz"], None, lib.mz,
                                                                 lib.intensity, lib.indptr, l_pmz, None, 20.0, "ppm", None,
                                                                 a.fragment_tol, 0),
                                        a.warmup, a.reps, after=lambda: c.stage_ms("kernel")[0])
        a_pairs = int(cand.sum(dtype=torch.int64).item())
        # shape of the work
        host = lambda t: t.cpu().numpy()
        lab_h, med_h = host(labels), host(medoids)
        sizes = np.bincount(lab_h, minlength=nc)
        hist = np.histogram(sizes, bins=hist_edges)[0]
        hist_tot += hist
        order = np.argsort(lab_h, kind="stable")
        pad = (-n) % 64
        tile_sizes = np.concatenate([sizes[lab_h[order]], np.ones(pad, np.int64)]).reshape(-1, 64)
        singleton_tiles = int((tile_sizes.max(axis=1) == 1).sum())
        # the numpy restatement on a sample of clusters, against the device's bits, scaled to all clusters
        case = dict(mz=host(d["mz"]), intensity=host(d["intensity"]), indptr=host(d["indptr"]), labels=lab_h, medoids=med_h)
        sample = np.sort(np.random.default_rng(charge).choice(nc, min(a.sample, nc), replace=False))
        rows = np.flatnonzero(np.isin(lab_h, sample))
        pmz_h, rt_h = host(d["precursor_mz"]), host(d["retention_time"])
        mc.scores_ref(case, *mc.medoid_form(case), a.fragment_tol, rows=rows[:1])      # (scipy's import is not the restatement's time)
        t0 = time.perf_counter()
        r_sim, r_matched = mc.scores_ref(case, *mc.medoid_form(case), a.fragment_tol, rows=rows)
        r_cols = mc.summary_ref(lab_h, nc, r_sim, pmz_h, rt_h, clusters=sample)
        t_np = time.perf_counter() - t0
        same = mc.same(r_sim[rows], host(sim)[rows]) and mc.same(r_matched[rows], host(matched)[rows]) and \
            all(mc.same(r_cols[k][sample], host(cols[k])[sample]) for k in mc.COLUMNS)
        k_ms, s_ms = med(kern), med(stage_ms)
        rec = dict(charge=charge, spectra=n, clusters=nc, max_members=int(sizes.max()), size_histogram=dict(zip(hist_names, hist.tolist())),
                   tiles=int(tile_sizes.shape[0]), singleton_only_tiles=singleton_tiles, solver_pairs=solver,
                   score_kernel_ms=k_ms, score_kernel_ms_all=[round(x, 3) for x in kern], stage_ms=s_ms,
                   stage_ms_all=[round(x, 3) for x in stage_ms], cluster_pass_ms=med(pass_ms),
                   cluster_pass_ms_all=[round(x, 3) for x in pass_ms], pairs_per_s_kernel=round(n / (k_ms * 1e-3)) if k_ms > 0 else None,
                   pairs_per_s_stage=round(n / (s_ms * 1e-3)), assign_pairs=a_pairs, assign_kernel_ms=med(a_kern),
                   assign_pairs_per_s_kernel=round(a_pairs / (med(a_kern) * 1e-3)) if med(a_kern) > 0 else None,
                   mean_similarity=round(float(host(sim).astype(np.float64).mean()), 6), numpy_sample_clusters=len(sample),
                   numpy_sample_members=len(rows), numpy_sample_s=round(t_np, 3), numpy_s_scaled=round(t_np * nc / len(sample), 1),
                   sample_equals_device=bool(same))
        say(rec)
        for k in keys:
            tot[k] += rec[k]
    for k in ("score_kernel_ms", "stage_ms", "cluster_pass_ms", "assign_kernel_ms", "numpy_s_scaled"):
        tot[k] = round(tot[k], 3)
    tot["size_histogram"] = dict(zip(hist_names, hist_tot.tolist()))
    tot["pairs_per_s_kernel"] = round(tot["spectra"] / (tot["score_kernel_ms"] * 1e-3)) if tot["score_kernel_ms"] > 0 else None
    tot["assign_pairs_per_s_kernel"] = round(tot["assign_pairs"] / (tot["assign_kernel_ms"] * 1e-3)) if tot["assign_kernel_ms"] > 0 else None
    tot["stage_over_cluster_pass"] = round(tot["stage_ms"] / tot["cluster_pass_ms"], 4) if tot["cluster_pass_ms"] > 0 else None
    tot["numpy_over_device"] = round(tot["numpy_s_scaled"] / (tot["stage_ms"] * 1e-3)) if tot["stage_ms"] > 0 else None
    say(dict(tool="memberscore_rate", n=a.n, **tot))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
