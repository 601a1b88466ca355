"""The representative search's rate (`fal_assign_nearest`): library = the medoid representatives of a clustering of 1 M
synthetic spectra (`synth.generate_device`, seed 42, the default nearest-neighbour path), queries = a second 1 M draw of the
same generator (seed 43), both precursor charges.

Per charge: library rows, queries, window pairs scored (the candidates: sum of n_cand), pairs the solver finished, the scoring
kernel's time (the library's stage timer) and the whole call's (HIP events around it: sorts, kernels, the one wait) -- the median
of `--reps` passes behind `--warmup` -- and pairs/s of both.  Then the numpy restatement (the rule spelled out with
`oracle.falcon_oracle`: vectorised candidate test, `cosine_fast` per candidate) on `--sample` queries, checked against the
device's results, its time scaled to all queries, and the ratio.  The report goes to `--out`.

    python tools/assign_rate.py [--n 1000000] [--reps 5] [--warmup 2] [--sample 2000] [--out profiles/assign/assign_rate_1M.txt]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def restate(q, l, rows, tol, mode, fragment_tol, min_matches):
    """the rule for the queries `rows` (host arrays) -> best_row, best_dist, n_cand"""
    from oracle import falcon_oracle as fo
    f32 = np.float32
    best_row, best_dist, n_cand = np.full(len(rows), -1, np.int32), np.ones(len(rows), f32), np.zeros(len(rows), np.int32)
    pk = lambda d, r: (d["mz"][d["indptr"][r]:d["indptr"][r + 1]], d["intensity"][d["indptr"][r]:d["indptr"][r + 1]])
    for k, i in enumerate(rows):
        md = np.abs(fo.mass_diff(np.full(len(l["precursor_mz"]), q["precursor_mz"][i], f32), l["precursor_mz"], mode == "Da"))
        cand = np.flatnonzero(md <= tol)
        n_cand[k] = len(cand)
        if not len(cand):
            continue
        dist = np.empty(len(cand), f32)
        for x, j in enumerate(cand):
            sim, nm = fo.cosine_fast(*pk(q, i), *pk(l, j), fragment_tol)
            dist[x] = f32(1.0 - (0.0 if nm < min_matches else sim))
        w = np.lexsort((cand, l["precursor_mz"][cand], dist))[0]
        best_row[k], best_dist[k] = cand[w], dist[w]
    return best_row, best_dist, n_cand


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--fragment_tol", type=float, default=0.05)
    ap.add_argument("--min_matches", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from falcon_amd import synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    out_path = a.out or os.path.join("profiles", "assign", f"assign_rate_{a.n // 1_000_000}M.txt" if a.n % 1_000_000 == 0
                                     else f"assign_rate_{a.n}.txt")
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x if isinstance(x, str) else json.dumps(x))

    dev = torch.device("cuda", 0)
    first = synth.generate_device(a.n, dev, seed=42)
    second = synth.generate_device(a.n, dev, seed=43)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.enable_timing(True)
    p = AnnParams(eps=a.eps)
    say(f"assign_rate: n = {a.n} per draw, eps = {a.eps}, 20 ppm, fragment_tol = {a.fragment_tol}, min_matches = {a.min_matches}, "
        f"median of {a.reps} passes after {a.warmup} warm-ups; device {torch.cuda.get_device_name(0)}")
    tot = dict(queries=0, library=0, pairs=0, solver_pairs=0, kernel_ms=0.0, call_ms=0.0, numpy_s_scaled=0.0)
    for charge in (2, 3):
        d = synth.select_charge_device(first, charge)
        ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
        labels, medoids = pipe.run(ds, 20.0, "ppm", None, a.fragment_tol, 2 ** 15, p)
        lib = pipe._take_rows(c, ds, medoids.long())
        l_pmz = d["precursor_mz"][medoids.long()].contiguous()
        q = synth.select_charge_device(second, charge)
        args = (q["mz"], q["intensity"], q["indptr"], q["precursor_mz"], None, lib.mz, lib.intensity, lib.indptr, l_pmz, None,
                20.0, "ppm", None, a.fragment_tol, a.min_matches)
        kern, call = [], []
        for rep in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            row, dist, cand = c.assign_nearest(*args)
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                kern.append(c.stage_ms("kernel")[0])
                call.append(e0.elapsed_time(e1))
        pairs, solver = int(cand.sum(dtype=torch.int64).item()), c.counter(9)
        k_ms, c_ms = float(np.median(kern)), float(np.median(call))
        # the restatement on a sample, against the device's results
        host = lambda t: t.cpu().numpy()
        qh = dict(mz=host(q["mz"]), intensity=host(q["intensity"]), indptr=host(q["indptr"]), precursor_mz=host(q["precursor_mz"]))
        lh = dict(mz=host(lib.mz), intensity=host(lib.intensity), indptr=host(lib.indptr), precursor_mz=host(l_pmz))
        nq = len(qh["precursor_mz"])
        rows = np.sort(np.random.default_rng(charge).choice(nq, min(a.sample, nq), replace=False))
        t0 = time.perf_counter()
        r_row, r_dist, r_cand = restate(qh, lh, rows, 20.0, "ppm", a.fragment_tol, a.min_matches)
        t_np = time.perf_counter() - t0
        same = (np.array_equal(r_row, host(row)[rows]) and np.array_equal(r_dist.view(np.int32), host(dist)[rows].view(np.int32))
                and np.array_equal(r_cand, host(cand)[rows]))
        rec = dict(charge=charge, library=int(medoids.numel()), queries=nq, pairs=pairs, solver_pairs=solver,
                   kernel_ms=round(k_ms, 3), kernel_ms_all=[round(x, 3) for x in kern], call_ms=round(c_ms, 3),
                   call_ms_all=[round(x, 3) for x in call], pairs_per_s_kernel=round(pairs / (k_ms * 1e-3)) if k_ms > 0 else None,
                   pairs_per_s_call=round(pairs / (c_ms * 1e-3)), assigned=int(((row >= 0) & (dist <= a.eps)).sum().item()),
                   numpy_sample=len(rows), numpy_sample_s=round(t_np, 3), numpy_s_scaled=round(t_np * nq / len(rows), 1),
                   sample_equals_device=bool(same))
        say(rec)
        for k in ("queries", "library", "pairs", "solver_pairs", "kernel_ms", "call_ms", "numpy_s_scaled"):
            tot[k] += rec[k]
    tot["pairs_per_s_kernel"] = round(tot["pairs"] / (tot["kernel_ms"] * 1e-3)) if tot["kernel_ms"] > 0 else None
    tot["pairs_per_s_call"] = round(tot["pairs"] / (tot["call_ms"] * 1e-3)) if tot["call_ms"] > 0 else None
    tot["numpy_over_device"] = round(tot["numpy_s_scaled"] / (tot["call_ms"] * 1e-3)) if tot["call_ms"] > 0 else None
    say(dict(tool="assign_rate", n=a.n, **tot))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
