"""The representative network's rate (`fal_network_edges`), three measurements in one session, medians of `--reps` passes behind
`--warmup` by HIP events and the library's stage timers (stage "kernel" = the tile kernel, "tail" = the greedy kernel):

1. search cost: the medoids of 1 M synthetic spectra (`synth.generate_device`, seed 42; default nearest-neighbour clustering),
   per precursor charge, at the default thresholds.  Those spectra share no analogues: this is the tile kernel and its prefilter.
   `--max_shift` is halved until the pairs in scope are at most `--max_pairs`; the value used is reported.
2. greedy and filter cost: tests/network_cases.py's analogue families scaled to about `--families_nodes` nodes (template t at the
   precursor of template t mod 25), with top_k = 0 and top_k = 10.
3. yardsticks: exact mode's edge kernel on the same 1 M spectra as tools/exact_rate.py times it (pairs per second), and the numpy
   restatement on `--sample` consecutive nodes (in precursor order) of the families, checked against the device's bits and scaled
   by the pairs in scope.

Pairs in scope are counted with a float64 search over the sorted float32 precursors (the float32 rule differs at one-ulp
boundaries only).  The report goes to `--out`.

    python tools/network_rate.py [--n 1000000] [--max_shift 200] [--max_pairs 4e9] [--families_nodes 100000] [--sample 300]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def pairs_in_scope(pmz, max_shift):
    s = np.sort(np.asarray(pmz, np.float64))
    return int((np.searchsorted(s, s + max_shift, side="right") - np.arange(len(s)) - 1).sum())


def timed(c, fn, warmup, reps):
    """-> (HIP-event ms, tile-kernel ms, greedy-kernel ms) of every steady pass, the last result"""
    import torch
    ms, out = [], None
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warmup:
            ms.append((e0.elapsed_time(e1), c.stage_ms("kernel")[0], c.stage_ms("tail")[0]))
    return np.array(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--fragment_tol", type=float, default=0.05)
    ap.add_argument("--max_shift", type=float, default=200.0)
    ap.add_argument("--max_pairs", type=float, default=4e9)
    ap.add_argument("--families_nodes", type=int, default=100_000)
    ap.add_argument("--sample", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip_exact", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "network", "network_rate.txt"))
    a = ap.parse_args()
    import torch
    from falcon_amd import synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    from tests import network_cases as nc
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x if isinstance(x, str) else json.dumps(x))

    med = lambda v: round(float(np.median(v)), 3)
    dev = torch.device("cuda", 0)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.plan(0)
    c.enable_timing(True)
    say(f"network_rate: medians of {a.reps} passes after {a.warmup} warm-ups, HIP events and stage timers; fragment_tol = "
        f"{a.fragment_tol}; device {torch.cuda.get_device_name(0)}")

    # ---- 1. search cost ------------------------------------------------------------------------------------------------------
    data = synth.generate_device(a.n, dev, seed=42)
    tot = dict(nodes=0, pairs_in_scope=0, greedy_pairs=0, edges=0, call_ms=0.0, tile_kernel_ms=0.0, greedy_kernel_ms=0.0)
    for charge in (2, 3):
        d = synth.select_charge_device(data, charge)
        ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
        labels, medoids = pipe.run(ds, 20.0, "ppm", None, a.fragment_tol, 2 ** 15, AnnParams(eps=0.1))
        medoids = medoids.to(torch.int32).contiguous()
        pmz = d["precursor_mz"][medoids.long()].contiguous()
        pmz_h = pmz.cpu().numpy()
        shift = a.max_shift
        while pairs_in_scope(pmz_h, shift) > a.max_pairs:
            shift /= 2
        pairs = pairs_in_scope(pmz_h, shift)
        ms, out = timed(c, lambda: c.network_edges(d["mz"], d["intensity"], d["indptr"], medoids, pmz, a.fragment_tol, shift, 0.7, 6, 10),
                        a.warmup, a.reps)
        call, tile, greedy = med(ms[:, 0]), med(ms[:, 1]), med(ms[:, 2])
        rec = dict(measure="search", charge=charge, nodes=int(medoids.numel()), max_shift_used=shift, pairs_in_scope=pairs,
                   greedy_pairs=c.counter(12), pairs_passed_on_share=round(c.counter(12) / max(pairs, 1), 9), edges=int(out[0].numel()),
                   call_ms=call, tile_kernel_ms=tile, greedy_kernel_ms=greedy, call_ms_all=[round(float(x), 3) for x in ms[:, 0]],
                   pairs_per_s_tile_kernel=round(pairs / (tile * 1e-3)) if tile > 0 else None, pairs_per_s_call=round(pairs / (call * 1e-3)))
        say(rec)
        for k in tot:
            tot[k] += rec[k]
    tot["pairs_per_s_tile_kernel"] = round(tot["pairs_in_scope"] / (tot["tile_kernel_ms"] * 1e-3)) if tot["tile_kernel_ms"] > 0 else None
    say(dict(measure="search_total", n=a.n, **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in tot.items()}))
    search_rate = tot["pairs_per_s_tile_kernel"]

    # ---- 3a. yardstick: exact mode's edge kernel -----------------------------------------------------------------------------------
    exact_rate = None
    if not a.skip_exact:
        p = AnnParams(eps=0.1, exact=True, clustering="hierarchical", linkage="complete", min_matches=0)
        ex_pairs, ex_ms = 0, 0.0
        for charge in (2, 3):
            d = synth.select_charge_device(data, charge)
            ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
            for _ in range(2):
                pipe.run(ds, 20.0, "ppm", None, a.fragment_tol, 2 ** 15, p)
                torch.cuda.synchronize()
            nb = np.diff(pipe.last["splits"]).astype(np.int64)
            ex_pairs += int((nb * (nb - 1) // 2).sum())
            ex_ms += c.stage_ms("kernel")[0]
        exact_rate = round(ex_pairs / (ex_ms * 1e-3)) if ex_ms > 0 else None
        say(dict(measure="exact_edges_kernel", pairs=ex_pairs, kernel_ms=round(ex_ms, 3), pairs_per_s_kernel=exact_rate,
                 network_tile_over_exact=round(search_rate / exact_rate, 4) if exact_rate and search_rate else None))
    del data

    # ---- 2. greedy and filter cost ---------------------------------------------------------------------------------------------
    t0 = time.perf_counter()
    nodes = nc.analogue_case(seed=1, n_templates=max(1, a.families_nodes // 15), wrap=25)
    t_gen = time.perf_counter() - t0
    an = nc.ANALOGUE
    dn = {k: c.to_dev(nodes[k]) for k in ("mz", "intensity", "indptr", "rows", "precursor_mz")}
    pairs = pairs_in_scope(nodes["precursor_mz"], an["max_shift"])
    fam = {}
    for top_k in (0, 10):
        ms, out = timed(c, lambda: c.network_edges(dn["mz"], dn["intensity"], dn["indptr"], dn["rows"], dn["precursor_mz"],
                                                   an["fragment_tol"], an["max_shift"], an["min_cosine"], an["min_matched"], top_k),
                        a.warmup, a.reps)
        fam[top_k] = dict(measure="families", top_k=top_k, nodes=len(nodes["rows"]), generate_s=round(t_gen, 1), pairs_in_scope=pairs,
                          greedy_pairs=c.counter(12), edges=int(out[0].numel()), call_ms=med(ms[:, 0]), tile_kernel_ms=med(ms[:, 1]),
                          greedy_kernel_ms=med(ms[:, 2]), call_ms_all=[round(float(x), 3) for x in ms[:, 0]],
                          greedy_pairs_per_s_kernel=round(c.counter(12) / (med(ms[:, 2]) * 1e-3)) if med(ms[:, 2]) > 0 else None,
                          pairs_per_s_tile_kernel=round(pairs / (med(ms[:, 1]) * 1e-3)) if med(ms[:, 1]) > 0 else None)
        say(fam[top_k])
    say(dict(measure="families_filter", top_k_filter_ms=round(fam[10]["call_ms"] - fam[0]["call_ms"], 3),
             edges_before=fam[0]["edges"], edges_after=fam[10]["edges"]))

    # ---- 3b. yardstick: the numpy restatement on consecutive nodes of the families ---------------------------------------------------
    order = np.argsort(nodes["precursor_mz"], kind="stable")
    take = np.sort(order[len(order) // 2:len(order) // 2 + a.sample])
    sub = nc.permute_nodes(nodes, take)
    t0 = time.perf_counter()
    want = nc.network_ref(sub, an["fragment_tol"], an["max_shift"], an["min_cosine"], an["min_matched"], 10)
    t_np = time.perf_counter() - t0
    got = tuple(t.cpu().numpy() for t in c.network_edges(sub["mz"], sub["intensity"], sub["indptr"], sub["rows"], sub["precursor_mz"],
                                                         an["fragment_tol"], an["max_shift"], an["min_cosine"], an["min_matched"], 10))
    sub_pairs = pairs_in_scope(sub["precursor_mz"], an["max_shift"])
    scaled = t_np * pairs / max(sub_pairs, 1)
    say(dict(measure="numpy_restatement", sample_nodes=len(take), sample_pairs_in_scope=sub_pairs, sample_s=round(t_np, 3),
             sample_equals_device=bool(nc.same_edges(got, want)), scaled_to_families_s=round(scaled, 1),
             numpy_over_device=round(scaled / (fam[10]["call_ms"] * 1e-3)) if fam[10]["call_ms"] > 0 else None))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
