"""The library search's rate (`fal_library_search`), three measurements in one session, medians of `--reps` passes behind
`--warmup` by HIP events and the library's stage timers (stage "kernel" = the tile kernel, "tail" = the greedy kernels):

1. analog search: tests/network_cases.py's analogue families scaled to about `--families_nodes` nodes (template t at the precursor
   of template t mod 25) as queries against a library of the same size drawn with another seed, at the case's max_shift (50),
   top_n = 1 and top_n = 0, and against themselves (the other seed's compounds give no hits; a self-search gives every family's
   links twice) -- and `fal_network_edges` on the query nodes in the same session: `net_tile_kernel`'s pairs in scope
   per second are the yardstick of `lib_tile_kernel`'s (the work per pair is the same plus the orientation swap).
2. exact search: the medoids of `--n` synthetic spectra (`synth.generate_device`, seed 42; default nearest-neighbour clustering),
   per precursor charge, against the spectra of that charge among `--library_n` more (seed 43) at 20 ppm: the sparse regime, with
   the lane arithmetic (pairs in scope over the 4,096 pair slots of every launched workgroup).  Untuned.
3. yardstick: the numpy restatement (tests/library_cases.py) on `--sample` consecutive queries (in precursor order) of the
   families against the library entries in their scope, checked against the device's bits and scaled by the pairs in scope.

Pairs in scope are counted with a float64 search over the sorted float32 precursors (the float32 rule differs at one-ulp
boundaries only).  The report goes to `--out`.

    python tools/library_rate.py [--n 1000000] [--library_n 100000] [--families_nodes 100000] [--sample 300]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SIDE = ("mz", "intensity", "indptr", "rows", "precursor_mz")


def pairs_in_range(q_pmz, l_pmz, lo_of, hi_of):
    """(query, library) pairs with lo_of(q) <= l <= hi_of(q), and the 64 x 64 tiles a search over the sorted sides launches"""
    q, l = np.sort(np.asarray(q_pmz, np.float64)), np.sort(np.asarray(l_pmz, np.float64))
    first, end = np.searchsorted(l, lo_of(q), side="left"), np.searchsorted(l, hi_of(q), side="right")
    pairs = int((end - first).sum())
    t0 = np.arange(0, len(q), 64)
    t1 = np.minimum(t0 + 63, len(q) - 1)
    chunks = np.maximum(end[t1] - first[t0] + 63, 0) // 64
    return pairs, int(chunks.sum())


def pairs_in_scope_self(pmz, max_shift):
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
    ap.add_argument("--library_n", type=int, default=100_000)
    ap.add_argument("--fragment_tol", type=float, default=0.05)
    ap.add_argument("--families_nodes", type=int, default=100_000)
    ap.add_argument("--sample", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip_exact", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "library", "library_rate.txt"))
    a = ap.parse_args()
    import torch
    from falcon_amd import synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    from tests import library_cases as lc
    from tests import network_cases as nc
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x if isinstance(x, str) else json.dumps(x))

    med = lambda v: round(float(np.median(v)), 3)
    rate = lambda n, ms: round(n / (ms * 1e-3)) if ms > 0 else None
    dev = torch.device("cuda", 0)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.plan(0)
    c.enable_timing(True)
    say(f"library_rate: medians of {a.reps} passes after {a.warmup} warm-ups, HIP events and stage timers; fragment_tol = "
        f"{a.fragment_tol}; device {torch.cuda.get_device_name(0)}")

    # ---- 1. analog search, and the network's tile kernel on the same nodes --------------------------------------------------------
    an = nc.ANALOGUE
    n_templates = max(1, a.families_nodes // 15)
    q = nc.analogue_case(seed=1, n_templates=n_templates, wrap=25)
    l = nc.analogue_case(seed=2, n_templates=n_templates, wrap=25)
    dq, dl = ({k: c.to_dev(s[k]) for k in SIDE} for s in (q, l))
    shift = an["max_shift"]
    pairs, wgs = pairs_in_range(q["precursor_mz"], l["precursor_mz"], lambda x: x - shift, lambda x: x + shift)
    analog = {}
    room = max(4 * len(q["rows"]), 1 << 22)            # (one call a pass: the hits of top_n = 0 fit)

    def analog_pass(name, dlib, n_lib, pairs, wgs, top_n):
        ms, out = timed(c, lambda: c.library_search(*(dq[k] for k in SIDE), *(dlib[k] for k in SIDE), an["fragment_tol"], 20.0, False,
                                                    True, shift, an["min_cosine"], an["min_matched"], top_n, max_hits=room),
                        a.warmup, a.reps)
        tile, greedy = med(ms[:, 1]), med(ms[:, 2])
        rec = dict(measure=name, top_n=top_n, queries=len(q["rows"]), library=n_lib, max_shift=shift, pairs_in_scope=pairs,
                   workgroups=wgs, lanes_busy_share=round(pairs / max(wgs * 4096, 1), 4), greedy_pairs=c.counter(14),
                   hits=int(out[0].numel()), call_ms=med(ms[:, 0]), tile_kernel_ms=tile, greedy_kernel_ms=greedy,
                   call_ms_all=[round(float(x), 3) for x in ms[:, 0]], greedy_pairs_per_s_kernel=rate(c.counter(14), greedy),
                   pairs_per_s_tile_kernel=rate(pairs, tile))
        say(rec)
        return rec

    for top_n in (1, 0):
        analog[top_n] = analog_pass("analog", dl, len(l["rows"]), pairs, wgs, top_n)
    # (another seed's compounds are no analogues of the queries': no hits, few greedy pairs.  The queries as their own library:
    # every family's links in both directions and every node's hit on itself -- the greedy kernels and the two sort passes at work)
    self_pairs, self_wgs = pairs_in_range(q["precursor_mz"], q["precursor_mz"], lambda x: x - shift, lambda x: x + shift)
    for top_n in (1, 0):
        analog_pass("analog_self", dq, len(q["rows"]), self_pairs, self_wgs, top_n)
    net_pairs = pairs_in_scope_self(q["precursor_mz"], shift)
    ms, out = timed(c, lambda: c.network_edges(*(dq[k] for k in SIDE), an["fragment_tol"], shift, an["min_cosine"], an["min_matched"], 0),
                    a.warmup, a.reps)
    net = dict(measure="network_same_nodes", nodes=len(q["rows"]), pairs_in_scope=net_pairs, greedy_pairs=c.counter(12),
               edges=int(out[0].numel()), call_ms=med(ms[:, 0]), tile_kernel_ms=med(ms[:, 1]), greedy_kernel_ms=med(ms[:, 2]),
               pairs_per_s_tile_kernel=rate(net_pairs, med(ms[:, 1])))
    say(net)
    if net["pairs_per_s_tile_kernel"] and analog[0]["pairs_per_s_tile_kernel"]:
        say(dict(measure="lib_tile_over_net_tile", per_pair_in_scope=round(analog[0]["pairs_per_s_tile_kernel"] /
                                                                            net["pairs_per_s_tile_kernel"], 4)))

    # ---- 3. yardstick: the numpy restatement on consecutive queries of the families ------------------------------------------------
    r = lc.rule(True, max_shift=shift)
    order = np.argsort(q["precursor_mz"], kind="stable")
    take = np.sort(order[len(order) // 2:len(order) // 2 + a.sample])
    sq = nc.permute_nodes(q, take)
    lo, hi = float(sq["precursor_mz"].min()) - shift - 1.0, float(sq["precursor_mz"].max()) + shift + 1.0
    lt = np.flatnonzero((l["precursor_mz"] >= lo) & (l["precursor_mz"] <= hi))
    lt = lt[::max(1, len(lt) // (4 * a.sample))]                 # (a few library entries a query: the restatement is slow)
    sl = nc.permute_nodes(l, lt)
    t0 = time.perf_counter()
    want = lc.search_ref(sq, sl, an["fragment_tol"], r, an["min_cosine"], an["min_matched"], 1)
    t_np = time.perf_counter() - t0
    got = tuple(t.cpu().numpy() for t in c.library_search(*(sq[k] for k in SIDE), *(sl[k] for k in SIDE), an["fragment_tol"], 20.0,
                                                          False, True, shift, an["min_cosine"], an["min_matched"], 1))
    sub_pairs, _ = pairs_in_range(sq["precursor_mz"], sl["precursor_mz"], lambda x: x - shift, lambda x: x + shift)
    scaled = t_np * pairs / max(sub_pairs, 1)
    say(dict(measure="numpy_restatement", sample_queries=len(take), sample_library=len(lt), sample_pairs_in_scope=sub_pairs,
             sample_s=round(t_np, 3), sample_equals_device=bool(lc.same_hits(got, want)), scaled_to_analog_s=round(scaled, 1),
             numpy_over_device=round(scaled / (analog[1]["call_ms"] * 1e-3)) if analog[1]["call_ms"] > 0 else None))
    del dq, dl

    # ---- 2. exact search: the sparse regime ----------------------------------------------------------------------------------------
    if not a.skip_exact:
        data = synth.generate_device(a.n, dev, seed=42)
        ref = synth.generate_device(a.library_n, dev, seed=43)
        ppm = 20.0
        tot = dict(queries=0, library=0, pairs_in_scope=0, workgroups=0, greedy_pairs=0, hits=0, call_ms=0.0, tile_kernel_ms=0.0,
                   greedy_kernel_ms=0.0)
        for charge in (2, 3):
            d, lb = synth.select_charge_device(data, charge), synth.select_charge_device(ref, charge)
            ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
            _, medoids = pipe.run(ds, ppm, "ppm", None, a.fragment_tol, 2 ** 15, AnnParams(eps=0.1))
            medoids = medoids.to(torch.int32).contiguous()
            pmz = d["precursor_mz"][medoids.long()].contiguous()
            l_rows = torch.arange(int(lb["precursor_mz"].numel()), dtype=torch.int32, device=dev)
            w = ppm * 1e-6
            pairs, wgs = pairs_in_range(pmz.cpu().numpy(), lb["precursor_mz"].cpu().numpy(), lambda x: x / (1.0 + w), lambda x: x / (1.0 - w))
            ms, out = timed(c, lambda: c.library_search(d["mz"], d["intensity"], d["indptr"], medoids, pmz, lb["mz"], lb["intensity"],
                                                        lb["indptr"], l_rows, lb["precursor_mz"], a.fragment_tol, ppm, False, False,
                                                        200.0, 0.7, 6, 1), a.warmup, a.reps)
            rec = dict(measure="exact", charge=charge, queries=int(medoids.numel()), library=int(l_rows.numel()), precursor_tol_ppm=ppm,
                       pairs_in_scope=pairs, workgroups=wgs, lanes_busy_share=round(pairs / max(wgs * 4096, 1), 4),
                       greedy_pairs=c.counter(14), hits=int(out[0].numel()), call_ms=med(ms[:, 0]), tile_kernel_ms=med(ms[:, 1]),
                       greedy_kernel_ms=med(ms[:, 2]), call_ms_all=[round(float(x), 3) for x in ms[:, 0]],
                       pairs_per_s_tile_kernel=rate(pairs, med(ms[:, 1])), pairs_per_s_call=rate(pairs, med(ms[:, 0])))
            say(rec)
            for k in tot:
                tot[k] += rec[k]
        tot["lanes_busy_share"] = round(tot["pairs_in_scope"] / max(tot["workgroups"] * 4096, 1), 4)
        tot["pairs_per_s_tile_kernel"] = rate(tot["pairs_in_scope"], tot["tile_kernel_ms"])
        say(dict(measure="exact_total", n=a.n, library_n=a.library_n,
                 **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in tot.items()}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
