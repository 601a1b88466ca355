"""The GraphML export's rate (`graphml_io.write`, `Context.format_records`): the host writer of record and the device path on the
same blocks in one session.

The workload is tools/network_rate.py's: tests/network_cases.py's analogue families scaled to about `--nodes` nodes, the links
`fal_network_edges` returns at top_k = 10, their molecular families (cap 100), every tenth node annotated from a synthetic string
table of `--library` rows (names with markup characters and quotes, SMILES, InChIKeys), the annotations carried 3 hops.  One charge.

The device path step by step -- the tables (`graphml_io.tables`: host gathers, the string blobs, the uploads), the two sizing
calls, formatting plus the copy to the host, the file write -- and end to end through `graphml_io.write`, as the median of `--reps`
passes after `--warmup` warm-ups; the host writer (`graphml_io.write_graphml`) on the whole file if a first pass over
`--host_sample` nodes and links says it takes under a minute, otherwise on that sample, scaled.  The two files are compared.  The
report goes to `--out`.

    python tools/graphml_rate.py [--nodes 100000]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def string_table(rows: int):
    text = lambda f: np.array([f(i) for i in range(rows)], dtype=str)
    return dict(library_id=text(lambda i: f"CCMSLIB{i:011d}"), name=text(lambda i: f'Compound {i}, "form {i % 7}" <{i % 13}-O-acyl> & salt'),
                library_file=text(lambda i: "GNPS-LIBRARY.mgf"), adduct=text(lambda i: ("M+H", "M+Na", "", "M+NH4")[i % 4]),
                smiles=text(lambda i: "CC(C)CC1=CC=C(C=C1)C(C)C(=O)O" + "C" * (i % 40)), inchikey=text(lambda i: f"HEFNNWSXXWATRW-{i:010d}-N"))


def workload(c, pipe, n_nodes: int, library_rows: int):
    """-> the one charge block of `graphml_io`"""
    import torch
    from falcon_amd.cluster import cluster as fcl
    from tests import network_cases as nc
    nodes = nc.analogue_case(seed=1, n_templates=max(1, n_nodes // 15), wrap=25)
    an = nc.ANALOGUE
    dn = {k: c.to_dev(nodes[k]) for k in ("mz", "intensity", "indptr", "rows", "precursor_mz")}
    n = len(nodes["rows"])
    u, v, sim, matched = c.network_edges(dn["mz"], dn["intensity"], dn["indptr"], dn["rows"], dn["precursor_mz"], an["fragment_tol"],
                                         an["max_shift"], an["min_cosine"], an["min_matched"], 10)
    pmz = np.asarray(nodes["precursor_mz"], np.float32)
    hu, hv = u.cpu().numpy(), v.cpu().numpy()
    net = fcl.network_families(dict(a=hu, b=hv, similarity=sim, matched=matched, delta_mz=pmz[hv] - pmz[hu]), n, 100, 0.02, pipeline=pipe)
    net.update(charge="2", first=0)
    named = np.arange(0, n, 10)
    lib = string_table(library_rows)
    rng = np.random.default_rng(3)
    hits = dict(lib, cluster=named.astype(np.int32), library=(named % library_rows).astype(np.int32),
                similarity=rng.uniform(0.7, 1.0, len(named)).astype(np.float32), matched=rng.integers(6, 40, len(named)).astype(np.int32),
                delta_mz=rng.normal(0, 0.01, len(named)).astype(np.float32), charge="2", first=0)
    seed = np.full(n, -1, np.int32)
    seed[named] = np.arange(len(named))
    source, hops, _, score, _, _ = c.network_propagate(net["a"], net["b"], net["similarity"], n, seed, 3, 0.0)
    source, hops, score = source.cpu().numpy(), hops.cpu().numpy(), score.cpu().numpy()
    reached = np.flatnonzero(hops >= 0).astype(np.int32)
    ann = dict(lib, cluster=reached, hops=hops[reached], source=source[reached], score=score[reached],
               library=hits["library"][seed[source[reached]]], n_families=net["n_families"], charge="2", first=0)
    torch.cuda.synchronize()
    return dict(charge="2", first=0, precursor_mz=pmz, retention_time=rng.uniform(0, 3600, n).astype(np.float32),
                size=rng.integers(1, 50, n).astype(np.int32), network=net, library=hits, annotations=ann)


def cut(block, n_nodes: int, n_links: int):
    """the block's first clusters and links: the host writer's sample"""
    net, lib, ann = block["network"], block["library"], block["annotations"]
    per = lambda d, keys, keep: dict(d, **{k: d[k][keep] for k in keys})
    return dict(block, precursor_mz=block["precursor_mz"][:n_nodes], retention_time=block["retention_time"][:n_nodes], size=block["size"][:n_nodes],
                network=dict(per(net, ("a", "b", "similarity", "matched", "delta_mz", "family"), slice(0, n_links)),
                             node_family=net["node_family"][:n_nodes], node_size=net["node_size"][:n_nodes]),
                library=per(lib, ("cluster", "library", "similarity", "matched", "delta_mz"), lib["cluster"] < n_nodes),
                annotations=per(ann, ("cluster", "hops", "source", "score", "library"), ann["cluster"] < n_nodes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--library", type=int, default=5000)
    ap.add_argument("--host_sample", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "network", "graphml_rate.txt"))
    a = ap.parse_args()
    import torch
    from falcon_amd.cluster.cluster import ClusterPipeline
    from falcon_amd.ms_io import graphml_io as G
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x if isinstance(x, str) else json.dumps(x))

    med = lambda v: round(float(np.median(v)), 4)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.plan(0)
    say(f"graphml_rate: medians of {a.reps} passes after {a.warmup} warm-ups, wall clock around synchronising calls; device "
        f"{torch.cuda.get_device_name(0)}")
    block = workload(c, pipe, a.nodes, a.library)
    blocks, header, sw = [block], ["falcon version rate", "network = True", "network_families = True"], (True, True, True)
    n, m = len(block["size"]), len(block["network"]["a"])
    say(dict(nodes=n, links=m, families=int(block["network"]["n_families"]), nodes_with_a_hit=len(block["library"]["cluster"]),
             nodes_with_an_annotation=len(block["annotations"]["cluster"]), library_rows=a.library))
    tmp = tempfile.mkdtemp()

    # ---- the host writer ---------------------------------------------------------------------------------------------------------------
    def host_pass(bl, path):
        t0 = time.perf_counter()
        with open(path, "w", encoding="utf-8", newline="\n") as f:
            G.write_graphml(f, header, bl, *sw)
        return time.perf_counter() - t0

    k_nodes, k_links = min(a.host_sample, n), min(a.host_sample * max(m, 1) // max(n, 1), m)
    sample_s = host_pass([cut(block, k_nodes, k_links)], os.path.join(tmp, "sample.graphml"))
    scaled = sample_s * (n + m) / max(k_nodes + k_links, 1)
    rec = dict(host_writer_sample_s=round(sample_s, 3), sample_nodes=k_nodes, sample_links=k_links, scaled_to_the_file_s=round(scaled, 2))
    whole = scaled < 60.0
    if whole:
        rec["host_writer_whole_file_s"] = round(host_pass(blocks, os.path.join(tmp, "host.graphml")), 3)
    host_s = rec["host_writer_whole_file_s"] if whole else scaled
    say(rec)

    # ---- the device path, step by step ----------------------------------------------------------------------------------------------
    steps = {k: [] for k in ("tables_s", "sizing_s", "format_and_copy_s", "file_write_s", "end_to_end_s")}
    path = os.path.join(tmp, "device.graphml")
    for rep in range(a.warmup + a.reps):
        t = [time.perf_counter()]
        both, why = G.tables(blocks, c, *sw)
        assert why is None, why
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        sized = []
        for table in both:
            cols = c._records_table(table)
            sized.append((cols, c.records_write_sizes(cols)))
        t.append(time.perf_counter())
        chunks = []
        for cols, (_, offsets, _) in sized:
            chunks += list(c._write_chunks(cols["n"], offsets, None, True, lambda x, y, d, h: c.records_write(cols, offsets, x, y, d, h)))
        t.append(time.perf_counter())
        with open(path, "wb") as f:
            f.write(G.prologue(header, sw).encode("utf-8"))
            for chunk in chunks:
                f.write(memoryview(chunk))
            f.write(G.EPILOGUE.encode("ascii"))
        t.append(time.perf_counter())
        G.write(os.path.join(tmp, "end_to_end"), header, blocks, c, "device", *sw)
        t.append(time.perf_counter())
        if rep >= a.warmup:
            for k, dt in zip(steps, np.diff(t)):
                steps[k].append(dt)
    size = os.path.getsize(path)
    rec = {k: med(v) for k, v in steps.items()}
    rec.update(file_bytes=size, format_and_copy_GB_per_s=round(size / med(steps["format_and_copy_s"]) / 1e9, 3),
               end_to_end_all_s=[round(float(x), 4) for x in steps["end_to_end_s"]])
    say(rec)
    same = None
    if whole:
        same = open(path, "rb").read() == open(os.path.join(tmp, "host.graphml"), "rb").read() == \
            open(os.path.join(tmp, "end_to_end.network.graphml"), "rb").read()
    say(dict(host_writer_s=round(host_s, 3), host_timed_on="the whole file" if whole else "the sample, scaled",
             device_end_to_end_s=rec["end_to_end_s"], host_over_device=round(host_s / rec["end_to_end_s"], 1), files_equal=same))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
