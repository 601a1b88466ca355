"""The graph tail of a big job, per charge partition: `python tools/graph_tail_10m.py 10000000 <tag>` runs the 10 M float32
configuration (precursors 400-1,200 m/z, low_dim 400) four times and prints, for every pass after the first and each partition,
its bucket table, the dbscan / tail stage times and which graph-tail path ran (`fal_ctx_counter(10)`; -1: a library without it).
profiles/NOTES.md, "Graph tail per bucket tile", holds the figures."""
import sys, time, json, numpy as np, torch
sys.path.insert(0, '.')
from falcon_amd import synth, device as dv
from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
N = int(sys.argv[1]); tag = sys.argv[2]
ctx = dv.Context(0); pipe = ClusterPipeline(ctx)
data = synth.generate_device(N, ctx.tdev, mz_lo=400.0, mz_hi=1200.0)
p = AnnParams(scan="f32", n_probe=16, dtype="f32", low_dim=400)
parts = []
for ch in (2, 3):
    c = synth.select_charge_device(data, ch)
    parts.append(SpectrumDataset(*[ctx.to_dev(c[k], torch.float32) for k in ("precursor_mz", "retention_time", "mz", "intensity")], ctx.to_dev(c["indptr"], torch.int64)))
del data
REPS = 4
out = []
for rep in range(REPS):
    timed = rep >= 1
    ctx.enable_timing(timed)
    for pi, ds in enumerate(parts):
        labels, medoids = pipe.run(ds, 20.0, "ppm", None, 0.05, 2 ** 15, p)
        if timed:
            sizes = np.diff(np.asarray(pipe.last["splits"]))
            try:
                path = ctx.counter(10)
            except Exception:
                path = -1
            out.append(dict(tag=tag, rep=rep, charge=2 + pi, rows=len(ds), buckets=len(sizes), max_bucket=int(sizes.max()),
                            median_bucket=int(np.median(sizes)), dbscan=round(ctx.stage_ms("dbscan")[0], 3),
                            tail=round(ctx.stage_ms("tail")[0], 3), tiled=path, clusters=int(medoids.numel())))
            print("CFG", json.dumps(out[-1]), flush=True)
