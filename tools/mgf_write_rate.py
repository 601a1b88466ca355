"""The representative MGF's export rate on BASELINE configs[1]'s workload: 1 M synthetic spectra (`synth.generate_device`, seed 42),
both precursor charges, labels and medoids from the default nearest-neighbour path, then the export of every cluster's
representative -- the medoid's peaks, and the consensus peaks (`fal_consensus_spectra`) -- with both writers.

Prints per charge and representative form: entries, peaks, bytes written, the host writer (`mgf_io.write_spectra`, file write
included) timed on a uniform sample of `--sample` entries and SCALED to all entries, the device stage (`Context.format_mgf`:
sizes, format and the copies to pinned host memory, HIP events around the whole generator, median and minimum of `--reps`
passes after `--warmup` warm-ups) and the whole device export (`mgf_io.write_representatives`: title blob, device stage and the
file write, host clock), and whether the sample's entries are the same bytes from both writers.  Then one JSON line with the
totals of each form.

    python tools/mgf_write_rate.py [--n 1000000] [--reps 5] [--warmup 2] [--sample 5000] [--dir DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--fragment_tol", type=float, default=0.05)
    ap.add_argument("--min_fraction", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5, help="timed passes of the device stage")
    ap.add_argument("--warmup", type=int, default=2, help="passes of the device stage before the timed ones")
    ap.add_argument("--sample", type=int, default=5000, help="entries the host writer is timed on (scaled to all)")
    ap.add_argument("--dir", type=str, default=None, help="where the files are written (default: a temporary directory)")
    a = ap.parse_args()
    import torch
    from falcon_amd import synth
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset
    from falcon_amd.ms_io import mgf_io
    dev = torch.device("cuda", 0)
    data = synth.generate_device(a.n, dev, seed=42)
    pipe = ClusterPipeline(device=0)
    c = pipe.ctx
    c.plan(0)
    p = AnnParams(eps=a.eps)
    keys = ("entries", "peaks", "bytes", "host_scaled_ms", "device_stage_ms", "device_stage_min_ms", "device_export_ms")
    tot = {form: dict.fromkeys(keys, 0) for form in ("medoid", "consensus")}
    base = 0
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for charge in (2, 3):
            d = synth.select_charge_device(data, charge)
            ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
            labels, medoids = pipe.run(ds, 20.0, "ppm", None, a.fragment_tol, 2 ** 15, p)
            labels, medoids = labels.to(torch.int32).contiguous(), medoids.to(torch.int32).contiguous()
            nc = int(medoids.shape[0])
            m64 = medoids.to(torch.int64)
            pmz, rt = d["precursor_mz"][m64].contiguous(), d["retention_time"][m64].contiguous()
            cluster = labels.to(torch.int64)[m64] + base
            base += nc
            ch = torch.full((nc,), charge, dtype=torch.int32, device=dev)
            titles = np.char.add("scan=", medoids.cpu().numpy().astype(str))
            cons = c.consensus_spectra(d["mz"], d["intensity"], d["indptr"], labels, medoids, a.fragment_tol, a.min_fraction)
            forms = {"medoid": (d["mz"], d["intensity"], d["indptr"], medoids),
                     "consensus": (cons[1], cons[2], cons[0], torch.arange(nc, dtype=torch.int32, device=dev))}
            for form, (mz, it, ip, rows) in forms.items():
                cols = (mz, it, ip, rows, pmz, rt, ch, cluster)
                blob = mgf_io.title_blob(titles)

                def stage():
                    n_bytes = 0
                    for chunk in c.format_mgf(*cols, blob[0], blob[1], copy=False):
                        n_bytes += len(chunk)
                    return n_bytes
                for _ in range(a.warmup):
                    stage()
                torch.cuda.synchronize()
                times = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    n_bytes = stage()
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                fn = os.path.join(tmp, f"device_{form}_{charge}.mgf")
                t0 = time.perf_counter()
                wrote = mgf_io.write_representatives(fn, c, *cols, titles)
                export_ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(fn)
                os.remove(fn)
                # the host writer on a uniform sample of the entries, and the device writer on the same entries
                rng = np.random.default_rng(0)
                sample = np.sort(rng.choice(nc, size=min(a.sample, nc), replace=False))
                st = torch.from_numpy(sample).to(dev)
                sub = (mz, it, ip, rows[st], pmz[st], rt[st], ch[st], cluster[st])
                host_cols = [t.cpu().numpy() for t in sub]
                fh = os.path.join(tmp, "host_sample.mgf")
                t0 = time.perf_counter()
                mgf_io.write_spectra(fh, mgf_io.entry_dicts(*host_cols, titles[sample]))
                host_ms = (time.perf_counter() - t0) * 1e3
                fd = os.path.join(tmp, "device_sample.mgf")
                mgf_io.write_representatives(fd, c, *sub, titles[sample])
                same = open(fh, "rb").read() == open(fd, "rb").read()
                n_peaks = int((ip[rows.to(torch.int64) + 1] - ip[rows.to(torch.int64)]).sum().item())
                row = dict(charge=charge, representatives=form, entries=nc, peaks=n_peaks, bytes=size, writer=wrote,
                           host_sample=len(sample), host_sample_ms=round(host_ms, 1),
                           host_scaled_ms=round(host_ms * nc / len(sample), 1), device_stage_ms=round(float(np.median(times)), 3),
                           device_stage_min_ms=round(float(min(times)), 3), device_export_ms=round(export_ms, 1),
                           sample_bytes_equal=bool(same), stage_bytes_equal_file=bool(n_bytes == size))
                print(row, flush=True)
                for k in keys:
                    tot[form][k] += row[k]
    for form, t in tot.items():
        t = {k: round(v, 3) if isinstance(v, float) else v for k, v in t.items()}
        t["host_over_device_export"] = round(t["host_scaled_ms"] / t["device_export_ms"], 1) if t["device_export_ms"] > 0 else None
        t["device_stage_gb_per_s"] = round(t["bytes"] / t["device_stage_ms"] / 1e6, 2) if t["device_stage_ms"] > 0 else None
        print(json.dumps(dict(tool="mgf_write_rate", n=a.n, eps=a.eps, representatives=form, reps=a.reps, warmup=a.warmup, **t)),
              flush=True)


if __name__ == "__main__":
    main()
