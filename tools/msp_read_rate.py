"""MSP library input rate: `falcon._load_annotation_library` (`--library lib.msp`) with the host reader against the device reader
on the same synthetic MSP file, and -- the yardstick for the device passes -- the MGF device reader on the same entries written
as MGF, all in one session.

Writes, for every `--n`, a synthetic library of n entries (Name, SpectrumID, PrecursorMZ, Charge, Precursor_type, SMILES,
InChIKey, Ion_mode, Comments, Num Peaks; repr() numbers; peak lists drawn from a pool of 1000 seeded lists of 10 to 60 peaks,
every second entry four peaks a line with `;`) as `.msp` and the same entries as a GNPS-style `.mgf`, then reports per file and
reader:
  load_s           the loader end to end (wall clock behind a stream synchronise): median of `--repeats` runs after `--warmups`
                   (`--host_repeats` / `--host_warmups` for the host reader)
  entries_per_s    entries of the file over load_s
and for a device reader, from its last run, the stages in seconds:
  parse_and_headers   `Context.parse_msp` / `parse_mgf`: upload, index, parse, headers, column copies
  string_columns      `mgf_io._text_column`: `fal_text_rows` and the str arrays made of its rows
  process_spectra     `falcon._process`: `fal_process_spectra` and its result copies
  file_read_and_rest  everything else: the file read and cut, the column rules, HOST re-reads
  host_share          entries the host rule read again, over the entries of the file
then one JSON line per file and reader, also appended to `--out`.

    python tools/msp_read_rate.py [--n 100000,1000000] [--dir /tmp/mspfiles] [--out profiles/library/msp_read_rate.txt]
"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.peakfile_rate import _Timed  # noqa: E402


def _peak_pool(rng, size=1000):
    """-> per list its peak texts ("mz intensity")"""
    pool = []
    for _ in range(size):
        k = int(rng.integers(10, 61))
        mz, it = np.sort(rng.uniform(50.0, 1500.0, k)), rng.uniform(1.0, 1e5, k)
        pool.append([f"{float(m)!r} {float(np.float32(v))!r}" for m, v in zip(mz, it)])
    return pool


def write_both(msp_fn, mgf_fn, n, seed=42):
    rng = np.random.default_rng(seed)
    pool = _peak_pool(rng)
    as_lines = ["".join(p + "\n" for p in peaks) for peaks in pool]
    as_rows = ["".join("; ".join(peaks[j:j + 4]) + "\n" for j in range(0, len(peaks), 4)) for peaks in pool]
    pmz, pick, z = rng.uniform(100.0, 1500.0, n), rng.integers(0, len(pool), n), rng.integers(0, 4, n)
    with open(msp_fn, "w") as msp, open(mgf_fn, "w") as mgf:
        for i in range(n):
            smiles, key = f"CC(=O)OC1=CC=CC=C1C(=O)O{i % 97}", f"KEY{i:011d}-UHFFFAOYSA-N"
            msp.write(f"Name: Compound {i} M+H\nSpectrumID: CCMSLIB{i:011d}\nPrecursorMZ: {float(pmz[i])!r}\nCharge: {z[i]}\n"
                      f"Precursor_type: M+H\nSMILES: {smiles}\nInChIKey: {key}\nIon_mode: Positive\nComments: \"scan={i + 1}\" \"synthetic\"\n"
                      f"Num Peaks: {len(pool[pick[i]])}\n{(as_rows if i % 2 else as_lines)[pick[i]]}\n")
            mgf.write(f"BEGIN IONS\nPEPMASS={float(pmz[i])!r}\nCHARGE={z[i]}\nIONMODE=Positive\nNAME=Compound {i} M+H\nADDUCT=M+H\n"
                      f"SMILES={smiles}\nINCHIKEY={key}\nSPECTRUMID=CCMSLIB{i:011d}\nSCANS={i + 1}\n{as_lines[pick[i]]}END IONS\n\n")


def measure(ctx, fn, reader, repeats, warmups, work):
    """the library loader on one file with one reader -> the JSON row"""
    import torch
    from falcon_amd import falcon
    from falcon_amd.config import config
    from falcon_amd.ms_io import mgf_io, msp_io
    msp = fn.lower().endswith(".msp")
    config.parse([os.path.join(work, "in.mgf"), os.path.join(work, "out"), "--library", fn, "--msp_reader" if msp else "--mgf_reader", reader])
    owner = msp_io if msp else mgf_io
    inner = owner.read_annotation_chunks
    counts, acc, runs, kept, s = {}, {}, [], 0, 0.0

    def counted(filenames, c, cnt=None, **kw):
        out = inner(filenames, c, counts, **kw)
        if cnt is not None:
            cnt.update(counts)
        return out

    for k in range(warmups + repeats):
        acc.clear()
        timers = [_Timed(acc, ctx, "parse_msp" if msp else "parse_mgf", "parse_and_headers"), _Timed(acc, mgf_io, "_text_column", "string_columns"),
                  _Timed(acc, falcon, "_process", "process_spectra")]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.ExitStack() as stack:
            for t in timers:
                stack.enter_context(t)
            owner.read_annotation_chunks = counted
            try:
                got = falcon._load_annotation_library(ctx)
            finally:
                owner.read_annotation_chunks = inner
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        kept = len(got["precursor_mz"])
        del got
        if k >= warmups:
            runs.append(s)
        print(f"  {os.path.basename(fn)} {reader} run {k + 1}: {s:.2f} s", flush=True)
    row = dict(tool="msp_read_rate", file="msp" if msp else "mgf", reader=reader, text_bytes=os.path.getsize(fn), kept_after_preprocessing=kept,
               load_s=round(float(np.median(runs)), 3), runs=len(runs), warmups=warmups, all_runs_s=[round(r, 3) for r in runs])
    if reader == "device":
        entries = counts.get("entries")
        acc["file_read_and_rest"] = s - sum(acc.values())
        stages = {k: round(v, 3) for k, v in sorted(acc.items())}
        row.update(stages_s=stages, parse_and_headers_ns_per_byte=round(1e9 * acc.get("parse_and_headers", 0.0) / row["text_bytes"], 3),
                   host_reread_entries=counts.get("host"), host_share=None if not entries else round(counts["host"] / entries, 6))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100000", help="entries of the synthetic libraries")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--host_repeats", type=int, default=5)
    ap.add_argument("--host_warmups", type=int, default=2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "library", "msp_read_rate.txt"))
    a = ap.parse_args()
    from falcon_amd.device import Context
    work = a.dir or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    jobs = []
    for n in [int(v) for v in a.n.split(",") if v]:
        msp_fn, mgf_fn = os.path.join(work, f"library_{n}.msp"), os.path.join(work, f"library_{n}.mgf")
        t0 = time.perf_counter()
        write_both(msp_fn, mgf_fn, n)
        print(f"wrote {n} entries as MSP ({os.path.getsize(msp_fn)} bytes) and MGF ({os.path.getsize(mgf_fn)} bytes) in "
              f"{time.perf_counter() - t0:.1f} s", flush=True)
        jobs += [(msp_fn, "device", n), (mgf_fn, "device", n), (msp_fn, "host", n)]
    ctx = Context(0)
    ctx.plan(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for fn, reader, n in jobs:
            rep, warm = (a.repeats, a.warmups) if reader == "device" else (a.host_repeats, a.host_warmups)
            row = measure(ctx, fn, reader, rep, warm, work)
            row.update(entries=n, entries_per_s=round(n / row["load_s"]))
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
    ctx.close()


if __name__ == "__main__":
    main()
