"""Library and representative MGF input rate: `falcon._load_annotation_library` (`--library`) and `falcon._load_library`
(`--assign_to`) with the host readers against the device readers, on the same files in one session.

Writes a synthetic GNPS-style library (no TITLE; SPECTRUMID, NAME, COMPOUND_NAME, ADDUCT, SMILES, INCHIKEY, IONMODE; repr()
numbers; peak lists drawn from a pool of 1000 seeded lists of 10 to 60 peaks) of every `--n` entries, and a representative MGF of
`--reps` entries in `mgf_io.write_spectra`'s layout (TITLE, PEPMASS, CHARGE, RTINSECONDS, CLUSTER; the same pool), then reports
per file and reader:
  load_s           the loader end to end (wall clock behind a stream synchronise): median of `--repeats` runs after `--warmups`
                   (`--host_repeats` / `--host_warmups` for the host reader, whose runs take tens of seconds at 1 M entries)
  entries_per_s    entries of the file over load_s
and for the device reader, from its last run, the stages in seconds:
  parse_and_headers   `Context.parse_mgf`: upload, `fal_mgf_index`, `fal_mgf_parse(_ex)`, `fal_mgf_headers`, column copies
  string_columns      `mgf_io._text_column`: `fal_text_rows` and the str arrays made of its rows
  process_spectra     `falcon._process`: `fal_process_spectra` and its result copies
  file_read_and_rest  everything else: the file read and cut, the column rules, HOST re-reads, partitioning, the .npz files
  host_share          entries the host rule read again, over the entries of the file
then one JSON line per file and reader, also appended to `--out`.

    python tools/library_read_rate.py [--n 100000,1000000] [--reps 643000] [--dir /tmp/libfiles] [--out profiles/library/library_read_rate.txt]
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
    pool = []
    for _ in range(size):
        k = int(rng.integers(10, 61))
        mz, it = np.sort(rng.uniform(50.0, 1500.0, k)), rng.uniform(1.0, 1e5, k)
        pool.append("".join(f"{float(m)!r}\t{float(np.float32(v))!r}\n" for m, v in zip(mz, it)))
    return pool


def write_library(fn, n, seed=42):
    rng = np.random.default_rng(seed)
    pool = _peak_pool(rng)
    pmz, pick, z = rng.uniform(100.0, 1500.0, n), rng.integers(0, len(pool), n), rng.integers(0, 4, n)
    with open(fn, "w") as f:
        for i in range(n):
            f.write(f"BEGIN IONS\nPEPMASS={float(pmz[i])!r}\nCHARGE={z[i]}\nMSLEVEL=2\nIONMODE=Positive\nNAME=Compound {i} M+H\n"
                    f"COMPOUND_NAME=Compound {i}\nADDUCT=M+H\nSMILES=CC(=O)OC1=CC=CC=C1C(=O)O{i % 97}\nINCHIKEY=KEY{i:011d}-UHFFFAOYSA-N\n"
                    f"SPECTRUMID=CCMSLIB{i:011d}\nSCANS={i + 1}\n{pool[pick[i]]}END IONS\n\n")


def write_representatives(fn, n, seed=43):
    rng = np.random.default_rng(seed)
    pool = _peak_pool(rng)
    pmz, pick, rt = rng.uniform(300.0, 1500.0, n).astype(np.float32), rng.integers(0, len(pool), n), rng.uniform(0, 7200, n).astype(np.float32)
    with open(fn, "w") as f:
        for i in range(n):
            f.write(f"BEGIN IONS\nTITLE=scan={i + 1}\nPEPMASS={float(pmz[i])!r}\nCHARGE={2 + i % 2}+\nRTINSECONDS={float(rt[i])!r}\n"
                    f"CLUSTER={i}\n{pool[pick[i]]}END IONS\n\n")


def measure(ctx, what, fn, reader, repeats, warmups, work):
    """one loader on one file with one reader -> the JSON row"""
    import torch
    from falcon_amd import falcon
    from falcon_amd.config import config
    from falcon_amd.ms_io import mgf_io
    option = "--library" if what == "library" else "--assign_to"
    config.parse([os.path.join(work, "in.mgf"), os.path.join(work, "out"), option, fn, "--mgf_reader", reader])
    spectra_dir = tempfile.mkdtemp(dir=work)
    load = (lambda: falcon._load_annotation_library(ctx)) if what == "library" else (lambda: falcon._load_library(spectra_dir, ctx))
    counts, acc, runs, kept = {}, {}, [], 0
    chunk_reader = "read_annotation_chunks" if what == "library" else "read_library_chunks"
    inner = getattr(mgf_io, chunk_reader)

    def counted(filenames, c, cnt=None, **kw):
        out = inner(filenames, c, counts, **kw)
        if cnt is not None:
            cnt.update(counts)
        return out

    for k in range(warmups + repeats):
        acc.clear()
        timers = [_Timed(acc, ctx, "parse_mgf", "parse_and_headers"), _Timed(acc, mgf_io, "_text_column", "string_columns"),
                  _Timed(acc, falcon, "_process", "process_spectra")]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.ExitStack() as stack:
            for t in timers:
                stack.enter_context(t)
            setattr(mgf_io, chunk_reader, counted)
            try:
                got = load()
            finally:
                setattr(mgf_io, chunk_reader, inner)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        kept = len(got["precursor_mz"]) if what == "library" else sum(len(v["precursor_mz"]) for v in got[0].values())
        del got
        if k >= warmups:
            runs.append(s)
        print(f"  {what} {reader} run {k + 1}: {s:.2f} s", flush=True)
    row = dict(tool="library_read_rate", file=what, reader=reader, text_bytes=os.path.getsize(fn), kept_after_preprocessing=kept,
               load_s=round(float(np.median(runs)), 3), runs=len(runs), warmups=warmups, all_runs_s=[round(r, 3) for r in runs])
    if reader == "device":
        entries = counts.get("entries")
        acc["file_read_and_rest"] = s - sum(acc.values())
        row.update(stages_s={k: round(v, 3) for k, v in sorted(acc.items())}, host_reread_entries=counts.get("host"),
                   host_share=None if not entries else round(counts["host"] / entries, 6))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100000,1000000", help="entries of the synthetic libraries")
    ap.add_argument("--reps", type=int, default=643000, help="entries of the representative MGF (0: skip it)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--host_repeats", type=int, default=5)
    ap.add_argument("--host_warmups", type=int, default=2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "library", "library_read_rate.txt"))
    a = ap.parse_args()
    from falcon_amd.device import Context
    work = a.dir or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    jobs = []
    for n in [int(v) for v in a.n.split(",") if v]:
        fn = os.path.join(work, f"library_{n}.mgf")
        t0 = time.perf_counter()
        write_library(fn, n)
        print(f"wrote {n} library entries, {os.path.getsize(fn)} bytes, in {time.perf_counter() - t0:.1f} s", flush=True)
        jobs.append(("library", fn, n))
    if a.reps:
        fn = os.path.join(work, f"representatives_{a.reps}.mgf")
        t0 = time.perf_counter()
        write_representatives(fn, a.reps)
        print(f"wrote {a.reps} representatives, {os.path.getsize(fn)} bytes, in {time.perf_counter() - t0:.1f} s", flush=True)
        jobs.append(("representatives", fn, a.reps))
    ctx = Context(0)
    ctx.plan(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for what, fn, n in jobs:
            for reader in ("device", "host"):
                rep, warm = (a.repeats, a.warmups) if reader == "device" else (a.host_repeats, a.host_warmups)
                row = measure(ctx, what, fn, reader, rep, warm, work)
                row.update(entries=n, entries_per_s=round(n / row["load_s"]))
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
    ctx.close()


if __name__ == "__main__":
    main()
