"""Peak-file input rate: where the time of reading a peak file goes -- mzML / mzXML: host XML pass against device decode; MGF:
host reader against the device reader.

Writes seeded synthetic MS2 spectra (`synth.generate`, seed 42) as mzML (64-bit m/z, 32-bit intensity, zlib), mzXML (32-bit
pairs, zlib, MS2 nested in MS1) and MGF, with an MS1 spectrum in front of every 10th MS2, then reports per XML format:
  xml_pass_s       the reader's streaming XML pass (`read_chunks`: metadata + base64 payload descriptors)
  host_decode_s    the same payload decoded with stdlib base64 + zlib on one host thread (`PeakChunk.host_spectra`)
  decode_call_ms   `fal_decode_peaks` (device events around the call after one warm-up, the payload already on the device;
                   its six kernels and two scans), and GB/s of base64 in; decode_call_with_upload_ms also copies the payload
  prepare_*        `falcon._prepare_spectra` end to end (read, decode, process_spectrum, partitions) in spectra/s, and the
                   MGF reader's on the same spectra
and for MGF:
  host_parse_s     `list(mgf_io.get_spectra(file))`, the host reader alone
  parse_call_ms    `fal_mgf_index` + `fal_mgf_parse` over the file's chunks with the text already on the device (device events,
                   median of 5 after one warm-up), GB/s of text; parse_call_with_upload_ms also copies the text
  host_share       spectra of the file the device hands back to the host reader
  prepare_s / prepare_host_reader_s   `falcon._prepare_spectra` end to end with `--mgf_reader device` / `host` (the latter is
                   the reader every MGF file went through before the device reader existed)
  prepare_parts_s  the device reader's prepare itemised: file read, parse calls (upload included), identifiers, HOST re-reads
                   and column copies (chunk_other), process_spectra + result copies, partitioning, writing the .npz files
then one JSON line per format.

    python tools/peakfile_rate.py [--n 1000000] [--dir /tmp/peakfiles] [--formats mzML,mzXML,MGF]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _spectra(n):
    from falcon_amd import synth
    d = synth.generate(n, seed=42)
    out = []
    for i in range(n):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        out.append({"identifier": str(i + 1), "precursor_mz": float(d["precursor_mz"][i]),
                    "precursor_charge": int(d["precursor_charge"][i]), "retention_time": float(d["retention_time"][i]),
                    "mz": d["mz"][a:b].astype(np.float64), "intensity": d["intensity"][a:b]})
    return out


def _prepare(fn, work, extra=()):
    from falcon_amd import falcon
    from falcon_amd.cluster import spectrum
    from falcon_amd.config import config
    config.parse([fn, os.path.join(work, "out"), "--work_dir", work, *extra])
    _, min_mz, max_mz = spectrum.get_dim(config.min_mz, config.max_mz, config.fragment_tol)
    os.makedirs(os.path.join(work, "spectra"), exist_ok=True)
    return lambda ctx: falcon._prepare_spectra(os.path.join(work, "spectra"), min_mz, max_mz, ctx)


class _Timed:
    """accumulate the wall time of `owner.name` calls under `key` (restored on exit)"""

    def __init__(self, acc, owner, name, key):
        self.acc, self.owner, self.name, self.key, self.fn = acc, owner, name, key, getattr(owner, name)

    def __enter__(self):
        def wrapped(*a, **k):
            t0 = time.perf_counter()
            try:
                return self.fn(*a, **k)
            finally:
                self.acc[self.key] = self.acc.get(self.key, 0.0) + time.perf_counter() - t0
        setattr(self.owner, self.name, wrapped)

    def __exit__(self, *exc):
        setattr(self.owner, self.name, self.fn)


def _mgf_row(ctx, fn, n, out_dir):
    import contextlib
    import torch
    from falcon_amd import falcon
    from falcon_amd.ms_io import mgf_io
    size = os.path.getsize(fn)
    t0 = time.perf_counter()
    n_host_reader = sum(1 for _ in mgf_io.get_spectra(fn))
    host_s = time.perf_counter() - t0
    # the chunks the reader cuts, as host buffers and as device tensors
    t0 = time.perf_counter()
    texts, buf = [], bytearray()
    with open(fn, "rb") as f:
        while True:
            more = f.read(mgf_io.DEFAULT_CHUNK_BYTES)
            buf += more
            cut = mgf_io._cut(buf, not more)
            if cut:
                texts.append(np.frombuffer(buf[:cut], np.uint8))
                del buf[:cut]
            if not more:
                break
    read_s = time.perf_counter() - t0
    res = ctx.parse_mgf(texts[0])                                       # warm-up: code objects, scratch slots
    ms = {}
    for what in ("with_upload", "on_device"):
        args = texts if what == "with_upload" else [torch.from_numpy(t.copy()).cuda() for t in texts]
        runs = []
        for _ in range(5):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            n_spec = n_hostst = 0
            for t in args:
                d = ctx.to_dev(t) if what == "with_upload" else t
                k, nnz, flags, _ = ctx.mgf_index(d)
                out = ctx.mgf_parse(d, k, nnz)
                n_spec += k
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1))
        ms[what] = float(np.median(runs))
        del args
    n_st = sum(int((ctx.parse_mgf(t)["status"] != 0).sum()) for t in texts)
    del texts, res, out
    row = dict(format="MGF", spectra=n_spec, host_reader_spectra=n_host_reader, text_bytes=size, chunks=len(runs) and None,
               host_parse_s=round(host_s, 2), parse_call_ms=round(ms["on_device"], 2),
               parse_call_with_upload_ms=round(ms["with_upload"], 2), parse_GBps=round(size / (ms["on_device"] * 1e-3) / 1e9, 2),
               host_parse_GBps=round(size / host_s / 1e9, 4), host_share=round(n_st / max(n_spec, 1), 6), file_read_s=round(read_s, 2))
    row.pop("chunks")
    for reader in ("host", "device", "device"):                      # the second device run is the one reported (warm page cache)
        run = _prepare(fn, tempfile.mkdtemp(dir=out_dir), ["--mgf_reader", reader])
        acc = {}
        timers = [_Timed(acc, ctx, "parse_mgf", "parse_calls"), _Timed(acc, mgf_io, "_identifiers", "identifiers"),
                  _Timed(acc, mgf_io, "_device_chunk", "chunk"), _Timed(acc, falcon, "_process", "process_spectra"),
                  _Timed(acc, falcon, "_partition", "partition"), _Timed(acc, np, "savez", "write_npz")] if reader == "device" else []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.ExitStack() as stack:
            for t in timers:
                stack.enter_context(t)
            charges = run(ctx)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        if reader == "host":
            row.update(prepare_host_reader_s=round(s, 2), prepare_host_reader_spectra_per_s=round(n / s))
        else:
            acc["chunk_other"] = acc.pop("chunk", 0.0) - acc.get("identifiers", 0.0)
            acc["file_read_and_cut"] = s - sum(acc.values())
            row.update(prepare_s=round(s, 2), prepare_spectra_per_s=round(n / s), charges=charges,
                       prepare_parts_s={k: round(v, 3) for k, v in sorted(acc.items())})
        print("MGF prepare", reader, round(s, 2), "s", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--formats", default="mzML,mzXML,MGF")
    a = ap.parse_args()
    formats = a.formats.split(",")
    import torch
    from falcon_amd.device import Context
    from falcon_amd.ms_io import ms_io, mzml_io, mzxml_io
    from tests import peakfile_writer as W
    out_dir = a.dir or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.perf_counter()
    spectra = _spectra(a.n)
    files = {"mzML": os.path.join(out_dir, "run.mzML"), "mzXML": os.path.join(out_dir, "run.mzXML"),
             "MGF": os.path.join(out_dir, "run.mgf")}
    if "mzML" in formats:
        W.write_mzml(files["mzML"], spectra, mz_bits=64, int_bits=32, zlib_arrays=True, ms1_every=10)
    if "mzXML" in formats:
        W.write_mzxml(files["mzXML"], spectra, bits=32, zlib_arrays=True, ms1_every=10, nested=True)
    ms_io.write_spectra(files["MGF"], spectra)
    del spectra
    print(f"wrote {a.n} spectra in {time.perf_counter() - t0:.1f} s:",
          {k: os.path.getsize(v) for k, v in files.items() if os.path.isfile(v)}, flush=True)
    ctx = Context(0)
    ctx.plan(0)
    rows = {}
    for fmt, reader in (("mzML", mzml_io), ("mzXML", mzxml_io)):
        if fmt not in formats:
            continue
        t0 = time.perf_counter()
        chunks = list(reader.read_chunks(files[fmt]))
        xml_s = time.perf_counter() - t0
        n_spec = sum(len(c) for c in chunks)
        b64 = sum(c.nbytes for c in chunks)
        t0 = time.perf_counter()
        n_host = sum(1 for c in chunks for _ in c.host_spectra())
        host_s = time.perf_counter() - t0
        tables = [c.tables() for c in chunks]
        ctx.decode_peaks(*tables[0])                                    # warm-up: code objects, scratch slots
        ms = {}
        for what in ("with_upload", "on_device"):
            # on_device: the payload is on the device before the call (the descriptor tables are still uploaded by it)
            args = tables if what == "with_upload" else [(torch.from_numpy(p).cuda(), a_, s_) for p, a_, s_ in tables]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in args:
                st = ctx.decode_peaks(*t)[3]
            e1.record()
            torch.cuda.synchronize()
            ms[what] = e0.elapsed_time(e1)
            del args
        bad = int((st != 0).sum().item())
        del tables, chunks
        kern_ms = ms["on_device"]
        rows[fmt] = dict(format=fmt, spectra=n_spec, host_decoded=n_host, status_nonzero=bad, base64_bytes=b64,
                         xml_pass_s=round(xml_s, 2), host_decode_s=round(host_s, 2), decode_call_ms=round(kern_ms, 2),
                         decode_call_with_upload_ms=round(ms["with_upload"], 2),
                         decode_GBps=round(b64 / (kern_ms * 1e-3) / 1e9, 2), host_decode_GBps=round(b64 / host_s / 1e9, 3))
        print(rows[fmt], flush=True)
    if "MGF" in formats:
        rows["MGF"] = _mgf_row(ctx, files["MGF"], a.n, out_dir)
    for fmt in ("mzML", "mzXML"):
        if fmt not in formats:
            continue
        run = _prepare(files[fmt], tempfile.mkdtemp(dir=out_dir))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        charges = run(ctx)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        row = rows.setdefault(fmt, dict(format=fmt))
        row.update(prepare_s=round(s, 2), prepare_spectra_per_s=round(a.n / s), charges=charges)
        print(fmt, "prepare", row["prepare_s"], "s", flush=True)
    for fmt in ("mzML", "mzXML"):
        if fmt in rows and "MGF" in rows:
            rows[fmt]["mgf_prepare_spectra_per_s"] = rows["MGF"]["prepare_spectra_per_s"]
    for row in rows.values():
        print(json.dumps(dict(tool="peakfile_rate", n=a.n, **row)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
