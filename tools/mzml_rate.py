"""mzML input rate: the device reader (`fal_mzml_index` + `fal_mzml_parse`, `mzml_io.read_chunks_device`) against the host reader
(`mzml_io.read_chunks`, `--mzml_reader host`) on the same file, machine and session.

Writes seeded synthetic MS2 spectra (`synth.generate`, seed 42) as mzML (64-bit m/z, 32-bit intensity, zlib) with an MS1 spectrum
in front of every 5th MS2, then reports
  index_call_ms / parse_call_ms   `fal_mzml_index` / `fal_mzml_parse` over the file's stretches with the text already on the
                   device (device events, median of 5 after one warm-up), and GB/s of text through both
  classify_blocks_staged_share   blocks of 256 tags whose bytes fit the classify pass's LDS tile (the others read global memory)
  host_share       spectra of the file the device hands back to the host reader
  prepare_host_reader_s / prepare_s   `falcon._prepare_spectra` end to end under `--mzml_reader host` / `device` (the second of
                   two device runs: warm page cache, as the host run has it from the file just written)
  prepare_parts_s  the device reader's prepare itemised: scan calls (upload included), identifiers and HOST spectra
                   (chunk_other), decode_peaks, process_spectra + result copies, partitioning, writing the .npz files; the
                   remainder is the file read and the cutting
  outputs_identical   every array of every `spectra_charge_*.npz` of the two readers compared byte for byte
then one JSON line.

    python tools/mzml_rate.py [--n 1000000] [--dir /tmp/peakfiles]
"""
import argparse
import contextlib
import glob
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.peakfile_rate import _Timed, _prepare, _spectra  # noqa: E402


def _stretches(fn, max_bytes):
    """the texts `read_chunks_device` hands to the device, in order"""
    from falcon_amd.ms_io import mzml_io

    texts = []
    with open(fn, "rb") as f:
        data = f.read()
    start = mzml_io._SPECTRUM_OPEN.search(data).start()
    end = data.rfind(mzml_io._CLOSE) + len(mzml_io._CLOSE)
    pos = start
    while pos < end:
        cut = data.rfind(mzml_io._CLOSE, pos, min(pos + max_bytes, end)) + len(mzml_io._CLOSE)
        if cut < len(mzml_io._CLOSE):
            cut = data.find(mzml_io._CLOSE, pos) + len(mzml_io._CLOSE)
        texts.append(np.frombuffer(data[pos:cut], np.uint8))
        pos = cut
    return texts


def _same_outputs(dir_a, dir_b):
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(dir_a, "spectra", "*.npz")))
    if names != sorted(os.path.basename(p) for p in glob.glob(os.path.join(dir_b, "spectra", "*.npz"))) or not names:
        return False
    for name in names:
        a, b = np.load(os.path.join(dir_a, "spectra", name)), np.load(os.path.join(dir_b, "spectra", name))
        if sorted(a.files) != sorted(b.files):
            return False
        for k in a.files:
            x, y = a[k], b[k]
            if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import torch
    from falcon_amd import _lib, falcon
    from falcon_amd.device import Context
    from falcon_amd.ms_io import mgf_io, mzml_io
    from tests import peakfile_writer as W
    out_dir = a.dir or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    fn = os.path.join(out_dir, "run.mzML")
    t0 = time.perf_counter()
    W.write_mzml(fn, _spectra(a.n), mz_bits=64, int_bits=32, zlib_arrays=True, ms1_every=5)
    size = os.path.getsize(fn)
    print(f"wrote {a.n} MS2 spectra in {time.perf_counter() - t0:.1f} s: {size} bytes", flush=True)
    ctx = Context(0)
    ctx.plan(0)
    texts = _stretches(fn, mzml_io.DEVICE_CHUNK_BYTES)
    ctx.scan_mzml(texts[0])                                             # warm-up: code objects, scratch slots
    d_texts = [torch.from_numpy(t.copy()).cuda() for t in texts]
    runs = {"index": [], "parse": []}
    n_spec = n_tags = 0
    for _ in range(5):
        ms = {"index": 0.0, "parse": 0.0}
        n_spec = n_tags = 0
        for d in d_texts:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            ev[0].record()
            k, inside, flags, tags = ctx.mzml_index(d)
            ev[1].record()
            out = ctx.mzml_parse(d, k)
            ev[2].record()
            torch.cuda.synchronize()
            ms["index"] += ev[0].elapsed_time(ev[1])
            ms["parse"] += ev[1].elapsed_time(ev[2])
            n_spec, n_tags = n_spec + k, n_tags + tags
            assert flags == 0
            del out
        for k_ in ms:
            runs[k_].append(ms[k_])
    status = np.concatenate([ctx.scan_mzml(d)["status"] for d in d_texts])
    # the classify pass stages a block of 256 tags into LDS when their byte range fits 32 KB (mzmlscan.hip): the share that does
    staged = blocks = 0
    for t in texts:
        first = np.flatnonzero(t == ord("<"))[::256]
        span = np.diff(np.append(first, len(t))) + (first & 15)
        staged, blocks = staged + int((span <= 32768).sum()), blocks + len(first)
    text_bytes, n_texts = sum(len(t) for t in texts), len(texts)
    del d_texts, texts
    index_ms, parse_ms = float(np.median(runs["index"])), float(np.median(runs["parse"]))
    row = dict(tool="mzml_rate", n=a.n, file_bytes=size, text_bytes=text_bytes, stretches=n_texts, spectra=n_spec, tags=n_tags,
               ok=int((status == _lib.MZML_ST_OK).sum()), skip=int((status == _lib.MZML_ST_SKIP).sum()),
               host=int((status == _lib.MZML_ST_HOST).sum()), host_share=round(float((status == _lib.MZML_ST_HOST).mean()), 6),
               classify_blocks_staged_share=round(staged / max(blocks, 1), 4), index_call_ms=round(index_ms, 2), parse_call_ms=round(parse_ms, 2),
               scan_GBps=round(text_bytes / ((index_ms + parse_ms) * 1e-3) / 1e9, 2))
    print(row, flush=True)
    works = {}
    for reader in ("host", "device", "device"):
        work = works[reader] = tempfile.mkdtemp(dir=out_dir)
        run = _prepare(fn, work, ["--mzml_reader", reader])
        acc = {}
        timers = [_Timed(acc, ctx, "scan_mzml", "scan_calls"), _Timed(acc, mzml_io, "_device_chunk", "chunk"),
                  _Timed(acc, mgf_io, "_identifiers", "identifiers"), _Timed(acc, ctx, "decode_peaks", "decode_peaks"),
                  _Timed(acc, falcon, "_process", "process_spectra"), _Timed(acc, falcon, "_partition", "partition"),
                  _Timed(acc, np, "savez", "write_npz")] if reader == "device" else []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.ExitStack() as stack:
            for t in timers:
                stack.enter_context(t)
            charges = run(ctx)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        if reader == "host":
            row.update(prepare_host_reader_s=round(s, 2), prepare_host_reader_spectra_per_s=round(a.n / s))
        else:
            acc["chunk_other"] = acc.pop("chunk", 0.0) - acc.get("identifiers", 0.0)
            acc["file_read_and_cut"] = s - sum(acc.values())
            row.update(prepare_s=round(s, 2), prepare_spectra_per_s=round(a.n / s), charges=charges,
                       prepare_parts_s={k: round(v, 3) for k, v in sorted(acc.items())})
        print("mzML prepare", reader, round(s, 2), "s", flush=True)
    row["outputs_identical"] = _same_outputs(works["host"], works["device"])
    row["speedup"] = round(row["prepare_host_reader_s"] / row["prepare_s"], 2)
    print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
