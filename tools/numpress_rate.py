"""MS-Numpress decode rate: `fal_decode_peaks` on numpress arrays against the same spectra as plain zlib floats, and the host
decoder.

Encodes seeded synthetic MS2 spectra (`synth.generate`, seed 42) twice into peak payloads (`PeakChunk`, what the mzML reader
hands to the device): m/z as MS-Numpress linear (fixed point 100000) + intensity as slof (fixed point 3000), both followed by
zlib (MS:1002746 / MS:1002748), and the same spectra as zlib 64-bit m/z + zlib 32-bit intensity.  The XML pass in front of the
decode (`tools/peakfile_rate.py`: xml_pass_s) is the same for both and not part of this measurement.  Reports per form:
  base64_bytes     the payload
  decode_call_ms   `fal_decode_peaks` with the payload already on the device (device events, median of 5 after one warm-up; the
                   descriptor tables are uploaded by the call), spectra/s and GB/s of base64 in
  host_decode_s    `PeakChunk.host_spectra` on the first `--sample` spectra, one host thread, and spectra/s
  sample_equal     numpress only: the device's m/z of the sample is bit-equal to the host decoder's, the slof intensity within
                   one float32 ulp
then one JSON line per form.

    python tools/numpress_rate.py [--n 1000000] [--sample 20000]
"""
import argparse
import base64
import json
import os
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MZ_FP, INT_FP = 100000.0, 3000.0
BATCH = 50_000                 # spectra encoded per vectorised pass


def half_byte_streams(x, indptr):
    """int64 values x (each within int32) of the rows of `indptr` -> (bytes of all rows, byte offsets i64[rows + 1]): every
    row a half-byte stream of its own (head nibble, data nibbles least significant first, padded to a whole byte)"""
    u = (x & 0xFFFFFFFF).astype(np.uint64)
    mag = np.where(x >= 0, x, ~x)                                       # its leading zero nibbles are the fill of x
    sig = np.zeros(len(x), np.int64)                                    # significant nibbles of mag
    for k in range(8):
        sig[mag >> (4 * k) != 0] = k + 1
    fill = np.where(x >= 0, 8 - sig, np.minimum(8 - sig, 7))
    head = np.where(x >= 0, fill, np.where(fill > 0, fill + 8, 0))
    size = 9 - fill                                                     # head + data nibbles
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    total = np.bincount(rows, weights=size, minlength=len(indptr) - 1).astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(total + (total & 1))])     # in nibbles
    end = np.cumsum(size)
    first = np.concatenate([[0], end])[indptr[:-1]]                     # nibbles in front of each row's first value
    start = row_off[rows] + (end - size) - first[rows]
    nib = np.zeros(row_off[-1], np.uint8)
    nib[start] = head
    for k in range(8):
        m = k < 8 - fill
        nib[start[m] + 1 + k] = ((u[m] >> np.uint64(4 * k)) & np.uint64(15)).astype(np.uint8)
    return ((nib[0::2] << 4) | nib[1::2]).tobytes(), row_off // 2


def encode_batch(mz, it, indptr):
    """-> per spectrum (linear m/z stream, slof intensity stream)"""
    y = np.rint(mz.astype(np.float64) * MZ_FP).astype(np.int64)
    pos = np.arange(len(y)) - np.repeat(indptr[:-1], np.diff(indptr))
    d = y.copy()
    d[1:] -= 2 * y[:-1]
    d[2:] += y[:-2]
    body = pos >= 2
    counts = np.diff(indptr)
    body_ptr = np.concatenate([[0], np.cumsum(np.maximum(counts - 2, 0))])
    data, off = half_byte_streams(d[body], body_ptr)
    u = np.clip(np.rint(np.log(it.astype(np.float64) + 1.0) * INT_FP), 0, 65535).astype("<u2").tobytes()
    y32 = y.astype("<i4").tobytes()
    mz_head, it_head = struct.pack(">d", MZ_FP), struct.pack(">d", INT_FP)
    out = []
    for s in range(len(counts)):
        a, b = int(indptr[s]), int(indptr[s + 1])
        out.append((mz_head + y32[4 * a:4 * min(a + 2, b)] + data[off[s]:off[s + 1]], it_head + u[2 * a:2 * b]))
    return out


def build_chunks(d, n, numpress):
    from falcon_amd import _lib
    from falcon_amd.ms_io.peak_payload import DEFAULT_CHUNK_BYTES, PeakChunk
    chunks = [PeakChunk()]
    f_mz = (_lib.PEAK_NUMPRESS_LINEAR if numpress else _lib.PEAK_F64) | _lib.PEAK_ZLIB
    f_it = (_lib.PEAK_NUMPRESS_SLOF if numpress else 0) | _lib.PEAK_ZLIB
    for lo in range(0, n, BATCH):
        hi = min(lo + BATCH, n)
        ip = d["indptr"][lo:hi + 1].astype(np.int64)
        mz, it = d["mz"][ip[0]:ip[-1]], d["intensity"][ip[0]:ip[-1]]
        ip = ip - ip[0]
        if numpress:
            streams = encode_batch(mz, it, ip)
        else:
            m, t = mz.astype("<f8").tobytes(), it.astype("<f4").tobytes()
            streams = [(m[8 * a:8 * b], t[4 * a:4 * b]) for a, b in zip(ip[:-1].tolist(), ip[1:].tolist())]
        for s, (sm, si) in enumerate(streams):
            ch = chunks[-1]
            k = int(ip[s + 1] - ip[s])
            ch.add_spectrum(str(lo + s + 1), float(d["precursor_mz"][lo + s]), int(d["precursor_charge"][lo + s]),
                            float(d["retention_time"][lo + s]), ch.add_array(base64.b64encode(zlib.compress(sm, 6)), k, f_mz),
                            ch.add_array(base64.b64encode(zlib.compress(si, 6)), k, f_it))
            if ch.nbytes >= DEFAULT_CHUNK_BYTES:
                chunks.append(PeakChunk())
    return chunks


def _sample(chunk, k):
    """the first k spectra of a chunk as a chunk of their own"""
    from falcon_amd.ms_io.peak_payload import PeakChunk
    out = PeakChunk()
    for i in range(min(k, len(chunk))):
        rows = []
        for r in chunk._spectra[i]:
            off, ln, count, flags = chunk._arrays[r]
            rows.append(out.add_array(bytes(chunk._buf[off:off + ln]), count, flags))
        out.add_spectrum(chunk.identifier[i], chunk.precursor_mz[i], chunk.precursor_charge[i], chunk.retention_time[i], *rows)
    return out


def measure(ctx, chunks, sample, numpress):
    import torch
    from falcon_amd.falcon import _raw_csr
    n_spec = sum(len(c) for c in chunks)
    b64 = sum(c.nbytes for c in chunks)
    tables = [c.tables() for c in chunks]
    args = [(torch.from_numpy(p.copy()).cuda(), a, s) for p, a, s in tables]
    bad = sum(int((ctx.decode_peaks(*t)[3] != 0).sum().item()) for t in args)         # warm-up: code objects, scratch slots
    runs = []
    for _ in range(5):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in args:
            ctx.decode_peaks(*t)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1))
    ms = float(np.median(runs))
    del args
    sm = _sample(chunks[0], sample)
    t0 = time.perf_counter()
    host = list(sm.host_spectra())
    host_s = time.perf_counter() - t0
    row = dict(form="numpress linear + slof, zlib" if numpress else "zlib f64 + f32", spectra=n_spec, status_nonzero=bad,
               base64_bytes=b64, decode_call_ms=round(ms, 2), decode_call_ms_runs=[round(r, 2) for r in runs],
               decode_spectra_per_s=round(n_spec / (ms * 1e-3)), decode_GBps=round(b64 / (ms * 1e-3) / 1e9, 2),
               host_sample=len(host), host_decode_s=round(host_s, 3), host_spectra_per_s=round(len(host) / host_s))
    if numpress:
        hmz, hit, hip = _raw_csr(host)
        ip, mz, it, st = (t.cpu().numpy() for t in ctx.decode_peaks(*sm.tables()))
        ulp = np.abs(it.astype(np.float64) - hit.astype(np.float64)) <= np.spacing(np.maximum(it, hit))
        row["sample_equal"] = bool(not st.any() and np.array_equal(ip, hip) and np.array_equal(mz.view(np.int64), hmz.view(np.int64))
                                   and ulp.all())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--sample", type=int, default=20_000)
    a = ap.parse_args()
    from falcon_amd import synth
    from falcon_amd.device import Context
    t0 = time.perf_counter()
    d = synth.generate(a.n, seed=42)
    print(f"generated {a.n} spectra, {int(d['indptr'][a.n])} peaks in {time.perf_counter() - t0:.1f} s", flush=True)
    ctx = Context(0)
    ctx.plan(0)
    for numpress in (True, False):
        t0 = time.perf_counter()
        chunks = build_chunks(d, a.n, numpress)
        print(f"encoded {'numpress' if numpress else 'plain'} payload in {time.perf_counter() - t0:.1f} s", flush=True)
        row = measure(ctx, chunks, a.sample, numpress)
        del chunks
        print(json.dumps(dict(tool="numpress_rate", n=a.n, **row)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
