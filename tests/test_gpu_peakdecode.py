"""`Context.decode_peaks` (`fal_decode_peaks`) against the host decode (stdlib base64 + zlib) plus `falcon._raw_csr`, bit for bit;
corrupted streams give a status and leave their neighbours intact; and the CLI reads mzML / mzXML into the same clusters as
MGF."""
import base64
import os
import zlib

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io.peak_payload import PeakChunk
from tests import peakfile_writer as W

pytestmark = pytest.mark.gpu

STRATEGIES = [(0, None), (1, None), (6, None), (9, None), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)]


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _encode(values, dtype, compress, level=6, strategy=None):
    raw = np.ascontiguousarray(values, dtype=dtype).tobytes()
    if compress:
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY if strategy is None else strategy)
        raw = c.compress(raw) + c.flush()
    return base64.b64encode(raw)


def _chunk(spectra, rng, pairs_every=0):
    """spectra -> PeakChunk with per-array random precision / compression / strategy (mzML form; every `pairs_every`-th spectrum
    as one interleaved big-endian mzXML array)"""
    ch = PeakChunk()
    for i, (mz, it) in enumerate(spectra):
        level, strat = STRATEGIES[int(rng.integers(len(STRATEGIES)))]
        comp = bool(rng.integers(4))
        if pairs_every and i % pairs_every == 0:
            bits = int(rng.choice([32, 64]))
            v = np.empty(2 * len(mz))
            v[0::2], v[1::2] = mz, it
            f = _lib.PEAK_PAIRS | _lib.PEAK_BIG_ENDIAN | (_lib.PEAK_F64 if bits == 64 else 0) | (_lib.PEAK_ZLIB if comp else 0)
            row = ch.add_array(_encode(v, ">f8" if bits == 64 else ">f4", comp, level, strat), len(mz), f)
            ch.add_spectrum(str(i), 500.0, 2, 1.0, row, row)
            continue
        rows = []
        for vals in (mz, it):
            bits = int(rng.choice([32, 64]))
            f = (_lib.PEAK_F64 if bits == 64 else 0) | (_lib.PEAK_ZLIB if comp else 0)
            rows.append(ch.add_array(_encode(vals, "<f8" if bits == 64 else "<f4", comp, level, strat), len(vals), f))
        ch.add_spectrum(str(i), 500.0, 2, 1.0, *rows)
    return ch


def _host_csr(ch):
    from falcon_amd.falcon import _raw_csr
    return _raw_csr(list(ch.host_spectra()))


def _device(ctx, ch):
    ip, mz, it, st = ctx.decode_peaks(*ch.tables())
    return ip.cpu().numpy(), mz.cpu().numpy(), it.cpu().numpy(), st.cpu().numpy()


def _random_spectra(rng, n, max_peaks=200, unsorted_frac=0.2):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, max_peaks + 1))
        mz = np.sort(rng.uniform(100.0, 2000.0, k))
        if k > 3 and rng.random() < unsorted_frac:
            mz[: k // 3] = mz[0]                                        # ties, then shuffled
            mz = rng.permutation(mz)
        out.append((mz, rng.uniform(0.0, 1e5, k).astype(np.float32)))
    return out


def test_decode_matches_host_randomized(ctx):
    rng = np.random.default_rng(1)
    spectra = _random_spectra(rng, 3000) + [(np.zeros(0), np.zeros(0, np.float32))] * 5
    big = np.sort(rng.uniform(100.0, 2000.0, 12000))                   # > 64 KB arrays, sorted and not
    spectra += [(big, rng.uniform(0, 1, 12000).astype(np.float32)), (rng.permutation(big), rng.uniform(0, 1, 12000).astype(np.float32))]
    ch = _chunk(spectra, rng, pairs_every=5)
    ip, mz, it, st = _device(ctx, ch)
    hmz, hit, hip = _host_csr(ch)
    assert not st.any(), np.flatnonzero(st)
    assert np.array_equal(ip, hip)
    assert np.array_equal(mz.view(np.int64), hmz.view(np.int64))
    assert np.array_equal(it.view(np.int32), hit.view(np.int32))


@pytest.mark.parametrize("level,strategy", STRATEGIES)
def test_every_deflate_form(ctx, level, strategy):
    rng = np.random.default_rng(100 + level + (strategy or 0))
    ch = PeakChunk()
    want = []
    for i in range(200):
        k = int(rng.integers(0, 3000))
        mz = np.sort(np.round(rng.uniform(100.0, 2000.0, k), 2))      # rounded: repeats for the LZ77 matches
        it = np.round(rng.uniform(0, 50, k)).astype(np.float32)
        r0 = ch.add_array(_encode(mz, "<f8", True, level, strategy), k, _lib.PEAK_F64 | _lib.PEAK_ZLIB)
        r1 = ch.add_array(_encode(it, "<f4", True, level, strategy), k, _lib.PEAK_ZLIB)
        ch.add_spectrum(str(i), 1.0, 1, 1.0, r0, r1)
        want.append((mz, it))
    ip, mz, it, st = _device(ctx, ch)
    assert not st.any()
    assert np.array_equal(mz, np.concatenate([w[0] for w in want])) and np.array_equal(it, np.concatenate([w[1] for w in want]))


def test_hundred_thousand_arrays(ctx):
    rng = np.random.default_rng(2)
    ch = _chunk(_random_spectra(rng, 50000, max_peaks=30, unsorted_frac=0.05), rng)
    assert len(ch.tables()[1]) == 100000
    ip, mz, it, st = _device(ctx, ch)
    hmz, hit, hip = _host_csr(ch)
    assert not st.any()
    assert np.array_equal(ip, hip) and np.array_equal(mz.view(np.int64), hmz.view(np.int64))
    assert np.array_equal(it.view(np.int32), hit.view(np.int32))


def test_corrupted_streams_set_status_and_spare_neighbours(ctx):
    rng = np.random.default_rng(3)
    good = _random_spectra(rng, 400, max_peaks=300, unsorted_frac=0.1)
    ch = PeakChunk()
    kinds = {}
    for i, (mz, it) in enumerate(good):
        kind = ["ok", "flip", "trunc", "adler", "count", "b64", "ok", "ok"][i % 8] if len(mz) > 8 else "ok"
        raw = zlib.compress(mz.astype("<f8").tobytes(), 6)
        count = len(mz)
        if kind == "flip":
            b = bytearray(raw)
            b[int(rng.integers(2, len(b) - 4))] ^= 1 << int(rng.integers(8))
            raw = bytes(b)
        elif kind == "trunc":
            raw = raw[: len(raw) // 2]
        elif kind == "adler":
            raw = raw[:-1] + bytes([raw[-1] ^ 0x40])
        elif kind == "count":
            count += int(rng.choice([-1, 1]))
        txt = base64.b64encode(raw)
        if kind == "b64":
            txt = txt[:3] + b"!" + txt[4:]
        r0 = ch.add_array(txt, count, _lib.PEAK_F64 | _lib.PEAK_ZLIB)
        r1 = ch.add_array(_encode(it, "<f4", True), len(it), _lib.PEAK_ZLIB)
        ch.add_spectrum(str(i), 1.0, 1, 1.0, r0, r1)
        kinds[i] = kind
    ip, mz, it, st = _device(ctx, ch)
    for i, (m, t) in enumerate(good):
        seg = slice(ip[i], ip[i + 1])
        if kinds[i] in ("trunc", "adler", "count", "b64"):
            assert st[i] != 0, (i, kinds[i])
        if st[i] == 0:                                                  # a flip may land in padding bits: then the data is intact
            order = np.lexsort((m, np.zeros(len(m), int)))
            assert np.array_equal(mz[seg], m[order]) and np.array_equal(it[seg], t[order]), (i, kinds[i])
        else:
            assert kinds[i] != "ok" and not mz[seg].any()
    assert (st[[i for i in kinds if kinds[i] == "flip"]] != 0).mean() > 0.5
    # bad descriptors: outside the payload, misaligned, unknown flags, array index out of range -> status, no fault
    payload, arrays, spec = ch.tables()
    arrays = arrays.copy()
    spec = spec.copy()
    arrays[spec[0, 0], 0] = len(payload) + 8
    arrays[spec[1, 0], 0] += 4
    arrays[spec[2, 0], 3] |= 64
    spec[3, 1] = len(arrays) + 5
    ip2, mz2, it2, st2 = (t.cpu().numpy() for t in ctx.decode_peaks(payload, arrays, spec))
    assert np.all(st2[:4] & 1), st2[:4]                                 # FAL_PEAK_ST_DESC
    assert np.array_equal(ip2, ip) and np.array_equal(st2[4:], st[4:])
    assert np.array_equal(mz2[ip[4]:], mz[ip[4]:]) and np.array_equal(it2[ip[4]:], it[ip[4]:])


def _cli(args):
    from falcon_amd.falcon import main
    assert main(args) == 0


def _rows(csv):
    lines = open(csv).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    return [l for l in head if not l.startswith("# work_dir")], [l.split(",", 1)[1] for l in lines[len(head) + 1:]]


@pytest.mark.parametrize("extra", [[], ["--exact"]])
def test_cli_mzml_mzxml_match_mgf(tmp_path, extra):
    from falcon_amd import synth
    from falcon_amd.ms_io import ms_io
    d = synth.generate(3000, seed=31)
    spectra = []
    for i in range(3000):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        spectra.append({"identifier": str(i + 1), "precursor_mz": float(d["precursor_mz"][i]),
                        "precursor_charge": int(d["precursor_charge"][i]), "retention_time": float(d["retention_time"][i]),
                        "mz": d["mz"][a:b].astype(np.float64), "intensity": d["intensity"][a:b]})
    W.write_mzml(str(tmp_path / "in.mzML"), spectra, mz_bits=64, zlib_arrays=True, ms1_every=10, param_groups=True)
    W.write_mzml(str(tmp_path / "in32.mzML"), spectra, mz_bits=32, zlib_arrays=True, ms1_every=10)
    W.write_mzxml(str(tmp_path / "in.mzXML"), spectra, bits=64, zlib_arrays=True, ms1_every=10)
    common = ["--export_representatives", "--work_dir"]
    outs = {}
    for name in ("in.mzML", "in32.mzML", "in.mzXML"):
        # the same spectra as MGF: as the host reader returns them (mzXML: RT in minutes; 32-bit m/z widened)
        mgf = str(tmp_path / (name + ".mgf"))
        ms_io.write_spectra(mgf, list(ms_io.get_spectra(str(tmp_path / name))))
        for src in (name, name + ".mgf"):
            out = str(tmp_path / ("out_" + src))
            _cli([str(tmp_path / src), out, *common, str(tmp_path / ("work_" + src)), *extra])
            outs[src] = out
        h1, r1 = _rows(outs[name] + ".csv")
        h2, r2 = _rows(outs[name + ".mgf"] + ".csv")
        assert h1 == h2 and r1 == r2 and len(r1) > 2500, name
        assert open(outs[name] + ".mgf").read() == open(outs[name + ".mgf"] + ".mgf").read()
        for f in ("spectra_charge_2.npz", "spectra_charge_3.npz"):
            a = np.load(os.path.join(str(tmp_path / ("work_" + name)), "spectra", f))
            b = np.load(os.path.join(str(tmp_path / ("work_" + name + ".mgf")), "spectra", f))
            for k in a.files:
                if k != "filename":
                    assert np.array_equal(a[k], b[k]), (name, f, k)
