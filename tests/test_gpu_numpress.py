"""MS-Numpress arrays through `Context.decode_peaks` (`fal_decode_peaks`) against the host decoder (`PeakChunk.host_spectra`,
`ms_io/numpress.py`) plus `falcon._raw_csr`: linear and pic bit for bit, slof within the margin of two `exp`s; damaged streams
give a status and leave their neighbours intact; a codec with a float-width flag is a bad descriptor; and the CLI clusters a
numpress mzML exactly as the same values stored as plain floats."""
import base64
import struct
import zlib

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io.peak_payload import PeakChunk
from tests import numpress_cases as N
from tests import peakfile_writer as W

pytestmark = pytest.mark.gpu

MZ_KINDS = ("linear", "pic", "f64", "f32")
INT_KINDS = ("pic", "slof", "linear", "f32", "f64")


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _stream(values, kind, fp):
    """values in one of the array forms -> (bytes before zlib / base64, flags without PEAK_ZLIB)"""
    if kind == "linear":
        return N.encode_linear_ints(N.linear_ints(values, fp), fp), N.LINEAR
    if kind == "pic":
        return N.encode_pic(np.rint(values).astype(np.int64)), N.PIC
    if kind == "slof":
        return N.encode_slof_ints(N.slof_ints(values, fp), fp), N.SLOF
    return np.ascontiguousarray(values, "<f8" if kind == "f64" else "<f4").tobytes(), _lib.PEAK_F64 if kind == "f64" else 0


def _add(ch, stream, count, flags, compress):
    return ch.add_array(base64.b64encode(zlib.compress(stream, 6) if compress else stream), count, flags | (_lib.PEAK_ZLIB if compress else 0))


def _spectra(rng, n, max_peaks=300, unsorted_frac=0.2):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, max_peaks + 1))
        mz = np.sort(rng.uniform(100.0, 2000.0, k))
        if k > 3 and rng.random() < unsorted_frac:
            mz[: k // 3] = mz[0]                                        # ties, then shuffled
            mz = rng.permutation(mz)
        out.append((mz, rng.uniform(0.0, 1e5, k)))
    return out


def _host_csr(ch):
    from falcon_amd.falcon import _raw_csr
    got = list(ch.host_spectra())
    assert len(got) == len(ch) and not ch.skipped, ch.skipped
    return _raw_csr(got)


def _device(ctx, tables):
    return tuple(t.cpu().numpy() for t in ctx.decode_peaks(*tables))


def _ulp32_apart(a, b):
    """float32 arrays at most one ulp apart"""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.fixture(scope="module")
def mixed(ctx):
    """(a)'s chunk, decoded once on the host and once on the device"""
    rng = np.random.default_rng(71)
    spectra = _spectra(rng, 2000) + [(np.zeros(0), np.zeros(0))] * 3
    big = np.sort(rng.uniform(100.0, 2000.0, 12000))                   # streams of more than 64 KB
    spectra.insert(1234, (rng.permutation(big), rng.uniform(0.0, 1e5, 12000)))
    ch, kinds = PeakChunk(), []
    for i, (mz, it) in enumerate(spectra):
        mk, ik = MZ_KINDS[int(rng.integers(len(MZ_KINDS)))], INT_KINDS[int(rng.integers(len(INT_KINDS)))]
        if i == 1234:
            mk, ik = "linear", "pic"
        s0, f0 = _stream(mz, mk, 10000.0)
        s1, f1 = _stream(it, ik, 3000.0 if ik == "slof" else 100.0)
        ch.add_spectrum(str(i), 500.0, 2, 1.0, _add(ch, s0, len(mz), f0, bool(rng.integers(2))), _add(ch, s1, len(it), f1, bool(rng.integers(2))))
        kinds.append((mk, ik))
    return ch, kinds, _host_csr(ch), _device(ctx, ch.tables())


def test_mixed_chunk_matches_the_host_decoder(mixed):
    ch, kinds, (hmz, hit, hip), (ip, mz, it, st) = mixed
    flags = ch.tables()[1][:, 3]
    seen = {(int(f) & _lib.PEAK_NUMPRESS_MASK, bool(f & _lib.PEAK_ZLIB)) for f in flags}
    assert seen == {(c, z) for c in (0, N.LINEAR, N.PIC, N.SLOF) for z in (False, True)}
    assert not st.any(), (np.flatnonzero(st)[:10], st[st != 0][:10])
    assert np.array_equal(ip, hip) and ip[-1] > 12000
    assert np.array_equal(mz.view(np.int64), hmz.view(np.int64))       # m/z is linear, pic or plain everywhere
    slof = np.repeat(np.array([ik == "slof" for _, ik in kinds]), np.diff(ip))
    assert 0.1 < slof.mean() < 0.3
    assert np.array_equal(it[~slof].view(np.int32), hit[~slof].view(np.int32))
    assert np.all(_ulp32_apart(it[slof], hit[slof]))
    print("slof intensity of the mixed chunk: %d of %d float32 values differ from the host's (by one ulp)"
          % (int((it[slof] != hit[slof]).sum()), int(slof.sum())))


@pytest.mark.filterwarnings("ignore:overflow encountered in cast")     # exp(65535 / 93) - 1 as float32, on the host side
def test_slof_against_the_host_decoder(ctx):
    """(b): slof in the intensity slot within 1 float32 ulp, in the m/z slot within 2^-49 (1 + h) of the host value h: up to
    3 ulp of the device exp, 1 of the host's, and the two roundings of the subtraction"""
    rng = np.random.default_rng(72)
    ch = PeakChunk()
    for i, (mz, it) in enumerate(_spectra(rng, 300)):
        fp_mz, fp_it = float(rng.choice([5000.0, 8000.5, 1234.0])), float(rng.choice([3000.0, 5000.0, 700.25]))
        s0, f0 = _stream(mz, "slof", fp_mz)
        s1, f1 = _stream(it, "slof", fp_it)
        ch.add_spectrum(str(i), 500.0, 2, 1.0, _add(ch, s0, len(mz), f0, bool(i & 1)), _add(ch, s1, len(it), f1, bool(i & 2)))
    every = np.arange(65536)                                            # every 16-bit logarithm once, at two fixed points
    for fp in (6000.0, 93.0):
        s = N.encode_slof_ints(every, fp)
        ch.add_spectrum(f"all {fp}", 500.0, 2, 1.0, _add(ch, s, 65536, N.SLOF, True), _add(ch, s, 65536, N.SLOF, False))
    hmz, hit, hip = _host_csr(ch)
    ip, mz, it, st = _device(ctx, ch.tables())
    assert not st.any() and np.array_equal(ip, hip)
    assert np.isfinite(hmz).all() and np.isfinite(mz).all()
    err = np.abs(mz - hmz) / (1.0 + hmz)
    fin = np.isfinite(hit)                                              # exp(65535 / 93) - 1 is inf as a float32, on both sides
    print("slof m/z: largest |device - host| / (1 + host) = %.3f x 2^-52 over %d values (%d differ); "
          "slof intensity: %d of %d float32 values differ" % (err.max() * 2.0 ** 52, len(mz), int((mz != hmz).sum()),
                                                              int((it != hit).sum()), len(it)))
    assert err.max() <= 2.0 ** -49
    assert np.array_equal(np.isfinite(it), fin) and np.all(_ulp32_apart(it[fin], hit[fin]))
    assert np.array_equal(it[~fin].view(np.int32), hit[~fin].view(np.int32))


def test_damaged_arrays_set_status_and_spare_neighbours(ctx):
    """(c): every fourth spectrum carries a truncated stream, a count off by one or a bad fixed point"""
    rng = np.random.default_rng(73)
    clean, bad, kinds = PeakChunk(), PeakChunk(), []
    damage = ("truncated", "count", "fp")
    for i, (mz, it) in enumerate(_spectra(rng, 400, unsorted_frac=0.1)):
        mk, ik = ("linear", "pic")[int(rng.integers(2))], INT_KINDS[int(rng.integers(3))]
        kind = damage[(i // 4) % 3] if i % 4 == 1 and len(mz) > 8 else "ok"
        if kind == "fp" and mk != "linear" and ik == "pic":
            mk = "linear"                                               # pic has no fixed point
        s0, f0 = _stream(mz, mk, 10000.0)
        s1, f1 = _stream(it, ik, 3000.0 if ik == "slof" else 100.0)
        z0, z1 = bool(rng.integers(2)), bool(rng.integers(2))
        clean.add_spectrum(str(i), 500.0, 2, 1.0, _add(clean, s0, len(mz), f0, z0), _add(clean, s1, len(it), f1, z1))
        c0 = c1 = len(mz)
        if kind == "truncated":                                         # the numpress stream, or the zlib stream around it
            which = int(rng.integers(3))
            if which == 0:
                s0 = s0[: int(rng.integers(1, len(s0)))]
            elif which == 1:
                s1 = s1[: int(rng.integers(1, len(s1)))]
            else:
                s0, f0, z0 = zlib.compress(s0, 6)[:-5], f0 | _lib.PEAK_ZLIB, False
        elif kind == "count":
            c0 = c1 = len(mz) + int(rng.choice([-1, 1]))
        elif kind == "fp":
            wrong = struct.pack(">d", float(rng.choice([0.0, -1000.0, np.nan, np.inf])))
            if mk == "linear" and (ik == "pic" or rng.integers(2)):
                s0 = wrong + s0[8:]
            else:
                s1 = wrong + s1[8:]
        bad.add_spectrum(str(i), 500.0, 2, 1.0, _add(bad, s0, c0, f0, z0), _add(bad, s1, c1, f1, z1))
        kinds.append(kind)
    assert {k: kinds.count(k) > 20 for k in damage} == {k: True for k in damage}
    ip, mz, it, st = _device(ctx, clean.tables())
    assert not st.any()
    ip2, mz2, it2, st2 = _device(ctx, bad.tables())
    want = {"truncated": 16 | 32 | 256 | 8 | 64, "count": 16 | 32, "fp": 256}
    for i, kind in enumerate(kinds):
        seg, seg2 = slice(ip[i], ip[i + 1]), slice(ip2[i], ip2[i + 1])
        if kind == "ok":
            assert st2[i] == 0, (i, st2[i])
            assert np.array_equal(mz2[seg2].view(np.int64), mz[seg].view(np.int64)), i
            assert np.array_equal(it2[seg2].view(np.int32), it[seg].view(np.int32)), i
        else:
            assert st2[i] != 0 and st2[i] & ~want[kind] == 0, (i, kind, st2[i])
            assert not mz2[seg2].any() and not it2[seg2].any(), (i, kind)
    assert {int(s) for s in st2} >= {0, 16, 32, 256}


def test_codec_with_a_float_width_byte_order_or_pair_flag_is_a_bad_descriptor(ctx, mixed):
    """(d), on the first spectra of (a)'s chunk"""
    ch, kinds, _, (ip, mz, it, st) = mixed
    payload, arrays, spec = ch.tables()
    arrays = arrays.copy()
    rows = [i for i, (mk, _) in enumerate(kinds) if mk in ("linear", "pic")][:4]
    for i, flag in zip(rows, (_lib.PEAK_F64, _lib.PEAK_BIG_ENDIAN, _lib.PEAK_PAIRS, 64)):
        arrays[spec[i, 0], 3] |= flag
    ip2, mz2, it2, st2 = _device(ctx, (payload, arrays, spec))
    assert np.all(st2[rows] == 1), st2[rows]                            # FAL_PEAK_ST_DESC
    keep = np.ones(len(kinds), bool)
    keep[rows] = False
    assert np.array_equal(ip2, ip) and not st2[keep].any()
    peaks = np.repeat(keep, np.diff(ip))
    assert np.array_equal(mz2[peaks].view(np.int64), mz[peaks].view(np.int64)) and not mz2[~peaks].any()
    assert np.array_equal(it2[peaks].view(np.int32), it[peaks].view(np.int32)) and not it2[~peaks].any()


def _rows(csv):
    lines = open(csv).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    return [l for l in head if not l.startswith("# work_dir")], [l.split(",", 1)[1] for l in lines[len(head) + 1:]]


def test_cli_clusters_a_numpress_mzml_like_the_same_values_as_plain_floats(tmp_path):
    """(e): linear m/z + pic intensity, the zlib-combined terms on every other spectrum"""
    from falcon_amd import synth
    from falcon_amd.falcon import main
    from falcon_amd.ms_io import ms_io
    d = synth.generate(300, seed=33)
    spectra = []
    for i in range(300):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        y = N.linear_ints(d["mz"][a:b], 100000.0)
        v = np.rint(d["intensity"][a:b].astype(np.float64) * 1000.0).astype(np.int64)
        spectra.append({"identifier": str(i + 1), "precursor_mz": float(d["precursor_mz"][i]),
                        "precursor_charge": int(d["precursor_charge"][i]), "retention_time": float(d["retention_time"][i]),
                        "mz": (N.LINEAR, N.encode_linear_ints(y, 100000.0), bool(i & 1), b - a),
                        "intensity": (N.PIC, N.encode_pic(v), bool(i & 1), b - a)})
    N.write_mzml(str(tmp_path / "np.mzML"), spectra)
    decoded = list(ms_io.get_spectra(str(tmp_path / "np.mzML")))
    assert len(decoded) == 300 and sum(len(s["mz"]) for s in decoded) == d["indptr"][300]
    W.write_mzml(str(tmp_path / "plain.mzML"), decoded, mz_bits=64, int_bits=32, zlib_arrays=True)
    rows = {}
    for name in ("np", "plain"):
        out = str(tmp_path / ("out_" + name))
        assert main([str(tmp_path / (name + ".mzML")), out, "--work_dir", str(tmp_path / ("work_" + name))]) == 0
        rows[name] = _rows(out + ".csv")
    assert rows["np"] == rows["plain"] and len(rows["np"][1]) > 200     # a row per spectrum that passes preprocessing
