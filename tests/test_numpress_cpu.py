"""MS-Numpress without a GPU: the Python decoders (`ms_io/numpress.py`, what `get_spectra` decodes with and the device path's
oracle) and `csrc/numpress.h` under a host build (tests/hostbuild_numpress.py) against the test-side encoders of
tests/numpress_cases.py -- known answers, round trips, damaged streams, guard bytes -- plus the upper-bound form of the
inflater, the mzML reader's flags and `get_spectra` on a numpress file, and the numpress kernel's scratch use."""
import base64
import os
import struct
import zlib

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io import ms_io, mzml_io, numpress
from falcon_amd.ms_io.peak_payload import PeakChunk
from tests import hostbuild_numpress as H
from tests import isa_lint as L
from tests import numpress_cases as N

needs_compiler = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler and no hipcc")
ST_OVERFLOW, ST_SHORT, ST_NUMPRESS = 16, 32, 256


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("hostbuild_numpress"))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _slof_close(got, want):
    """the issue's slof margin: 2^-49 (1 + h) around the value h"""
    got, want = np.asarray(got), np.asarray(want)
    with np.errstate(invalid="ignore"):                                 # inf (a tiny fixed point) must be inf
        return len(got) == len(want) and bool(np.all((got == want) | (np.abs(got - want) <= 2.0 ** -49 * (1.0 + want))))


def _check_known(codec, got, want):
    if codec == N.SLOF:
        assert got[0] == 0.0 and _slof_close(got, np.array(want))
    else:
        assert np.array_equal(_bits(got), _bits(want)), got


def test_flags_and_status_word():
    assert (_lib.PEAK_NUMPRESS_LINEAR, _lib.PEAK_NUMPRESS_PIC, _lib.PEAK_NUMPRESS_SLOF, _lib.PEAK_NUMPRESS_MASK) == (16, 32, 48, 48)
    assert _lib.PEAK_STATUS[256] == "bad MS-Numpress stream"
    header = open(os.path.join(L.ROOT, "include", "falcon_hip.h")).read()
    for name, value in (("NUMPRESS_LINEAR", 16), ("NUMPRESS_PIC", 32), ("NUMPRESS_SLOF", 48), ("NUMPRESS_MASK", 48),
                        ("ST_NUMPRESS", 256)):
        assert f"#define FAL_PEAK_{name} {value} " in " ".join(header.split()) + " ", name


@pytest.mark.parametrize("name", sorted(N.KNOWN))
def test_known_answers_python(name):
    codec, stream, want = N.KNOWN[name]
    got = numpress.decode(codec, stream)
    assert got.dtype == np.float64 and len(got) == len(want)
    _check_known(codec, got, want)


@needs_compiler
@pytest.mark.parametrize("name", sorted(N.KNOWN))
def test_known_answers_host_build(lib, name):
    codec, stream, want = N.KNOWN[name]
    st, got, guard = H.decode(lib, codec, stream, len(want))
    assert st == 0 and guard and len(got) == len(want)
    _check_known(codec, got, want)


def test_encoders_write_the_known_answers_and_reach_every_head_nibble():
    assert N.encode_pic([0, 1, 15, 16, -1, 100000]) == N.KNOWN["pic"][1]
    assert N.encode_pic([0, 1, 15, 16, -1, 100000, 0]) == N.KNOWN["pic + 80"][1]
    assert N.encode_linear_ints([100000, 100500, 101250], 1000.0) == N.KNOWN["linear"][1]
    assert N.encode_slof_ints([0, 1000], 1000.0) == N.KNOWN["slof"][1]
    assert N.int_nibbles(-1) == [15, 15] and N.int_nibbles(0) == [8] and N.int_nibbles(-2 ** 31) == [0] + [0] * 7 + [8]
    heads, parities = set(), set()
    for count in N.COUNTS:
        for ints in N.int_cases(count, 5).values():
            h, p = N.heads_and_parity(ints)
            heads |= h
            parities.add(p)
    assert heads == set(range(16)) and parities == {0, 1}
    heads, parities = set(), set()
    for count in N.COUNTS:
        for _, y in N.mz_cases(count, 6).values():
            h, p = N.heads_and_parity([y[i] - 2 * y[i - 1] + y[i - 2] for i in range(2, len(y))])
            heads |= h
            parities.add(p)
    assert heads == set(range(16)) and parities == {0, 1}


@pytest.mark.parametrize("count", N.COUNTS)
def test_round_trips_python(count):
    for name, ints in N.int_cases(count, 10 + count).items():
        got = numpress.decode(N.PIC, N.encode_pic(ints))
        assert np.array_equal(_bits(got), _bits(ints.astype(np.float64))), name
    for name, (fp, y) in N.mz_cases(count, 20 + count).items():
        stream = N.encode_linear_ints(y, fp)
        fp2, y2 = numpress.linear_integers(stream)
        assert fp2 == fp and np.array_equal(y2, y), name                # the encoder's integers
        assert np.array_equal(_bits(numpress.decode(N.LINEAR, stream)), _bits(y.astype(np.float64) / fp)), name
    rng = np.random.default_rng(30 + count)
    for fp in (1000.0, 3000.5, 100.25):                                # exp(65535 / fp) stays finite
        u = rng.integers(0, 65536, count)
        got = numpress.decode(N.SLOF, N.encode_slof_ints(u, fp))
        assert _slof_close(got, N.slof_values(u, fp)), fp


@needs_compiler
@pytest.mark.parametrize("count", N.COUNTS)
def test_round_trips_host_build_bit_equal_to_python(lib, count):
    for name, ints in N.int_cases(count, 10 + count).items():
        stream = N.encode_pic(ints)
        st, got, guard = H.decode(lib, N.PIC, stream, count)
        assert st == 0 and guard, name
        assert np.array_equal(_bits(got), _bits(ints.astype(np.float64))), name
        assert np.array_equal(_bits(got), _bits(numpress.decode(N.PIC, stream))), name
        assert len(stream) <= lib.t_numpress_max_bytes(N.PIC, count)
    for name, (fp, y) in N.mz_cases(count, 20 + count).items():
        stream = N.encode_linear_ints(y, fp)
        st, got, guard = H.decode(lib, N.LINEAR, stream, count)
        assert st == 0 and guard, name
        assert np.array_equal(_bits(got), _bits(y.astype(np.float64) / fp)), name
        assert np.array_equal(_bits(got), _bits(numpress.decode(N.LINEAR, stream))), name
        assert len(stream) <= lib.t_numpress_max_bytes(N.LINEAR, count)
    rng = np.random.default_rng(30 + count)
    for fp in (1000.0, 3000.5, 100.25):                                # exp(65535 / fp) stays finite
        u = rng.integers(0, 65536, count)
        stream = N.encode_slof_ints(u, fp)
        st, got, guard = H.decode(lib, N.SLOF, stream, count)
        assert st == 0 and guard and _slof_close(got, N.slof_values(u, fp)), fp
        assert len(stream) == lib.t_numpress_max_bytes(N.SLOF, count)


@needs_compiler
def test_inflated_capacity_is_reached_by_nine_nibble_values(lib):
    """the bound of the inflate stage: a value is at most 9 nibbles"""
    for count in (0, 1, 2, 3, 4, 7, 300, 301):
        worst = np.resize(np.array([2 ** 30, -2 ** 30]), count)
        assert len(N.encode_pic(worst)) == lib.t_numpress_max_bytes(N.PIC, count) == (9 * count + 1) // 2
        y = np.resize(np.array([0, 2 ** 29]), count)                           # second differences of +-2^30
        want = 8 if count == 0 else 12 if count == 1 else 16 + (9 * (count - 2) + 1) // 2
        assert len(N.encode_linear_ints(y, 1.0)) == lib.t_numpress_max_bytes(N.LINEAR, count) == want
        assert lib.t_numpress_max_bytes(N.SLOF, count) == 8 + 2 * count


def _python_refuses(codec, stream, count):
    try:
        return len(numpress.decode(codec, stream)) != count
    except ValueError:
        return True


def _damaged_streams():
    """(codec, stream, declared count, must the status be non-zero?)"""
    rng = np.random.default_rng(40)
    out = []
    fp, y = N.mz_cases(7, 41)["shuffled"]
    good = N.encode_linear_ints(y, fp)
    out += [(N.LINEAR, good[:cut], 7, True) for cut in range(len(good))]                 # each prefix of a valid linear stream
    fp, y = N.mz_cases(300, 42)["fine"]
    good300 = N.encode_linear_ints(y, fp)
    out += [(N.LINEAR, good300[:cut], 300, True) for cut in range(0, len(good300), 7)]
    ints = N.int_cases(7, 43)["mixed"]
    pic = N.encode_pic(ints)
    out += [(N.PIC, pic[:cut], 7, True) for cut in range(len(pic))]
    slof = N.encode_slof_ints(rng.integers(0, 65536, 7), 1000.0)
    out += [(N.SLOF, slof[:cut], 7, True) for cut in range(len(slof))]                   # odd bodies and short headers among them
    out.append((N.SLOF, slof + b"\x01", 7, True))
    for bad in (0.0, -0.0, float("nan"), float("inf"), -float("inf"), -1000.0):
        out.append((N.LINEAR, struct.pack(">d", bad) + good[8:], 7, True))
        out.append((N.LINEAR, struct.pack(">d", bad), 0, True))
        out.append((N.SLOF, struct.pack(">d", bad) + slof[8:], 7, True))
    for codec, stream, count in ((N.LINEAR, good, 7), (N.LINEAR, good300, 300), (N.PIC, pic, 7), (N.SLOF, slof, 7),
                                 (N.LINEAR, good[:12], 1), (N.LINEAR, good[:16], 2), (N.LINEAR, good[:8], 0), (N.PIC, b"", 0)):
        out.append((codec, stream, count + 1, True))                                     # a declared count off by one
        if count:
            out.append((codec, stream, count - 1, True))
        out.append((codec, stream, count, False))                                        # and the stream as it is
    for k in range(300):                                                                 # random bytes: whatever they decode to
        codec = (N.LINEAR, N.PIC, N.SLOF)[k % 3]
        body = rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        out.append((codec, (struct.pack(">d", 10.0) if k % 2 else b"") + body, int(rng.integers(0, 12)), None))
    return out


def test_damaged_streams_python():
    for codec, stream, count, must_fail in _damaged_streams():
        if must_fail is not None:
            assert _python_refuses(codec, stream, count) == must_fail, (codec, len(stream), count)


@needs_compiler
def test_damaged_streams_host_build(lib):
    seen = set()
    for codec, stream, count, must_fail in _damaged_streams():
        st, got, guard = H.decode(lib, codec, stream, count)
        assert guard, (codec, len(stream), count)
        refused = _python_refuses(codec, stream, count)
        if refused or must_fail:
            assert st != 0, (codec, len(stream), count)                 # what the Python decoder refuses is refused
        else:
            assert st == 0, (codec, len(stream), count)
            want = numpress.decode(codec, stream)
            assert _slof_close(got, want) if codec == N.SLOF else np.array_equal(_bits(got), _bits(want))
        assert st & ~(ST_OVERFLOW | ST_SHORT | ST_NUMPRESS) == 0
        seen.add(st)
    assert {0, ST_OVERFLOW, ST_SHORT, ST_NUMPRESS} <= seen


@needs_compiler
def test_inflate_accepts_a_shorter_output_in_its_upper_bound_form(lib):
    data = N.encode_linear_ints(N.mz_cases(300, 50)["shuffled"][1], 1000.0)
    stream = zlib.compress(data, 6)
    for cap in (len(data), len(data) + 1, len(data) + 500):
        st, n, out, guard = H.inflate_upto(lib, stream, cap, exact=False)
        assert st == 0 and n == len(data) and out[:n] == data and guard, cap
    st, n, out, guard = H.inflate_upto(lib, stream, len(data) + 1, exact=True)          # the declared-size form is as it was
    assert st == ST_SHORT and guard
    st, n, out, guard = H.inflate_upto(lib, stream, len(data), exact=True)
    assert st == 0 and n == len(data) and out == data and guard
    for exact in (False, True):
        st, n, out, guard = H.inflate_upto(lib, stream, len(data) - 1, exact=exact)
        assert st == ST_OVERFLOW and guard
        st, n, out, guard = H.inflate_upto(lib, stream[:-1], len(data), exact=exact)     # the trailer is still checked
        assert st != 0 and guard
    st, n, out, guard = H.inflate_upto(lib, zlib.compress(b""), 64, exact=False)
    assert st == 0 and n == 0 and guard


def _chunk_row(stream, count, flags, compress=False):
    ch = PeakChunk()
    return ch, ch.add_array(base64.b64encode(zlib.compress(stream) if compress else stream), count, flags)


def test_host_values_decodes_numpress_arrays_and_raises_on_every_error():
    for name, (codec, stream, want) in N.KNOWN.items():
        for compress in (False, True):
            ch, row = _chunk_row(stream, len(want), codec | (_lib.PEAK_ZLIB if compress else 0), compress)
            got = ch.host_values(row)
            assert got.dtype == np.float64
            _check_known(codec, got, want)
            for count in (len(want) - 1, len(want) + 1):
                ch, row = _chunk_row(stream, count, codec | (_lib.PEAK_ZLIB if compress else 0), compress)
                with pytest.raises(ValueError):
                    ch.host_values(row)
    codec, stream, want = N.KNOWN["linear"]
    for bad, flags in ((stream[:-1], codec), (stream[:10], codec), (struct.pack(">d", 0.0) + stream[8:], codec),
                       (stream, codec | _lib.PEAK_ZLIB), (stream, codec | _lib.PEAK_F64), (stream, codec | _lib.PEAK_PAIRS),
                       (stream, codec | _lib.PEAK_BIG_ENDIAN), (N.KNOWN["slof"][1] + b"\0", N.SLOF)):
        ch, row = _chunk_row(bad, 3, flags)
        with pytest.raises(ValueError):
            ch.host_values(row)


PLANS = N.PLANS


def test_reader_sets_the_flags_of_the_plain_and_the_combined_terms(tmp_path):
    spectra, _ = N.encoded_spectra(len(PLANS), 60, PLANS)
    fn = str(tmp_path / "flags.mzML")
    N.write_mzml(fn, spectra)
    (chunk,) = list(mzml_io.read_chunks(fn))
    assert not chunk.skipped and len(chunk) == len(PLANS)
    _, arrays, spec = chunk.tables()
    for i, (mc, mzl, ic, izl) in enumerate(PLANS):
        assert arrays[spec[i, 0], 3] == mc | (_lib.PEAK_ZLIB if mzl else 0), i      # the 64-bit float term is ignored
        assert arrays[spec[i, 1], 3] == ic | (_lib.PEAK_ZLIB if izl else 0), i
        assert arrays[spec[i, 0], 2] == arrays[spec[i, 1], 2] == spectra[i]["mz"][3]


def test_contradictory_and_truncation_terms_stay_skipped(tmp_path):
    spectra, _ = N.encoded_spectra(8, 61, PLANS[:1] + PLANS[4:5])       # linear m/z: plain on even, zlib-combined on odd spectra
    ids = [s["identifier"] for s in spectra]
    extra = {ids[0]: N.W._cv("MS:1000574", "zlib compression"), ids[1]: N.W._cv("MS:1000576", "no compression"),
             ids[2]: N.W._cv("MS:1002313", "MS-Numpress positive integer compression"),
             ids[3]: N.W._cv("MS:1003089", "truncation, delta prediction and zlib compression")}
    fn = str(tmp_path / "contra.mzML")
    N.write_mzml(fn, spectra, extra)
    (chunk,) = list(mzml_io.read_chunks(fn))
    assert chunk.skipped == {"MS-Numpress linear": 4}
    assert chunk.identifier == ids[4:]
    txt = open(fn).read().replace('accession="MS:1002312"', 'accession="MS:1003090"', 1).replace('accession="MS:1000574"', 'accession="MS:0"')
    open(fn, "w").write(txt)
    (chunk,) = list(mzml_io.read_chunks(fn))
    assert chunk.skipped == {"unsupported compression": 1, "MS-Numpress linear": 3}


def test_get_spectra_returns_the_decoded_values(tmp_path):
    spectra, want = N.encoded_spectra(60, 62, PLANS)
    fn = str(tmp_path / "np.mzML")
    N.write_mzml(fn, spectra)
    got = list(ms_io.get_spectra(fn))
    assert [g["identifier"] for g in got] == [s["identifier"] for s in spectra]
    for g, s, (m_val, i_val), plan in zip(got, spectra, want, PLANS * 10):
        assert g["precursor_mz"] == s["precursor_mz"] and g["precursor_charge"] == s["precursor_charge"]
        assert g["mz"].dtype == np.float64 and g["intensity"].dtype == np.float32
        assert np.array_equal(_bits(g["mz"]), _bits(m_val)), s["identifier"]
        if plan[2] == N.SLOF:
            assert np.all(np.abs(g["intensity"].astype(np.float64) - i_val) <= np.spacing(i_val)), s["identifier"]
        else:
            assert np.array_equal(g["intensity"], i_val), s["identifier"]


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_numpress_kernel_uses_no_scratch(tmp_path):
    meta = L.kernel_meta(L.compile_to_asm("peakdecode.hip", tmp_path), "private_segment_fixed_size")
    mine = {k: v for k, v in meta.items() if "numpress_decode_kernel" in k}
    assert len(mine) == 1 and not any(mine.values()), mine
