"""mzML / mzXML readers (falcon_amd.ms_io) on generated files: fields and arrays bit for bit, MS1 skipped, nested mzXML scans,
referenceable param groups, truncated files, unsupported arrays counted; and the device decoder's kernels build without scratch."""
import logging
import os

import numpy as np
import pytest

from falcon_amd.ms_io import ms_io, mzml_io, mzxml_io
from tests import isa_lint as L
from tests import peakfile_writer as W


def _check(got, spectra, mz_bits=64, rt_div=1.0):
    assert [g["identifier"] for g in got] == [s["identifier"] for s in spectra]
    for g, s in zip(got, spectra):
        assert g["precursor_mz"] == s["precursor_mz"]
        assert g["precursor_charge"] == s["precursor_charge"]
        assert g["retention_time"] == s["retention_time"] / rt_div
        want = s["mz"] if mz_bits == 64 else s["mz"].astype(np.float32).astype(np.float64)
        assert g["mz"].dtype == np.float64 and g["intensity"].dtype == np.float32
        assert np.array_equal(g["mz"], want) and np.array_equal(g["intensity"], s["intensity"])


@pytest.mark.parametrize("kw", [
    dict(),
    dict(indexed=True),
    dict(mz_bits=32, int_bits=32, zlib_arrays=False),
    dict(mz_bits=64, int_bits=64, zlib_arrays=True, param_groups=True),
    dict(mz_bits=32, zlib_arrays=True, indexed=True, param_groups=True),
])
def test_mzml_variants_round_trip(tmp_path, kw):
    spectra = W.synthetic_spectra(150, seed=11, unsorted_every=9)
    fn = str(tmp_path / "run.mzML")
    W.write_mzml(fn, spectra, ms1_every=10, **kw)
    _check(list(ms_io.get_spectra(fn)), spectra, kw.get("mz_bits", 64))


@pytest.mark.parametrize("kw", [dict(), dict(bits=64), dict(zlib_arrays=False), dict(bits=64, zlib_arrays=False, nested=False)])
def test_mzxml_variants_round_trip(tmp_path, kw):
    spectra = [dict(s, identifier=str(i + 1)) for i, s in enumerate(W.synthetic_spectra(120, seed=12))]
    fn = str(tmp_path / "run.mzXML")
    W.write_mzxml(fn, spectra, ms1_every=7, **kw)
    # retentionTime="PT<s>S" is reported in minutes, as pyteomics does
    _check(list(ms_io.get_spectra(fn)), spectra, kw.get("bits", 32), rt_div=60)


def test_nested_mzxml_scans_are_found(tmp_path):
    spectra = [dict(s, identifier=str(i + 1)) for i, s in enumerate(W.synthetic_spectra(30, seed=13))]
    fn = str(tmp_path / "n.mzxml")
    W.write_mzxml(fn, spectra, ms1_every=10, nested=True)
    txt = open(fn).read()
    assert txt.index('msLevel="2"') < txt.index("</scan>")            # the MS2 scans really sit inside their MS1 scan
    assert [g["identifier"] for g in ms_io.get_spectra(fn)] == [s["identifier"] for s in spectra]


def test_extension_is_case_insensitive_and_mzml_in_scope(tmp_path):
    """main used to answer every .mzML input with 'outside this build's scope ... convert to MGF'"""
    spectra = W.synthetic_spectra(5, seed=14)
    for name in ("x.mzML", "y.MZML", "z.mzml"):
        fn = str(tmp_path / name)
        W.write_mzml(fn, spectra)
        assert len(list(ms_io.get_spectra(fn))) == 5
    fn = str(tmp_path / "w.MZXML")
    W.write_mzxml(fn, [dict(s, identifier=str(i)) for i, s in enumerate(spectra)])
    assert len(list(ms_io.get_spectra(fn))) == 5
    gz = tmp_path / "a.mzML.gz"                                         # compressed inputs stay out of scope, as in the reference
    gz.write_bytes(b"")
    with pytest.raises(ValueError, match="Unknown spectrum file type"):
        list(ms_io.get_spectra(str(gz)))


def test_possible_charge_and_missing_fields(tmp_path):
    spectra = W.synthetic_spectra(20, seed=15)
    fn = str(tmp_path / "c.mzML")
    W.write_mzml(fn, spectra, charge_term="MS:1000633")
    assert [g["precursor_charge"] for g in ms_io.get_spectra(fn)] == [s["precursor_charge"] for s in spectra]
    # no selected ion m/z: skipped, as the reference's KeyError handler does
    txt = open(fn).read().replace('accession="MS:1000744"', 'accession="MS:0000000"', 1)
    open(fn, "w").write(txt)
    assert [g["identifier"] for g in ms_io.get_spectra(fn)] == [s["identifier"] for s in spectra[1:]]


def test_missing_retention_time_is_minus_one(tmp_path):
    spectra = W.synthetic_spectra(4, seed=16)
    fn = str(tmp_path / "r.mzML")
    W.write_mzml(fn, spectra)
    txt = open(fn).read().replace('accession="MS:1000016"', 'accession="MS:1000017"')
    open(fn, "w").write(txt)
    assert [g["retention_time"] for g in ms_io.get_spectra(fn)] == [-1.0] * 4
    fx = str(tmp_path / "r.mzXML")
    W.write_mzxml(fx, [dict(s, identifier=str(i)) for i, s in enumerate(spectra)])
    txt = open(fx).read().replace("retentionTime=", "rtX=")
    open(fx, "w").write(txt)
    assert [g["retention_time"] for g in ms_io.get_spectra(fx)] == [-1.0] * 4
    assert mzxml_io._minutes("PT90.5S") == 90.5 / 60 and mzxml_io._minutes("PT1M30S") == 1.5


@pytest.mark.parametrize("ext", ["mzML", "mzXML"])
def test_truncated_file_keeps_earlier_spectra(tmp_path, caplog, ext):
    spectra = [dict(s, identifier=str(i + 1)) for i, s in enumerate(W.synthetic_spectra(40, seed=17))]
    fn = str(tmp_path / f"t.{ext}")
    (W.write_mzml if ext == "mzML" else W.write_mzxml)(fn, spectra)
    txt = open(fn).read()
    open(fn, "w").write(txt[:len(txt) // 2])
    with caplog.at_level(logging.WARNING, logger="falcon"):
        got = list(ms_io.get_spectra(fn))
    assert 5 < len(got) < 40
    _check(got, spectra[:len(got)], 64 if ext == "mzML" else 32, 1.0 if ext == "mzML" else 60.0)
    assert any("Failed to read file" in r.message for r in caplog.records)


def test_numpress_and_bad_base64_are_skipped_and_counted(tmp_path):
    spectra = W.synthetic_spectra(30, seed=18)
    spectra = [s for s in spectra if len(s["mz"]) >= 8]
    fn = str(tmp_path / "u.mzML")
    W.write_mzml(fn, spectra, numpress={spectra[2]["identifier"]}, bad_base64={spectra[5]["identifier"], spectra[6]["identifier"]})
    (chunk,) = list(mzml_io.read_chunks(fn))
    assert chunk.skipped == {"MS-Numpress linear": 1}
    assert len(chunk) == len(spectra) - 1                               # bad base64 is found when the arrays are decoded
    got = list(chunk.host_spectra())
    assert sum(chunk.skipped.values()) == 3 and any(k.startswith("undecodable") for k in chunk.skipped)
    keep = [s for i, s in enumerate(spectra) if i not in (2, 5, 6)]
    _check(got, keep)


def test_payload_tables_are_aligned(tmp_path):
    spectra = W.synthetic_spectra(25, seed=19)
    fn = str(tmp_path / "p.mzML")
    W.write_mzml(fn, spectra, mz_bits=32, ms1_every=4)
    (chunk,) = list(mzml_io.read_chunks(fn))
    payload, arrays, spec = chunk.tables()
    assert spec.shape == (25, 2) and arrays.shape[1] == 4
    assert np.all(arrays[:, 0] % 8 == 0) and np.all(arrays[:, 1] % 4 == 0)
    assert np.all(arrays[:, 0] + arrays[:, 1] <= len(payload))
    assert np.array_equal(arrays[spec[:, 0], 2], [len(s["mz"]) for s in spectra])


def test_chunks_split_between_spectra(tmp_path):
    spectra = W.synthetic_spectra(60, seed=20)
    fn = str(tmp_path / "s.mzML")
    W.write_mzml(fn, spectra)
    chunks = list(mzml_io.read_chunks(fn, max_bytes=4096))
    assert len(chunks) > 3
    _check([g for c in chunks for g in c.host_spectra()], spectra)


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_decode_kernels_use_no_scratch(tmp_path):
    meta = L.kernel_meta(L.compile_to_asm("peakdecode.hip", tmp_path), "private_segment_fixed_size")
    pd = {k: v for k, v in meta.items() if "pd_" in k}
    assert len(pd) == 5, sorted(pd)
    assert not {k: v for k, v in pd.items() if v}, pd
