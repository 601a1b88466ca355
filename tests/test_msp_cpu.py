"""`csrc/mspparse.h` on the host against a Python restatement of the MSP grammar (`tests/msp_cases.py`), the host reader
`msp_io.read_annotation_library` on three hand-written styles and on designed entries for every rule, the `--msp_reader` option,
and the new kernels' resources (no GPU needed)."""
import os

import numpy as np
import pytest

from falcon_amd.ms_io import mgf_io, msp_io
from tests import hostbuild_msp as H
from tests import isa_lint as L
from tests import msp_cases as M

needs_compiler = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("mspshim"))


LINES = ["", "   ", "\t\r", "Name: x", "name:x", "  NAME :x", "Name:a:b", "Names:", "Nam: e", "name", "Name", "Num Peaks: 3", "NUM PEAKS:3", "num peaks :",
         "Num  Peaks: 3", "NumPeaks: 3", "Num Peaks 3", "PrecursorMZ: 500.5", "DB#: 7", "Comments: \"a:b\"", ": no key", ":", "100.5 20", "100.5 20; 3 4",
         "1:2", "Name: x\r", "\tName\t:\tx\t", "x" * 4096, "k: " + "x" * 4093, "k: " + "x" * 4094, " " * 5000, " " * 3000 + "Name: padded" + " " * 3000,
         "Name: " + "n" * 4091]


def _kind(line: bytes):
    s = line.strip(M.WS)
    if not s:
        return H.BLANK
    key = M.split_line(s)[0]
    kind = H.OTHER if key is None else H.NAME if key == b"name" else H.NUMPEAKS if key == b"num peaks" else H.HEADER
    return kind | (H.LONG if len(s) > 4096 else 0)


@needs_compiler
def test_line_kinds_and_the_split_at_the_first_colon(lib):
    got = H.lines(lib, LINES)
    for line, (kind, key, value) in zip(LINES, got):
        raw = line.encode()
        s = raw.strip(M.WS)
        assert kind == _kind(raw), line[:40]
        want_key, _, want_value = M.split_line(s)
        assert (key.lower().encode() if key is not None else None) == want_key and value.encode() == want_value, line[:40]
    by = dict(zip(LINES, got))
    assert by["Name:a:b"] == (H.NAME, "Name", "a:b") and by["  NAME :x"] == (H.NAME, "NAME", "x") and by["Names:"] == (H.HEADER, "Names", "")
    assert by["name"] == (H.OTHER, None, "") and by["Num Peaks 3"][0] == H.OTHER and by["Num  Peaks: 3"][0] == H.HEADER
    assert by["100.5 20"][0] == H.OTHER and by["1:2"] == (H.HEADER, "1", "2") and by[": no key"] == (H.HEADER, "", "no key")
    assert by["x" * 4096][0] == H.OTHER and by["k: " + "x" * 4093][0] == H.HEADER and by["k: " + "x" * 4094][0] == H.HEADER | H.LONG
    assert by[" " * 5000][0] == H.BLANK and by[" " * 3000 + "Name: padded" + " " * 3000][0] == H.NAME
    assert {k & H.KIND for k, _, _ in got} == {H.BLANK, H.NAME, H.NUMPEAKS, H.HEADER, H.OTHER}


PEAK_LINES = ["1 2;3 4;", ";;", "1 2 \"a;b\"", "\"1 2; 3 4", "", "1 2", "1", " 1\t2 ; 3 ", "1 2;;3 4", "; ;\t;", "1 2 3 4; 5", "1 2 \"a\"; 3 4", "1 2; 3 4 \"x;y\" ; 5 6",
              ";1 2", "1 2;", "a b; c", "1;2;3;4;5;6;7;8;9;10", " ; 1 2 ; ", "Num Peaks: 3", "1 2\r", "12.5\t7\t\"note\""]


@needs_compiler
def test_peak_segments_and_their_tokens(lib):
    got = H.segments(lib, PEAK_LINES)
    for line, (count, toks) in zip(PEAK_LINES, got):
        want = M.segments(line.encode())
        assert count == len(want), line
        for (a, b), seg in zip(toks, want):
            t = seg.split()
            assert a.encode() == t[0] and b.encode() == (t[1] if len(t) > 1 else b""), line
    by = {line: count for line, (count, _) in zip(PEAK_LINES, got)}
    assert [by[k] for k in ("1 2;3 4;", ";;", "1 2 \"a;b\"", "\"1 2; 3 4", "")] == [2, 0, 1, 0, 0]
    assert by["1;2;3;4;5;6;7;8;9;10"] == 10 and by["1 2 \"a\"; 3 4"] == 1 and by["Num Peaks: 3"] == 1
    assert dict(zip(PEAK_LINES, got))["1 2 3 4; 5"][1] == [("1", "2"), ("5", "")]


COUNTS = ["3", "03", "+3", "3 4", "1234567890", "123456789", "0", "", "-3", "3.0", "1_0", " 3", "3 ", "٣".encode("utf-8"), "000000000", "0000000001"]


@needs_compiler
def test_the_num_peaks_fast_form(lib):
    got, ok = H.counts(lib, COUNTS)
    assert [t for t, o in zip(COUNTS, ok) if o] == ["3", "03", "123456789", "0", "000000000"]
    for t, g, o in zip(COUNTS, got, ok):
        assert (M.fast_count(t if isinstance(t, bytes) else t.encode()) is not None) == bool(o), t
        if o:
            assert int(g) == int(t), t
    # what it leaves open, int() takes ("+3", 10 digits, "1_0", padded forms) or refuses ("3 4", "3.0"): never a guess
    assert int("+3") == 3 and int("1234567890") == 1234567890 and int("1_0") == 10 and int(" 3") == 3
    for t in ("3 4", "3.0", ""):
        with pytest.raises(ValueError):
            int(t)


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_the_msp_kernels_use_no_scratch(tmp_path_factory):
    asm = L.compile_to_asm("mspparse.hip", tmp_path_factory.mktemp("isa"))
    res = L.kernel_meta(asm, "private_segment_fixed_size")
    mine = {k: v for k, v in res.items() if "msp_" in k}
    assert sum("msp_parse_kernel" in k for k in mine) == 1 and sum("msp_headers_kernel" in k for k in mine) == 1 and len(mine) == 9, sorted(res)
    assert not {k: v for k, v in mine.items() if v != 0}


# ---- the host reader --------------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, text, newline="\n"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(text.replace("\n", newline).encode("ascii"))
    return path


def _check(spec, want):
    for k in ("identifier", "name", "precursor_mz", "precursor_charge", "adduct", "ionmode", "smiles", "inchikey"):
        assert spec[k] == want[k], (k, spec[k], want[k])
    assert spec["retention_time"] == -1.0 and spec["mz"].dtype == np.float64 and spec["intensity"].dtype == np.float32
    assert spec["mz"].tolist() == want["mz"] and spec["intensity"].tolist() == [np.float32(v) for v in want["intensity"]]


@pytest.mark.parametrize("style", sorted(M.STYLES))
@pytest.mark.parametrize("newline", ["\n", "\r\n"], ids=["lf", "crlf"])
def test_the_host_reader_on_the_three_styles(tmp_path, style, newline):
    text, want = M.STYLES[style]
    path = _write(tmp_path, f"{style}.msp", text, newline)
    counts = {}
    got = msp_io.read_annotation_library([path], counts)
    assert len(got) == len(want) and counts == dict(entries=len(want), skipped=0)
    for g, w in zip(got, want):
        _check(g, w)
        assert g["filename"] == path and sorted(g) == sorted(["identifier", "precursor_mz", "precursor_charge", "retention_time", "mz", "intensity", "name",
                                                               "filename", "adduct", "smiles", "inchikey", "ionmode"])


E, DESIGNED = M.entry, M.DESIGNED


def test_the_host_reader_on_designed_entries(tmp_path):
    text = "Comment: before the first entry\n100.5 1\nNum Peaks: 1\n\n" + "".join(t for t, _ in DESIGNED)
    for newline in ("\n", "\r\n"):
        path = _write(tmp_path, "designed.msp", text, newline)
        counts = {}
        got = msp_io.read_annotation_library([path], counts)
        kept = [(i + 1, w) for i, (_, w) in enumerate(DESIGNED) if w is not None]
        assert counts == dict(entries=len(DESIGNED), skipped=len(DESIGNED) - len(kept)) and len(got) == len(kept)
        default = dict(precursor_mz=500.5, precursor_charge=0, adduct="", ionmode="", smiles="", inchikey="", mz=[100.5, 200.25, 150.125], intensity=[1.0, 3.5, 2.0])
        for g, (number, w) in zip(got, kept):
            name = DESIGNED[number - 1][0].split("\n")[0].split(":", 1)[1].strip()
            _check(g, {**default, "identifier": f"designed.msp:{number}", "name": name, **w})
    assert DESIGNED[8][1] == dict(identifier="designed.msp:9")                     # (numbered behind kept entries; skipped ones count too:)
    assert [n for n, _ in kept][-1] == len(DESIGNED) and sum(w is None for _, w in DESIGNED[:kept[-1][0]]) == 14


def test_two_files_count_from_one_each_and_the_last_entry_needs_no_newline(tmp_path):
    a = _write(tmp_path, "a.msp", E("one") + E("skipped", pm=None) + E("three", blank=False).rstrip("\n"))
    b = _write(tmp_path, "B.MSP", "\n\n" + E("first of b"))
    counts = {}
    got = msp_io.read_annotation_library([a, b], counts)
    assert [s["identifier"] for s in got] == ["a.msp:1", "a.msp:3", "B.MSP:1"] and counts == dict(entries=4, skipped=1)
    assert [s["filename"] for s in got] == [a, a, b] and got[1]["mz"].tolist() == [100.5, 200.25, 150.125]
    assert msp_io.read_annotation_library([_write(tmp_path, "empty.msp", "no entry here\n")], counts) == [] and counts == dict(entries=0, skipped=0)


def test_the_cut_in_front_of_a_name_line():
    text = (E("one") + E("two") + E("three")).encode()
    at = msp_io._cut(bytearray(text), False)
    assert text[at:].startswith(b"Name: three") and msp_io._cut(bytearray(text), True) == len(text)
    assert msp_io._cut(bytearray(E("only one").encode()), False) == 0 and msp_io._cut(bytearray(b"x" * 300000), False) == 0
    far = (E("one") + E("two", peaks=["1 2"] * 40000)).encode()                     # the last Name: line lies outside the first window
    assert far[msp_io._cut(bytearray(far), False):].startswith(b"Name: two")
    for tail, want in ((b"  nAmE\t: partial", b"  nAmE\t: partial"), (b"Names: x\nname", b"Name: three")):
        longer = text + tail
        assert longer[msp_io._cut(bytearray(longer), False):].startswith(want)


def test_the_msp_reader_option(tmp_path):
    from falcon_amd.config import config
    config.parse(["in.mgf", "out"])
    default = config.msp_reader
    assert default in ("device", "host")
    config.parse(["in.mgf", "out", "--msp_reader", "host"])
    assert config.msp_reader == "host"
    ini = tmp_path / "falcon.ini"
    ini.write_text("msp_reader = device\n")
    config.parse(["in.mgf", "out", "-c", str(ini)])
    assert config.msp_reader == "device"
    ini.write_text("msp_reader = elsewhere\n")
    with pytest.raises(SystemExit):
        config.parse(["in.mgf", "out", "-c", str(ini)])
    with pytest.raises(SystemExit):
        config.parse(["in.mgf", "out", "--msp_reader", "elsewhere"])
    config.parse(["in.mgf", "out"])
    assert config.msp_reader == default


def test_mgf_stretches_keep_their_cut_and_parser():
    """`mgf_io._stretches` without the new arguments cuts behind END IONS and parses with `ctx.parse_mgf`, as before"""
    import inspect
    sig = inspect.signature(mgf_io._stretches)
    assert sig.parameters["cut"].default is None and sig.parameters["parser"].default is None
