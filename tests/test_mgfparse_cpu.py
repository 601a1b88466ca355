"""`csrc/mgfparse.h` on the host: the device MGF reader's number conversion against Python's `float()` bit for bit, its line
classifier, header keys and CHARGE fast form against `mgf_io`'s own logic, and the kernels' resources (no GPU needed)."""
import os

import numpy as np
import pytest

from falcon_amd.ms_io import mgf_io
from tests import hostbuild_mgf as H
from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("mgfshim"))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _corpus():
    rng = np.random.default_rng(20240)
    x = np.exp(rng.uniform(np.log(1e-5), np.log(1e7), 20000))
    toks = [repr(float(v)) for v in x]
    toks += [repr(float(np.float32(v))) for v in x]
    toks += ["%.4f" % v for v in x[:4000]] + ["%.6e" % v for v in x[:4000]] + ["%.6E" % v for v in x[:200]]
    toks += [str(int(v)) for v in x[:2000]] + [str(int(v)) for v in rng.integers(0, 2 ** 62, 2000)]
    toks += ["+5", ".5", "5.", "-0", "1e23", "9007199254740993", "9007199254740995", "0.1", "1e-22", "1e22", "0", "-0.0", "0e5",
             "00012.500", "1E+2", "-.25e-3", "9007199254740992", "9007199254740991", "1e-27", "9999999999999999999e27",
             "0.000000000000000000000001", "123456789012345678.9"]
    # 19-digit integers around multiples of 2^11 (the spacing of doubles in [2^63, 2^64)): exact values, the halfway points where
    # ties go to the even neighbour, and one off either side
    for m in rng.integers(2 ** 52, (10 ** 19 - 1) // 2048 - 2, 300):
        for d in (0, 1, 1023, 1024, 1025, 2047):
            v = int(m) * 2048 + d
            if 10 ** 18 <= v < 10 ** 19:
                toks.append(str(v))
    return toks


def test_numbers_match_float_bit_for_bit(lib):
    toks = _corpus()
    assert len(toks) > 50000
    want = np.array([float(t) for t in toks])                # float() decides every token of the corpus
    got, ok = H.parse_doubles(lib, toks)
    assert ok.all(), [t for t, o in zip(toks, ok) if not o][:20]
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert len(bad) == 0, [(toks[i], got[i].hex(), want[i].hex()) for i in bad[:10]]
    assert np.signbit(got[toks.index("-0")]) and got[toks.index("-0")] == 0.0
    # the corpus reaches every path: Clinger's, the exact product and the long division
    w = np.array([int(t) for t in toks if t.isdigit()], dtype=object)
    assert any(v > 2 ** 53 for v in w) and any(len(t) >= 18 and "." in t and "e" not in t for t in toks)


def test_intensity_is_the_double_rounded_to_float32(lib):
    toks = [repr(float(v)) for v in np.random.default_rng(3).uniform(0, 1e6, 2000)]
    got, ok = H.parse_doubles(lib, toks)
    assert ok.all()
    assert np.array_equal(got.astype(np.float32).view(np.uint32), np.asarray([float(t) for t in toks], np.float32).view(np.uint32))


@pytest.mark.parametrize("tok", ["nan", "inf", "-inf", "1_0", "1e400", "1234567890123456789012345", "1e", "--1", "1.2.3", "",
                                 "+", ".", "e5", "1e+", "0x10", "1 2", "1e28", "1e-28", "Infinity", "1,5", "١"])
def test_tokens_outside_the_grammar_are_not_decided(lib, tok):
    _, ok = H.parse_doubles(lib, [tok.encode("utf-8")])
    assert not ok[0]


def test_charge_fast_form(lib):
    toks = ["2+", "3-", "2", "0", "12+", "007", "2+ and 3+", "2,3", "+2", "2++", "", "+", "two", "1234567890", "2 +", "1_0"]
    got, ok = H.parse_charges(lib, toks)
    for t, g, o in zip(toks, got, ok):
        if o:                                             # decided: what _parse_charge gives
            assert g == mgf_io._parse_charge(t), t
    assert list(ok) == [True] * 6 + [False] * 10


def _host_line(line):
    """mgf_io.get_spectra's own steps on one line inside an open spectrum -> (kind, key, value)"""
    line = line.strip()
    if not line or line[0] in "#;!/":
        return H.SKIP, None, None
    if line == "BEGIN IONS":
        return H.BEGIN, None, None
    if line == "END IONS":
        return H.END, None, None
    if "=" in line and not (line[0].isdigit() or line[0] == "."):
        k, v = line.split("=", 1)
        k = k.strip().lower()
        return H.HEADER, k if k in ("title", "pepmass", "charge", "rtinseconds") else None, v.strip()
    return H.PEAK, None, None


LINES = ["Title = x", "TITLE=a=b", "1.5=3", "+1.5=2", " END IONS \r", "begin ions", "BEGIN IONS", "\tBEGIN IONS  ", "END IONS",
         "END IONS=", "# comment", ";c", "!c", "/c", " # indented", "", "   \t\r", "PEPMASS=431.25 1000", "pepMass =\t12.5\t", "CHARGE=2+",
         "RTINSECONDS= 12.5 ", "rtinseconds=", "SCANS=3", "=x", "TITLE", "100.5 20", ".5=1", "9=1", "a b", "TITLE =", "BEGIN IONS x",
         "CHARGE = 2+ and 3+", "Title\t=\ta b  c"]


def test_classifier_and_header_keys_match_the_host_reader(lib):
    got = H.classify(lib, LINES)
    for line, g in zip(LINES, got):
        assert (g[0] & H.KIND, g[1], g[2]) == _host_line(line), line
        assert not g[0] & H.LONG


def test_long_lines_are_flagged(lib):
    n = lib.t_max_line()
    lines = ["TITLE=" + "x" * (n - 6), "TITLE=" + "x" * (n - 5), "#" + "x" * (2 * n), "1.5 " + " " * n + "2", " " * n + "END IONS"]
    got = H.classify(lib, lines)
    assert [g[0] for g in got] == [H.HEADER, H.HEADER | H.LONG, H.SKIP, H.PEAK | H.LONG, H.END]


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_mgf_kernels_use_no_scratch(tmp_path_factory):
    asm = L.compile_to_asm("mgfparse.hip", tmp_path_factory.mktemp("isa"))
    res = {k: v for k, v in L.kernel_meta(asm, "private_segment_fixed_size").items() if "mgf_" in k}
    assert len(res) >= 7, sorted(res)
    assert not {k: v for k, v in res.items() if v != 0}
