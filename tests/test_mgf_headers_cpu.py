"""`csrc/mgfkeys.h` on the host: the table key of a header line against the host readers' `line.split("=", 1)` rule, the integer
fast form against Python's `int()`, the new kernels' resources, and the host library / representative readers pinned to the
outputs they had before their per-entry rule was factored out (no GPU needed)."""
import codecs
import hashlib
import locale
import os

import numpy as np
import pytest

from falcon_amd.ms_io import mgf_io
from tests import hostbuild_mgf_headers as H
from tests import isa_lint as L
from tests import mgf_library_cases as K

needs_compiler = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("mgfheadersshim"))


KEY32 = "k" * 32
TABLE = ["spectrumid", "name", "compound_name", "smiles", "cluster", "a", "two words", KEY32]
LINES = ["NAME=x", "name=x", "NaMe = padded ", "\tName\t=\tv\t", "  SMILES=C=O", "SMILES = C=O=", "NAMES=not name", "NAM=prefix", "NA=",
         "COMPOUND_NAME=c", "COMPOUND=", "COMPOUND_NAME2=", "_NAME=", "A=1", "a =", "AA=1", "=no key", "name", "two words=1", "TWO  WORDS=1",
         "Two Words = 2 ", "two words extra=1", KEY32.upper() + "=32", KEY32 + "k=33", " " + KEY32 + " = padded 32", "cluster=12",
         "CLUSTER==3", "spectrumid=CCMSLIB1 = 2", "name=", "name= ", "name==", "TITLE=own key of the parser", "name\r", "name=\r"]


def _host_key(line):
    """the host readers' own steps on a header line -> (key if it is a table key, value)"""
    line = line.strip()
    k, v = line.split("=", 1) if "=" in line else (line, "")
    k = k.strip().lower()
    return (k if k in TABLE else None), v.strip()


@needs_compiler
def test_table_keys_match_the_host_split(lib):
    assert lib.t_max_keys() == 16 and lib.t_max_key_bytes() == 32 and len(KEY32) == lib.t_max_key_bytes()
    got = H.table_keys(lib, LINES, TABLE)
    for line, g in zip(LINES, got):
        assert g == _host_key(line), line
    found = {g[0] for g in got}
    assert found == set(TABLE) | {None}
    assert dict(zip(LINES, got))["  SMILES=C=O"] == ("smiles", "C=O") and dict(zip(LINES, got))[KEY32 + "k=33"][0] is None


@needs_compiler
def test_a_table_of_one_and_of_sixteen_keys(lib):
    keys = [f"key{j:02d}" for j in range(16)]
    lines = [f"KEY{j:02d}= v{j}" for j in range(16)] + ["key16=x", "key0=x"]
    assert H.table_keys(lib, lines, keys) == [(k, f"v{j}") for j, k in enumerate(keys)] + [(None, "x"), (None, "x")]
    assert H.table_keys(lib, lines[:2], keys[1:2]) == [(None, "v0"), ("key01", "v1")]


INTS = ["0", "007", "-3", "+7", "9" * 18, "-" + "9" * 18, "1" + "0" * 17, "9" * 19, "1" + "0" * 18, "-0", "+0", "", "1_0", "1 2", "+", "-",
        "٣".encode("utf-8"), "0x5", "1.0", "1e3", " 1", "1 ", "--1", "+-1", "12a", "a12", "1+"]


@needs_compiler
def test_integer_fast_form_matches_int(lib):
    got, ok = H.parse_ints(lib, INTS)
    decided = [t for t, o in zip(INTS, ok) if o]
    assert decided == ["0", "007", "-3", "+7", "9" * 18, "-" + "9" * 18, "1" + "0" * 17, "-0", "+0"]
    for t, g, o in zip(INTS, got, ok):
        if o:                                             # decided: what int() gives
            assert int(g) == int(t), t
    # what it leaves open, int() takes ("1_0", 19 digits, the Arabic-Indic digit, padded forms) or refuses: never a guess
    text = [t.decode("utf-8") if isinstance(t, bytes) else t for t in INTS]
    assert int(text[INTS.index("1_0")]) == 10 and int(text[INTS.index("٣".encode("utf-8"))]) == 3 and int("9" * 19) > 2 ** 63 - 1
    for t in ("", "1 2", "+", "0x5"):
        with pytest.raises(ValueError):
            int(t)


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_header_kernels_use_no_scratch(tmp_path_factory):
    asm = L.compile_to_asm("mgfparse.hip", tmp_path_factory.mktemp("isa"))
    res = L.kernel_meta(asm, "private_segment_fixed_size")
    new = {k: v for k, v in res.items() if "mgf_headers_kernel" in k or "text_rows_kernel" in k}
    assert len(new) == 2, sorted(res)
    assert not {k: v for k, v in new.items() if v != 0}


# ---- the host readers, pinned ------------------------------------------------------------------------------------------------
# Recorded from `read_annotation_library` / `read_library` as they were before `_annotation_entry` was factored out, on
# `mgf_library_cases.write_corpus`: the SHA-256 of repr(canonical(entries)), and the designed entries spelled out.
FROZEN_BOTH = (286, dict(entries=292, skipped=6), "7767ac3d4e61fea5f8534fabaa1e07dbb8deabb728ebb87385cfbee9e5dcf763")
FROZEN_REPS = "148b7d8c047099e137008c04e2a256471504c63631f5cde03dcc8f7ef9056878"
# (identifier, charge, name, adduct, smiles, inchikey) of every entry that is none of the clean ones, in order
DESIGNED = [
    ("the title stands in", 0, "a", "", "", ""), ("lib_one.mgf:32", 0, "fallback id behind skipped entries", "", "", ""),
    ("S1", 0, "the compound name stands in", "", "", ""), ("S2", 0, "", "", "", ""), ("S3", 0, "", "", "", ""), ("S4", -1, "", "", "", ""),
    ("S5", 2, "", "", "", ""), ("S8", 0, "", "", "", ""), ("S10", 0, "second BEGIN wins", "", "", ""),
    ("S11", 0, "", "last", "CC=O", "MixedCase"), ("S12", 0, "n" * 256, "", "C" * 300, "k" * 257), ("S13", 0, "x" * 5000, "", "", ""),
    ("only a title", 0, "", "", "", ""), ("S14", 0, "", "", "", ""), ("S15", 0, "", "", "", ""), ("S16", 0, "", "", "", ""),
    ("lib_two.mgf:61", 0, "fallback id in front of the name outside the grammar", "", "", ""), ("S100", 0, "caféine", "", "", ""),
    ("lib_two.mgf:64", 0, "and its numbering goes on", "", "", ""),
]


def _digest(rows):
    return hashlib.sha256(repr(rows).encode()).hexdigest()


def test_the_host_library_reader_is_what_it_was(tmp_path):
    files = K.write_corpus(tmp_path)
    if codecs.lookup(locale.getpreferredencoding(False)).name != "utf-8":         # (the second file holds a UTF-8 name)
        with open(files[1], "rb") as f:
            raw = f.read()
        with open(files[1], "wb") as f:
            f.write(raw.decode("utf-8").encode(locale.getpreferredencoding(False), "replace"))
    counts = {}
    got = K.canonical(mgf_io.read_annotation_library(files, counts))
    small = [dict(g) for g in got if not dict(g)["identifier"].startswith("CCMSLIB")]
    name = lambda s: s if s != "caf?ine" else "caféine"                      # noqa: E731 -- (a locale without the letter)
    assert [(s["identifier"], s["precursor_charge"], name(s["name"]), s["adduct"], s["smiles"], s["inchikey"]) for s in small] == DESIGNED
    assert all(s["retention_time"] == (-1.0).hex() and s["ionmode"] == "" for s in small)
    assert [s["precursor_mz"] for s in small if s["identifier"] == "S14"] == [float("1e40").hex()]
    assert (len(got), counts) == FROZEN_BOTH[:2]
    if all(s["name"] != "caf?ine" for s in small):
        assert _digest(got) == FROZEN_BOTH[2]


def test_the_host_representative_reader_is_what_it_was(tmp_path):
    rng = np.random.default_rng(3)
    specs = [{"identifier": f"rep {i}", "precursor_mz": float(rng.uniform(300, 900)), "precursor_charge": [None, 2, -1][i % 3],
              "retention_time": float(i), "cluster": 5 * i + 1, "mz": np.sort(rng.uniform(100, 900, 6)),
              "intensity": rng.uniform(1, 100, 6).astype(np.float32)} for i in range(9)]
    a, b = str(tmp_path / "reps.mgf"), str(tmp_path / "reps2.mgf")
    mgf_io.write_spectra(a, specs)
    with open(b, "w") as f:
        f.write(K.rep("plus", "+7") + K.rep("underscore", "1_0") + K.rep("rejected", "3", pep=None) + K.rep("last", " 12 ", "CLUSTER=99"))
    got = mgf_io.read_library([a, b])
    assert [s["cluster"] for s in got] == [1, 6, 11, 16, 21, 26, 31, 36, 41, 7, 10, 12]
    assert [s["identifier"] for s in got[9:]] == ["plus", "underscore", "last"] and [s["filename"] for s in got] == [a] * 9 + [b] * 3
    assert _digest(K.canonical(got)) == FROZEN_REPS
    with open(b, "a") as f:
        f.write(K.rep("again", "6"))
    with pytest.raises(mgf_io.MgfLibraryError) as e:
        mgf_io.read_library([a, b])
    assert str(e.value) == f"{b}: spectrum 4 (TITLE=again) repeats CLUSTER=6 of {a} (TITLE=rep 1)"
