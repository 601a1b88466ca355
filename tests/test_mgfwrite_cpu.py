"""`csrc/mgfwrite.h` on the host: the device MGF writer's number text against Python's `repr(float(np.float32(x)))` byte for byte,
its length function, the power-of-five tables against Python integers and the entry layout against `mgf_io.write_spectra` (no
GPU needed)."""
import os

import numpy as np
import pytest

from tests import hostbuild_mgfwrite as H
from tests import isa_lint as L
from tests import mgfwrite_cases as K

pytestmark = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("mgfwriteshim"))


def _check_numbers(lib, x):
    got, length, intact = H.numbers(lib, x)
    assert intact, "a number wrote behind kMgfNumMax bytes"
    want = [K.expected_number(v) for v in x]
    bad = [(x[k].view(np.uint32), got[k], want[k]) for k in range(len(x)) if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(x)} differ: {bad[:10]}"
    assert np.array_equal(length, [len(w) for w in want])
    return max(len(w) for w in want)


def test_number_set_matches_repr(lib):
    x = K.number_set()
    assert len(x) >= 256 * 24 * 2
    longest = _check_numbers(lib, x)
    from falcon_amd import _lib
    assert longest <= lib.t_num_max() == _lib.MGF_NUM_MAX == 23


def test_special_values(lib):
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], np.float32)
    x = np.concatenate([x, np.array([0x7F800001, 0xFFC00000, 0xFFFFFFFF], np.uint32).view(np.float32)])
    got, _, _ = H.numbers(lib, x)
    assert got == [b"0.0", b"-0.0", b"inf", b"-inf", b"nan", b"nan", b"nan", b"nan", b"nan"]


def test_layout_switches(lib):
    """positional text for decimal point positions in (-4, 16], exponent text outside, on both sides of both switches"""
    x = np.array([1e-4, 1.0001e-4, 9.999e-5, 1e16, 9.99999e15, 1.00001e16, 1e22, 1.5e-45, 3.4028235e38, 1.0, 0.001, 123456.79], np.float32)
    got, _, _ = H.numbers(lib, x)
    assert [b"e" in g for g in got] == [True, False, True, True, False, True, True, True, True, False, False, False]
    assert got[0] == b"9.999999747378752e-05" and got[3] == b"1.0000000272564224e+16" and got[7] == b"1.401298464324817e-45"
    assert got[9] == b"1.0" and got[11] == b"123456.7890625" and got[4].endswith(b".0")
    _check_numbers(lib, x)


def test_million_random_bit_patterns(lib):
    longest = _check_numbers(lib, K.random_bits(1_000_000))
    assert longest <= lib.t_num_max()


def test_power_of_five_tables_are_exact(lib):
    inv, pw = H.pow5_table(lib, True), H.pow5_table(lib, False)
    assert len(inv) == 22 and len(pw) == 64
    for q, v in enumerate(inv):
        p = 5 ** q
        assert v == (1 << (p.bit_length() - 1 + 125)) // p + 1, q
    for i, v in enumerate(pw):
        p = 5 ** i
        s = p.bit_length() - 125
        assert v == (p >> s if s >= 0 else p << -s), i
    # the exponents float32 inputs reach stay inside the tables
    e2 = np.arange(-203, 74)
    q_pos = [(e * 78913 >> 18) - (e > 3) for e in e2[e2 >= 0]]
    i_neg = [-e - ((-e * 732923 >> 20) - (-e > 1)) for e in e2[e2 < 0]]
    assert 0 <= min(q_pos) and max(q_pos) < len(inv) and 0 <= min(i_neg) and max(i_neg) < len(pw)


@pytest.mark.parametrize("make", [K.entry_cases, K.number_entries, K.shuffled_rows])
def test_entries_match_write_spectra(lib, make):
    e = make()
    got = []
    for k, r in enumerate(e.rows):
        a, b = e.indptr[r], e.indptr[r + 1]
        text, want_len, intact = H.entry(lib, str(e.title[k]).encode("utf-8"), e.precursor_mz[k], int(e.charge[k]), e.retention_time[k],
                                         int(e.cluster[k]), e.mz[a:b], e.intensity[a:b])
        assert intact and len(text) == want_len
        got.append(text)
    want = e.expected()
    assert b"".join(got) == want


# ---- the host layers --------------------------------------------------------------------------------------------------------
def test_title_blob_offsets():
    from falcon_amd.ms_io import mgf_io
    e = K.entry_cases()
    blob, ptr = mgf_io.title_blob(e.title, "utf-8")
    raw = [str(t).encode("utf-8") for t in e.title]
    assert bytes(blob) == b"".join(raw) and list(np.diff(ptr)) == [len(t) for t in raw] and ptr[0] == 0
    assert mgf_io.title_blob(np.zeros(0, dtype=str), "utf-8")[1].tolist() == [0]
    assert mgf_io.title_blob(np.array(["a\nb", "c"]), "utf-8") is None                 # a newline inside a title
    assert mgf_io.title_blob(np.array(["a\n"]), "utf-8") is None
    assert mgf_io.title_blob(np.array(["\u8d28"]), "ascii") is None                     # the host writer raises on it
    assert mgf_io.title_blob(np.array(["a", "b"]), "utf-16") is None                    # not a superset of ASCII
    assert mgf_io.title_blob(np.array(["a\rb", "c"]), "utf-8")[1].tolist() == [0, 3, 4]


def test_blocks_of_emit_charge_give_the_host_writer_the_same_entries(tmp_path):
    """`falcon._emit_charge` keeps a block of arrays per charge; through the host writer the file is the one the per-cluster
    dicts gave: medoid peaks, or the consensus CSR with the medoid's columns"""
    from falcon_amd import falcon
    from falcon_amd.config import config
    from falcon_amd.ms_io import mgf_io
    e = K.shuffled_rows()
    n = len(e.indptr) - 1
    rng = np.random.default_rng(4)
    part = dict(identifier=np.array([f"id{i}" for i in range(n)]), filename=np.array(["f.mgf"] * n),
                precursor_mz=rng.uniform(300, 900, n).astype(np.float32), retention_time=rng.uniform(0, 50, n).astype(np.float32),
                mz=e.mz, intensity=e.intensity, indptr=e.indptr)
    labels = (np.arange(n) % 7).astype(np.int64)
    medoids = np.array([14, 1, 9, 3, 32, 5, 20])
    cons_ptr = np.array([0, 2, 2, 5, 6, 9, 12, 13], np.int64)
    cons = (cons_ptr, e.mz[100:113].copy(), e.intensity[100:113].copy())
    for consensus in (None, cons):
        config.parse(f"in.mgf {tmp_path / 'out'} --export_representatives --mgf_writer host")
        rows_all, blocks = [], []
        nxt = falcon._emit_charge(part, "2", labels, medoids, 10, rows_all, blocks, consensus)
        nxt = falcon._emit_charge(part, "None", labels, medoids, nxt, rows_all, blocks, consensus)
        assert nxt == 24 and len(blocks) == 2 and len(rows_all) == 2 * n
        fn = str(tmp_path / "blocks.mgf")
        falcon._write_representatives(fn, blocks, None)
        want = []
        for charge, base in ((2, 10), (None, 17)):
            for c, m in enumerate(medoids):
                a, b = (e.indptr[m], e.indptr[m + 1]) if consensus is None else (cons_ptr[c], cons_ptr[c + 1])
                src = (e.mz, e.intensity) if consensus is None else cons[1:]
                want.append({"identifier": f"id{m}", "precursor_mz": float(part["precursor_mz"][m]), "precursor_charge": charge,
                             "retention_time": float(part["retention_time"][m]), "mz": src[0][a:b], "intensity": src[1][a:b],
                             "cluster": int(labels[m]) + base})
        ref = str(tmp_path / "ref.mgf")
        mgf_io.write_spectra(ref, want)
        assert open(fn, "rb").read() == open(ref, "rb").read()


def test_mgf_writer_option(tmp_path, capsys):
    from falcon_amd import falcon
    from falcon_amd.config import Config, config
    c = Config()
    c.parse("in.mgf out")
    assert c.mgf_writer in ("device", "host")
    for w in ("device", "host"):
        c.parse(f"in.mgf out --mgf_writer {w}")
        assert c.mgf_writer == w
    ini = tmp_path / "falcon.ini"
    ini.write_text("mgf_writer = host\n")
    c.parse(f"in.mgf out -c {ini}")
    assert c.mgf_writer == "host"
    ini.write_text("mgf_writer = gpu\n")
    with pytest.raises(SystemExit):
        c.parse(f"in.mgf out -c {ini}")
    with pytest.raises(SystemExit):
        c.parse("in.mgf out --mgf_writer gpu")
    capsys.readouterr()
    config.parse("in.mgf out --export_representatives")
    base = falcon._option_lines()
    config.parse("in.mgf out --export_representatives --mgf_writer host")
    assert falcon._option_lines() == base and not any("mgf_writer" in l for l in base)


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_writer_kernels_use_no_scratch(tmp_path_factory):
    """the formatter keeps its digits in registers and its text in LDS: no private segment (DESIGN.md records the resources)"""
    asm = L.compile_to_asm("mgfwrite.hip", tmp_path_factory.mktemp("isa"))
    res = {k: v for k, v in L.kernel_meta(asm, "private_segment_fixed_size").items() if "mgf_write" in k}
    assert len(res) == 2, sorted(res)
    assert not {k: v for k, v in res.items() if v != 0}
    lds = {k: v for k, v in L.kernel_meta(asm, "group_segment_fixed_size").items() if "mgf_write_kernel" in k}
    assert list(lds.values()) == [4 * 3136]
