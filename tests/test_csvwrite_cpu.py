"""`csrc/csvwrite.h` on the host: the device CSV writer's number text against `str(np.float32(x))` byte for byte, its comparator
against `falcon._natural_key`, its rows against `csv.writer` as `falcon._write_cluster_info` drives it, and the host layers of
`--csv_writer` (no GPU needed)."""
import csv
import io
import logging
import os

import numpy as np
import pytest

from tests import csvwrite_cases as K
from tests import hostbuild_csvwrite as H
from tests import isa_lint as L

pytestmark = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("csvwriteshim"))


# ---- numbers ------------------------------------------------------------------------------------------------------------------------
def _check_numbers(lib, x):
    got, length, intact = H.numbers(lib, x)
    assert intact, "a number wrote behind kCsvNumMax bytes"
    want = [K.expected_number(v) for v in x]
    bad = [(hex(int(x[k:k + 1].view(np.uint32)[0])), got[k], want[k]) for k in range(len(x)) if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(x)} differ: {bad[:10]}"
    assert np.array_equal(length, [len(w) for w in want])
    return max(len(w) for w in want)


def test_number_set_matches_numpy(lib):
    x = K.number_set()
    assert len(x) > 100_000
    longest = _check_numbers(lib, x)
    from falcon_amd import _lib
    assert longest == lib.t_num_max() == _lib.CSV_NUM_MAX == 19          # "-9999999000000000.0"


def test_special_values_and_layout_switches(lib):
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-4, 9.999999e15, 1e16, 0.1, 1.0001e-4], np.float32)
    x = np.concatenate([x, np.array([0xFFC00000, *K.NUMPY_EIGHT_DIGITS], np.uint32).view(np.float32)])
    got, _, _ = H.numbers(lib, x)
    assert got[:10] == [b"0.0", b"-0.0", b"inf", b"-inf", b"nan", b"1e-04", b"9999999000000000.0", b"1e+16", b"0.1", b"0.00010001"]
    assert got[10:] == [b"nan", b"1.2621775e-29", b"1.5474251e+26", b"1.2379401e+27"]
    _check_numbers(lib, x)


def test_random_bit_patterns_match_numpy(lib):
    assert _check_numbers(lib, K.random_bits(200_000)) <= lib.t_num_max()


# ---- the comparator -------------------------------------------------------------------------------------------------------------------
def test_comparator_matches_natural_key_on_every_pair(lib):
    from falcon_amd.falcon import _natural_key
    s = K.compare_strings()
    assert {"", "1", "01", "001", "a", "a1", "a01", "a!", "a1b", "a9", "a10", "a1b2", "a1b10", "ab", "ab1", "abc1"} <= set(s)
    got = H.cmp_all(lib, s)
    keys = [_natural_key(t) for t in s]
    zeros = 0
    for i in range(len(s)):
        for j in range(len(s)):
            want = (keys[i] > keys[j]) - (keys[i] < keys[j])
            assert got[i, j] == want, (s[i], s[j], int(got[i, j]), want)
            assert (got[i, j] == 0) == (keys[i] == keys[j])
            zeros += want == 0 and i != j
    assert zeros >= 20                                    # leading-zero ties are in the list
    assert got[s.index("a1"), s.index("a!")] == -1       # a plain byte compare says otherwise


def test_longest_digit_run(lib):
    assert [H.max_digit_run(lib, t) for t in (b"", b"abc", b"7", b"a12b345c6", b"0001", b"9" * 5000 + b"x1")] == [0, 0, 1, 3, 4, 5000]


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
def _writer_rows(tuples):
    out = io.StringIO(newline="")
    w = csv.writer(out, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    for fn, sid, charge, pmz, rt, lab in tuples:
        w.writerow([fn, sid, charge, str(np.float32(pmz)), str(np.float32(rt)), lab])      # falcon._write_cluster_info's row
    return out.getvalue().encode("ascii")


@pytest.mark.parametrize("name", K.ROW_SETS)
def test_rows_match_csv_writer(lib, name):
    from falcon_amd.ms_io import csv_io
    rows = getattr(K, name)()
    quote_cr = csv_io.host_quotes_cr()
    got = []
    for i, t in enumerate(rows.tuples()):
        text, want_len, intact = H.row(lib, t[0].encode("ascii"), t[1].encode("ascii"), int(rows.charge[i]), float(rows.precursor_mz[i]),
                                       float(rows.retention_time[i]), int(rows.cluster[i]), quote_cr)
        assert intact and len(text) == want_len
        got.append(text)
    want = _writer_rows(rows.tuples())
    assert b"".join(got) == want
    if name == "ascii_rows":
        m = 127 if K.host_writes_nul() else 126
        ids = set(rows.identifier[:m])
        assert len(ids) == m and "\n" not in ids and "\x7f" in ids and set(rows.filename[m:2 * m]) == ids and 2 ** 62 in rows.cluster
        assert b'f.mzML,"""",' in want and b'f.mzML,",",' in want and b",None," in want and b",-2147483648," in want


def test_carriage_return_follows_the_flag(lib):
    assert H.row(lib, b"f", b"a\rb", 2, 1.0, 2.0, 3, False)[0] == b"f,a\rb,2,1.0,2.0,3\n"
    assert H.row(lib, b"f", b"a\rb", 2, 1.0, 2.0, 3, True)[0] == b'f,"a\rb",2,1.0,2.0,3\n'


# ---- the host layers --------------------------------------------------------------------------------------------------------------------
def test_file_ranks_give_names_with_equal_keys_one_rank():
    from falcon_amd.falcon import _natural_key
    from falcon_amd.ms_io import csv_io
    fn = np.array(["b10.mgf"] * 3 + ["b9.mgf"] * 2 + ["b09.mgf"] + ["a.mgf"] * 2 + ["b10.mgf"] + ["b009.mgf"] * 2)
    file_id, names, rank = csv_io.file_ranks(fn, _natural_key)
    assert names == ["b10.mgf", "b9.mgf", "b09.mgf", "a.mgf", "b009.mgf"]
    assert [names[i] for i in file_id] == fn.tolist()
    assert rank.tolist() == [2, 1, 1, 0, 1]
    assert csv_io.file_ranks(np.zeros(0, dtype=str), _natural_key)[1] == []


class _NoDevice:
    """a context that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError(f"the device writer was used: {name}")


class _LongRuns:
    """a context whose order call reports a digit run of 5,000"""

    def to_dev(self, a, dtype=None):
        return a

    _text_to_dev = to_dev

    def csv_order(self, *a):
        return None, 5000

    def format_csv(self, *a, **k):
        raise AssertionError("rows were formatted")


def _blocks():
    rows = K.ascii_rows().take(np.arange(130, 143))
    a, b = rows.take(np.arange(0, 6)), rows.take(np.arange(6, 13))
    a.charge[:], b.charge[:] = 2, 0
    return [a.block(), b.block()], a.tuples(through_numpy=True) + b.tuples(through_numpy=True)


@pytest.mark.parametrize("why", ["no context", "newline", "non-ascii", "float64", "digit run"])
def test_each_fallback_selects_the_host_writer(tmp_path, caplog, why):
    """the block path through the host writer gives the file the tuple path gives, with one debug line saying why"""
    from falcon_amd import falcon
    from falcon_amd.config import config
    blocks, tuples = _blocks()
    ctx = _NoDevice()
    if why == "no context":
        ctx = None
    elif why in ("newline", "non-ascii"):
        text = "two\nlines" if why == "newline" else "münchen=3"
        blocks[1]["identifier"] = np.array([text] + blocks[1]["identifier"][1:].tolist(), dtype=str)
        tuples[6] = (tuples[6][0], text) + tuples[6][2:]
    elif why == "float64":
        blocks[0]["retention_time"] = blocks[0]["retention_time"].astype(np.float64)
    else:
        ctx = _LongRuns()
    want_rows = sorted(tuples, key=lambda r: (falcon._natural_key(r[0]), falcon._natural_key(r[1])))
    want = K.body_of(want_rows, tmp_path)
    config.parse(["in.mgf", str(tmp_path / "blocks"), "--csv_writer", "device"])
    with caplog.at_level(logging.DEBUG, logger="falcon"):
        falcon._write_outputs([], [], ctx, csv_blocks=blocks)
    raw = open(tmp_path / "blocks.csv", "rb").read()
    assert raw[raw.index(K.COLUMN_ROW) + len(K.COLUMN_ROW):] == want and len(want_rows) == 13
    said = [r.getMessage() for r in caplog.records if "the host writer writes" in r.getMessage()]
    assert len(said) == 1, said


def test_emit_charge_collects_column_blocks_not_tuples(tmp_path):
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse(["in.mgf", str(tmp_path / "o")])
    n = 9
    part = dict(identifier=np.array([f"scan={i}" for i in range(n)]), filename=np.array(["f.mgf"] * n),
                precursor_mz=np.linspace(300, 900, n).astype(np.float32), retention_time=np.linspace(0, 50, n).astype(np.float32))
    labels = (np.arange(n) % 4).astype(np.int64)
    rows_all, blocks = [], []
    assert falcon._emit_charge(part, "3", labels, [0, 1, 2, 3], 10, rows_all, [], csv_blocks=blocks) == 14
    assert falcon._emit_charge(part, "None", labels, [0, 1, 2, 3], 14, rows_all, [], csv_blocks=blocks) == 18
    assert rows_all == [] and [b["charge"] for b in blocks] == [3, 0]
    from falcon_amd.ms_io import csv_io
    tuples = []
    falcon._emit_charge(part, "3", labels, [0, 1, 2, 3], 10, tuples, [])
    falcon._emit_charge(part, "None", labels, [0, 1, 2, 3], 14, tuples, [])
    assert list(csv_io.block_tuples(blocks)) == tuples


def test_csv_writer_option(tmp_path, capsys):
    from falcon_amd import falcon
    from falcon_amd.config import Config, config
    c = Config()
    c.parse("in.mgf out")
    assert c.csv_writer in ("device", "host")
    for w in ("device", "host"):
        c.parse(f"in.mgf out --csv_writer {w}")
        assert c.csv_writer == w
    ini = tmp_path / "falcon.ini"
    ini.write_text("csv_writer = host\n")
    c.parse(f"in.mgf out -c {ini}")
    assert c.csv_writer == "host"
    ini.write_text("csv_writer = gpu\n")
    with pytest.raises(SystemExit):
        c.parse(f"in.mgf out -c {ini}")
    with pytest.raises(SystemExit):
        c.parse("in.mgf out --csv_writer gpu")
    capsys.readouterr()
    config.parse("in.mgf out --csv_writer device")
    base = falcon._option_lines()
    config.parse("in.mgf out --csv_writer host")
    assert falcon._option_lines() == base and not any("csv_writer" in l for l in base)


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_writer_kernels_use_no_scratch(tmp_path_factory):
    """the formatter keeps its digits in registers and its text in LDS: no private segment; four 8 KiB tiles per block"""
    asm = L.compile_to_asm("csvwrite.hip", tmp_path_factory.mktemp("isa"))
    res = {k: v for k, v in L.kernel_meta(asm, "private_segment_fixed_size").items() if "csv_write" in k or "csv_check" in k}
    assert len(res) == 3, sorted(res)
    assert not {k: v for k, v in res.items() if v != 0}
    lds = {k: v for k, v in L.kernel_meta(asm, "group_segment_fixed_size").items() if "csv_write_kernel" in k}
    assert list(lds.values()) == [4 * 8192]
