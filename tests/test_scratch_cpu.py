"""csrc/scratch.h without a GPU (tests/hostbuild_scratch.py): the offsets and the one request of small layouts, the failures
that must not reach the context, three of the library's layouts against the size formulas they replaced, and a stand-alone
program that writes every array end to end under AddressSanitizer + UBSan."""
import subprocess

import pytest

from tests import hostbuild_scratch as hb
from tests.hostbuild import have_compiler
from tests.hostbuild_scratch import F64, I32, I64, PAD, U8

pytestmark = pytest.mark.skipif(not have_compiler(), reason="no host C++ compiler and no hipcc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hb.build(tmp_path_factory.mktemp("scratch"))


def _ok(lib, statements, slot=5):
    rc, off, seen, null_before = hb.layout(lib, statements, slot=slot)
    assert rc == 0 and null_before
    assert seen["calls"] == 1 and seen["slot"] == slot and seen["asked"] == seen["bytes"]     # one request, for the whole block
    return off, seen["bytes"]


def test_a_wider_array_behind_a_byte_is_padded_to_its_alignment(lib):
    assert _ok(lib, [(U8, 1), (I64, 1)]) == ([0, 8], 16)


def test_three_words_then_int64_start_at_16_not_12(lib):
    assert _ok(lib, [(I32, 3), (I64, 2)], slot=11) == ([0, 16], 32)


def test_wider_arrays_first_pack_without_padding(lib):
    assert _ok(lib, [(F64, 2), (I32, 3), (U8, 5)]) == ([0, 16, 28], 33)


def test_a_zero_length_array_moves_nothing_and_points_at_its_successor(lib):
    off, total = _ok(lib, [(I64, 2), (I32, 0), (I32, 3)])
    assert off == [0, 16, 16] and total == 28
    assert _ok(lib, [(I64, 2), (I32, 3)]) == ([0, 16], 28)


def test_pad_at_the_end_and_in_the_middle(lib):
    assert _ok(lib, [(I32, 3), (PAD, 64)]) == ([0, -2], 76)
    assert _ok(lib, [(I32, 3), (PAD, 64), (I64, 1)]) == ([0, -2, 80], 88)      # 12 + 64 = 76 -> the next multiple of 8
    assert _ok(lib, [(PAD, 64), (U8, 1)]) == ([-2, 64], 65)


@pytest.mark.parametrize("statements", [
    [(I32, 4), (I64, -1)],                    # a negative count
    [(I64, -1), (I32, 4)],
    [(I32, 4), (I64, 2 ** 61)],               # 2^64 bytes
    [(I64, 2 ** 60), (I64, 2 ** 60)],         # each fits, the sum does not
    [(I32, 4), (PAD, -8)],
])
def test_bad_counts_fail_closed_without_asking_the_context(lib, statements):
    rc, off, seen, null_before = hb.layout(lib, statements)
    assert rc == lib.t_einternal() and null_before
    assert seen["calls"] == 0
    assert all(o < 0 for o in off)            # every handle still yields nullptr


def test_the_contexts_failure_comes_back_unchanged_and_handles_stay_null(lib):
    rc, off, seen, _ = hb.layout(lib, [(I64, 2), (I32, 3)], fail=lib.t_enomem())
    assert rc == lib.t_enomem() and rc != lib.t_einternal()
    assert seen["calls"] == 1 and seen["asked"] == 28
    assert off == [-1, -1]


@pytest.mark.parametrize("n,m", [(3, 5), (0, 0), (4, 2)])
def test_families_block_is_the_formula_it_replaced(lib, n, m):
    rc, off, seen = hb.real(lib.t_families, 8, n, m)
    assert rc == 0 and seen["calls"] == 1 and seen["asked"] == seen["bytes"]
    assert seen["bytes"] == 64 + 8 * (n + 1) + 20 * n + 4 * m
    rank = 64                                 # blk + 64; parent = rank + n + 1; root, size, flag, lo n words each; round
    parent = rank + 8 * (n + 1)
    assert off == [0, rank, parent, parent + 4 * n, parent + 8 * n, parent + 12 * n, parent + 16 * n, parent + 20 * n]


@pytest.mark.parametrize("m", [1, 2])
def test_sorted_records_block_is_the_formula_it_replaced(lib, m):
    rc, off, seen = hb.real(lib.t_net_sort, 4, m)
    assert rc == 0 and seen["calls"] == 1 and seen["asked"] == seen["bytes"]
    assert seen["bytes"] == 28 * m + 64
    assert off == [0, 8 * m, 16 * m, 8 * (3 * m + 1)]      # sb, (u64*)sb + m, (i64*)sb + 2 m, (i64*)sb + 3 m + 1


@pytest.mark.parametrize("nt", [1, 2, 3])
def test_tile_tables_keep_their_offsets_and_totals_sit_on_8_bytes(lib, nt):
    rc, off, seen = hb.real(lib.t_tiles, 6, nt)
    assert rc == 0 and seen["calls"] == 1 and seen["asked"] == seen["bytes"]
    words = (nt + 1) + 4 * nt + 4 * (nt + 1) + nt + (nt + 1)
    old = 4 * (words + 2) + 8 * 5
    assert old <= seen["bytes"] <= old + 8 * 6
    cnt = 4 * (nt + 1)
    base = cnt + 16 * nt
    kept = base + 16 * (nt + 1)
    totals = 4 * ((words + 1) & ~1)           # tt + ((words + 1) & ~1)
    assert off == [0, cnt, base, kept, kept + 4 * nt, totals] and totals % 8 == 0
    assert totals + 40 <= seen["bytes"]


pytestmark_program = pytest.mark.skipif(hb.plain_compiler() is None, reason="no plain host C++ compiler for a stand-alone program")


def _run_and_check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert r.stdout.splitlines() == ["ok: every array written end to end"]


@pytestmark_program
def test_every_array_written_end_to_end_clean_under_asan_and_ubsan(tmp_path):
    why = hb.sanitizer_missing(tmp_path)
    if why:
        pytest.skip(why)
    _run_and_check(hb.build_program(tmp_path, "scratch_asan", hb.ASAN))


@pytestmark_program
def test_every_array_written_end_to_end_without_the_sanitizer(tmp_path):
    _run_and_check(hb.build_program(tmp_path, "scratch_plain", hb.PLAIN))
