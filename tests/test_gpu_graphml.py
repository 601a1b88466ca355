"""The record writer on the GPU (`fal_records_write_sizes`, `fal_records_write`, `Context.format_records`) under the GraphML
file's node and edge tables: the device-written text is byte for byte what `graphml_io.node_units` / `edge_units` -- the host
writer of record -- give for the same blocks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from falcon_amd.ms_io import graphml_io as G
from tests import graphml_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
CASES = [(name, n) for name in K.DEVICE_SETS for n in K.SIZES]


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


_WANT = {}


def case(name, n):
    """-> (blocks, (node units, edge units) of the host writer), computed once"""
    if (name, n) not in _WANT:
        blocks = K.DEVICE_SETS[name](n)
        _WANT[name, n] = (blocks, K.host_units(blocks))
    return _WANT[name, n]


def tables_of(ctx, blocks):
    both, why = G.tables(blocks, ctx, *K.SWITCHES)
    assert why is None
    return both


def _same(got: bytes, want: bytes, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{what}: first difference at byte {at}: {got[max(at - 60, 0):at + 40]!r} != {want[max(at - 60, 0):at + 40]!r}")


# ---- the checks (also run by tests/records_poison_worker.py in a process under FALCON_DEBUG_POISON=1) ------------------------------
def check_case(ctx, name, n, **options):
    blocks, units = case(name, n)
    for which, table, want in zip(("nodes", "edges"), tables_of(ctx, blocks), units):
        assert table["n"] == len(want) == n
        got = b"".join(c.tobytes() for c in ctx.format_records(table, **options))
        _same(got, b"".join(want), (name, n, which))


def check_sizes(ctx, name, n):
    blocks, units = case(name, n)
    for table, want in zip(tables_of(ctx, blocks), units):
        sizes, offsets, total = ctx.records_write_sizes(ctx._records_table(table))
        lens = [len(u) for u in want]
        assert sizes.cpu().tolist() == lens and total == sum(lens)
        assert offsets.cpu().tolist() == [0] + np.cumsum(lens, dtype=np.int64).tolist()


def check_chunking(ctx, name, n):
    blocks, units = case(name, n)
    for table, want in zip(tables_of(ctx, blocks), units):
        chunks = [c.tobytes() for c in ctx.format_records(table, max_bytes=300)]
        assert b"".join(chunks) == b"".join(want)
        lens, sizes = [len(c) for c in chunks], {len(u) for u in want}
        assert len(chunks) > n // 4 and all(k <= 300 or k in sizes for k in lens)           # a chunk above the target is one unit
        assert all(c.endswith(b"\n") for c in chunks)


def check_bounds(ctx):
    """`out` views at every misalignment inside a buffer of sentinels, ranges that begin and end inside tiles and at units longer
    than a tile; a view one byte short: FAL_EINVAL and an untouched buffer"""
    import torch
    from falcon_amd._lib import FAL_EINVAL, FalconHipError
    blocks, units = case("text", 65)
    window = [len(u) for u in units[0][20:30]]
    assert min(window) < 1000 and {K.TILE - 16, K.TILE - 15, K.TILE, K.TILE + 1, 3 * K.TILE + 7} <= set(window) and max(window) > 5 * K.TILE
    for table, want in zip(tables_of(ctx, blocks), units):
        cols = ctx._records_table(table)
        _, offsets, total = ctx.records_write_sizes(cols)
        n = len(want)
        # (units [20, 30) hold short units, units around a tile's size and units of several tiles)
        for front, (first, last) in zip(range(16), [(0, n), (5, 23), (7, 8), (9, 10), (4, 4), (60, n), (21, 22)] + [(20, 30)] * 9):
            text = b"".join(want[first:last])
            buf = torch.full((front + len(text) + 37,), SENTINEL, dtype=torch.uint8, device=ctx.tdev)
            ctx.records_write(cols, offsets, first, last, buf[front:front + len(text)])
            got = buf.cpu().numpy()
            _same(got[front:front + len(text)].tobytes(), text, (front, first, last))
            assert (got[:front] == SENTINEL).all() and (got[front + len(text):] == SENTINEL).all(), (front, first, last)
            if len(text) and front % 3 == 0:
                buf.fill_(SENTINEL)
                with pytest.raises(FalconHipError, match=f"code {FAL_EINVAL}:"):
                    ctx.records_write(cols, offsets, first, last, buf[front:front + len(text) - 1])
                assert (buf.cpu().numpy() == SENTINEL).all()
        wrong = offsets.clone()                                    # offsets that are not the columns': FAL_EINVAL, stores stay inside
        wrong[3:] += 1
        buf = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device=ctx.tdev)
        with pytest.raises(FalconHipError, match=f"code {FAL_EINVAL}:"):
            ctx.records_write(cols, wrong, 0, n, buf[16:16 + total + 1])
        got = buf.cpu().numpy()
        assert (got[:16] == SENTINEL).all() and (got[16 + total + 1:] == SENTINEL).all()


def _small_table():
    ptr = np.array([0, 3, 6, 9], np.int64)
    return dict(n=3, head=b"<", tail=b">\n", fields=[
        dict(kind="text", column=np.frombuffer(b"abc&efghi", np.uint8), ptr=ptr, index=np.array([2, -1, 1], np.int32), prefix=b"[", suffix=b"]"),
        dict(kind="i64", column=np.array([7, -8, 9], np.int64), prefix=b"(", suffix=b")")])


SMALL_TEXT = b"<[ghi](7)>\n<(-8)>\n<[&amp;ef](9)>\n"


def check_bad_arguments(ctx):
    """every bad-argument case of the contract: FAL_EINVAL; a good call behind each still gives the right bytes"""
    from falcon_amd._lib import FAL_EINVAL, REC_MAX_FIELDS, FalconHipError
    good = _small_table()

    def fine():
        assert b"".join(c.tobytes() for c in ctx.format_records(good)) == SMALL_TEXT

    def refused(table=None, cols=None):
        with pytest.raises(FalconHipError, match=f"code {FAL_EINVAL}:"):
            if cols is None:
                list(ctx.format_records(table))
            else:
                ctx.records_write_sizes(cols)
        fine()

    fine()
    text, number = good["fields"]
    with_text = lambda **change: dict(good, fields=[dict(text, **change), number])
    refused(with_text(index=np.array([2, 3, 1], np.int32)))                       # an index at its column's length
    refused(with_text(index=np.array([2, 2 ** 31 - 1, 1], np.int32)))              # and far beyond it
    refused(dict(good, fields=[text, dict(number, index=np.array([0, 1, 3], np.int32))]))
    refused(with_text(ptr=np.array([0, 3, 2, 9], np.int64)))                       # offsets that do not ascend
    refused(with_text(ptr=np.array([0, 3, 6, 10], np.int64)))                      # ... or leave the blob
    refused(with_text(ptr=np.array([-1, 3, 6, 9], np.int64), index=None))
    for c in (0x00, 0x01, 0x08, 0x0B, 0x0C, 0x0E, 0x1F):                           # a byte outside the device grammar
        refused(with_text(column=np.frombuffer(b"abc&efg" + bytes([c]) + b"i", np.uint8)))
    assert b"".join(x.tobytes() for x in ctx.format_records(with_text(column=np.frombuffer(b"abc&ef\t\n\r", np.uint8)))) == \
        SMALL_TEXT.replace(b"ghi", b"\t\n&#13;")
    assert len(list(ctx.format_records(dict(good, fields=[number] * REC_MAX_FIELDS)))) == 1
    refused(dict(good, fields=[number] * (REC_MAX_FIELDS + 1)))                    # more than 32 fields
    for field, name, at, value in ((0, "prefix", 1, 4097), (1, "suffix", 0, -1), (1, "prefix", 1, 10 ** 6), (0, "suffix", 1, None)):
        cols = ctx._records_table(good)                                            # a literal range outside the literal blob
        getattr(cols["fields"][field], name)[at] = cols["literals"].numel() + 1 if value is None else value      # (None: one byte beyond)
        refused(cols=cols)
    cols = ctx._records_table(good)
    cols["head"] = (0, cols["literals"].numel() + 1)
    refused(cols=cols)


def run_all(ctx):
    for name, n in CASES:
        check_case(ctx, name, n)
        check_sizes(ctx, name, n)
    for name in K.DEVICE_SETS:
        check_chunking(ctx, name, 65)
    check_bounds(ctx)
    check_bad_arguments(ctx)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_device_text_equals_the_host_writers(ctx, name, n):
    check_case(ctx, name, n)


@pytest.mark.parametrize("name,n", CASES)
def test_sizes_are_the_units_byte_counts(ctx, name, n):
    check_sizes(ctx, name, n)


@pytest.mark.parametrize("name", list(K.DEVICE_SETS))
def test_chunks_of_a_few_hundred_bytes(ctx, name):
    check_chunking(ctx, name, 65)


def test_write_stays_inside_its_buffer(ctx):
    check_bounds(ctx)


def test_bad_arguments_are_einval_and_leave_the_writer_working(ctx):
    check_bad_arguments(ctx)


def test_a_string_the_device_does_not_mirror_goes_to_the_host_writer(ctx):
    for kind in K.host_only_strings():
        both, why = G.tables(K.host_only(kind), ctx, *K.SWITCHES)
        assert both is None and "name" in why


def test_every_check_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 is read once per process: a fresh child runs every check again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "records_poison_worker.py")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
