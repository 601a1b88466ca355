"""csrc/inflate.h (the inflater of the peak-file decode kernel) under a host build (tests/hostbuild.py) against zlib: good
streams over the deflate parameter space, every kind of block, and damaged streams -- a status of 0 must mean the output is
the original bytes, nothing is ever written behind `out_cap`, and whatever zlib refuses is refused."""
import zlib

import numpy as np
import pytest

from tests import hostbuild

pytestmark = pytest.mark.skipif(not hostbuild.have_compiler(), reason="no host C++ compiler and no hipcc")

STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.build(tmp_path_factory.mktemp("hostbuild"))


def _inputs(rng):
    """the payload kinds of a peak file and the ones that stress the format"""
    mz = np.sort(rng.uniform(100, 1500, 300))
    return {
        "f64 m/z": mz.astype("<f8").tobytes(),
        "f32 intensity": rng.lognormal(5, 2, 400).astype("<f4").tobytes(),
        "random": rng.integers(0, 256, 700, dtype=np.uint8).tobytes(),
        "text": (b"the quick brown fox jumps over the lazy dog " * 40)[:1500],
        "runs": b"\x00" * 900 + b"ab" * 300 + b"\xff" * 259 + b"x",
        "one byte": b"q",
    }


def _deflate(data, level=6, wbits=15, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """zlib stream of `data`; `flushes` = [(position, flush mode)] inside it"""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    out, last = [], 0
    for pos, mode in flushes:
        out += [c.compress(data[last:pos]), c.flush(mode)]
        last = pos
    out += [c.compress(data[last:]), c.flush()]
    return b"".join(out)


def _check_good(lib, stream, data, what):
    assert zlib.decompress(stream) == data
    st, out, guard = hostbuild.inflate(lib, stream, len(data))
    assert st == 0 and out == data and guard, (what, st)


def test_good_streams_over_levels_strategies_windows(lib):
    rng = np.random.default_rng(1)
    inputs = _inputs(rng)
    n = 0
    for level in (0, 1, 6, 9):
        for strategy in STRATEGIES:
            for wbits in range(9, 16):
                for mem in (1, 8, 9):
                    for name, data in inputs.items():
                        _check_good(lib, _deflate(data, level, wbits, mem, strategy), data, (level, strategy, wbits, mem, name))
                        n += 1
    assert n == 4 * 5 * 7 * 3 * 6


def test_flushes_inside_the_stream(lib):
    rng = np.random.default_rng(2)
    for name, data in _inputs(rng).items():
        if len(data) < 100:
            continue
        third = len(data) // 3
        for modes in ((zlib.Z_SYNC_FLUSH,), (zlib.Z_FULL_FLUSH,), (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH),
                      (zlib.Z_FULL_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH)):
            fl = [(third * (i + 1) // len(modes) * 2, m) for i, m in enumerate(modes)]
            for level in (0, 1, 9):
                for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED):
                    _check_good(lib, _deflate(data, level, 15, 8, strategy, fl), data, (name, modes, level, strategy))
        # a flush at position 0 and two in a row: empty stored blocks
        _check_good(lib, _deflate(data, 6, 15, 8, zlib.Z_DEFAULT_STRATEGY, [(0, zlib.Z_SYNC_FLUSH), (50, zlib.Z_SYNC_FLUSH),
                                                                           (50, zlib.Z_FULL_FLUSH)]), data, name)


def test_empty_large_stored_and_long_runs(lib):
    rng = np.random.default_rng(3)
    for level in (0, 1, 9):
        _check_good(lib, _deflate(b"", level), b"", "empty")
    big = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()          # > 64 KB incompressible: several stored blocks
    s = _deflate(big, 0)
    assert len(s) > len(big) + 3 * 5
    _check_good(lib, s, big, "stored")
    _check_good(lib, _deflate(big, 9), big, "incompressible, level 9")
    for run in (b"\x00" * 300_000, b"\x07" * 258, b"\x07" * 259, b"abc" * 70_000, bytes(range(256)) * 600):
        for level in (1, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_RLE, zlib.Z_FIXED):
                _check_good(lib, _deflate(run, level, 15, 9, strategy), run, (len(run), level, strategy))
    # a window of 512 bytes: distances stay short, many blocks
    _check_good(lib, _deflate(bytes(range(256)) * 600, 9, 9, 1), bytes(range(256)) * 600, "wbits 9")


def _check_damaged(lib, bad, data, what):
    try:
        ref = zlib.decompress(bad)
    except zlib.error:
        ref = None
    st, out, guard = hostbuild.inflate(lib, bad, len(data))
    assert guard, what
    if st == 0:
        assert out == data, what                              # status 0 implies the input's bytes
    if ref is None:
        assert st != 0, what                                  # what zlib refuses is refused
    return st


def _corruption_streams():
    rng = np.random.default_rng(4)
    inp = _inputs(rng)
    return [
        (_deflate(inp["f64 m/z"][:400], 6), inp["f64 m/z"][:400]),                                  # dynamic block
        (_deflate(inp["text"][:300], 6, 15, 8, zlib.Z_FIXED), inp["text"][:300]),                    # fixed block
        (_deflate(inp["random"][:200], 0), inp["random"][:200]),                                     # stored block
        (_deflate(inp["runs"], 9, 9, 1, zlib.Z_RLE), inp["runs"]),                                   # overlapping copies
        (_deflate(inp["f32 intensity"][:600], 1, 12, 4, zlib.Z_FILTERED,
                  [(200, zlib.Z_FULL_FLUSH), (400, zlib.Z_SYNC_FLUSH)]), inp["f32 intensity"][:600]),  # several blocks
    ]


def test_every_single_bit_corruption_of_a_handful_of_streams(lib):
    refused = total = 0
    for stream, data in _corruption_streams():
        _check_good(lib, stream, data, "undamaged")
        for bit in range(8 * len(stream)):
            bad = bytearray(stream)
            bad[bit >> 3] ^= 1 << (bit & 7)
            refused += _check_damaged(lib, bytes(bad), data, (len(stream), bit)) != 0
            total += 1
    assert total > 5000 and refused > 0.95 * total


def test_ten_thousand_random_corruptions(lib):
    rng = np.random.default_rng(5)
    inputs = list(_inputs(rng).values())
    refused = 0
    for k in range(10_000):
        data = inputs[k % len(inputs)]
        stream = bytearray(_deflate(data, int(rng.choice([0, 1, 6, 9])), int(rng.integers(9, 16)), int(rng.integers(1, 10)),
                                    STRATEGIES[int(rng.integers(5))]))
        kind = k % 4
        if kind == 0:                                          # one bit
            bit = int(rng.integers(8 * len(stream)))
            stream[bit >> 3] ^= 1 << (bit & 7)
        elif kind == 1:                                        # a few bits
            for bit in rng.integers(8 * len(stream), size=3):
                stream[int(bit) >> 3] ^= 1 << (int(bit) & 7)
        elif kind == 2:                                        # one byte replaced
            stream[int(rng.integers(len(stream)))] = int(rng.integers(256))
        else:                                                  # bytes dropped from the middle
            at = int(rng.integers(2, len(stream)))
            del stream[at:at + int(rng.integers(1, 4))]
        refused += _check_damaged(lib, bytes(stream), data, (k, kind)) != 0
    assert refused > 9000


def test_truncation_at_every_byte(lib):
    for stream, data in _corruption_streams()[:3]:
        for cut in range(len(stream)):
            st = _check_damaged(lib, stream[:cut], data, cut)
            assert st != 0, cut


def test_capacity_smaller_or_larger_than_the_stream(lib):
    """the declared size bounds the output: one byte less -> refused with nothing written behind it; one more -> refused"""
    for stream, data in _corruption_streams():
        for cap in (0, 1, len(data) - 1, len(data) + 1):
            st, out, guard = hostbuild.inflate(lib, stream, cap)
            assert st != 0 and guard, cap
