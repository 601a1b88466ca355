"""Test-side MS-Numpress encoders (linear, pic, slof), written from the format DESIGN.md "MS-Numpress" states and sharing no code
with the decoders under test, the known answers of that section, seeded inputs that reach every head nibble and both nibble
parities, and a small mzML writer for numpress arrays (cvParam helpers of `peakfile_writer`).
"""
from __future__ import annotations

import base64
import struct
import zlib
from xml.sax.saxutils import quoteattr

import numpy as np

from falcon_amd import _lib
from tests import peakfile_writer as W

LINEAR, PIC, SLOF = _lib.PEAK_NUMPRESS_LINEAR, _lib.PEAK_NUMPRESS_PIC, _lib.PEAK_NUMPRESS_SLOF
COUNTS = (0, 1, 2, 3, 7, 300)

# codec -> (stream, values): the known answers of the format's statement
KNOWN = {
    "pic": (PIC, bytes.fromhex("8717f601ff30a681"), [0.0, 1.0, 15.0, 16.0, -1.0, 100000.0]),
    "pic + 80": (PIC, bytes.fromhex("8717f601ff30a68180"), [0.0, 1.0, 15.0, 16.0, -1.0, 100000.0, 0.0]),
    "linear": (LINEAR, bytes.fromhex("408f400000000000a086010094880100" "6af0"), [100.0, 100.5, 101.25]),
    "slof": (SLOF, bytes.fromhex("408f4000000000000000e803"), [0.0, float(np.e) - 1.0]),
}


def int_nibbles(x: int):
    """one signed 32-bit value -> [head nibble, data nibbles least significant first]"""
    assert -2 ** 31 <= x < 2 ** 31
    u = x & 0xFFFFFFFF
    nibs = [(u >> (4 * i)) & 15 for i in range(8)]                      # least significant first
    fill, limit = (0, 8) if x >= 0 else (15, 7)
    n = 0
    while n < limit and nibs[7 - n] == fill:
        n += 1
    return [n if x >= 0 else n + 8 if n else 0] + nibs[:8 - n]


def pack_nibbles(nibs) -> bytes:
    nibs = list(nibs) + [0] * (len(nibs) & 1)
    return bytes((a << 4) | b for a, b in zip(nibs[0::2], nibs[1::2]))


def encode_ints(values) -> bytes:
    return pack_nibbles([n for x in values for n in int_nibbles(int(x))])


def heads_and_parity(values):
    """-> (set of head nibbles, nibble total mod 2) of the half-byte stream of `values`"""
    per = [int_nibbles(int(x)) for x in values]
    return {p[0] for p in per}, sum(len(p) for p in per) & 1


def encode_pic(ints) -> bytes:
    return encode_ints(ints)


def encode_linear_ints(y, fp: float) -> bytes:
    """the integers y (each of y0, y1 and every second difference within int32) -> a linear stream"""
    y = [int(v) for v in y]
    out = struct.pack(">d", fp)
    if y:
        out += struct.pack("<i", y[0])
    if len(y) > 1:
        out += struct.pack("<i", y[1])
    return out + encode_ints(y[i] - (2 * y[i - 1] - y[i - 2]) for i in range(2, len(y)))


def linear_ints(values, fp: float):
    return np.rint(np.asarray(values, np.float64) * fp).astype(np.int64)


def slof_ints(values, fp: float):
    return np.clip(np.rint(np.log(np.asarray(values, np.float64) + 1.0) * fp), 0, 65535).astype(np.int64)


def encode_slof_ints(u, fp: float) -> bytes:
    return struct.pack(">d", fp) + np.asarray(u).astype("<u2").tobytes()


def slof_values(u, fp: float):
    """what a slof decoder returns for the integers u, by the format's formula in numpy"""
    return np.exp(np.asarray(u, np.float64) / fp) - 1.0


def mz_cases(count: int, seed: int):
    """name -> (fp, y int64[count]): m/z-like integers of a linear stream: ascending, descending and shuffled (negative
    differences), a fixed point at which second differences need all 8 nibbles, zeros, -1, and jumps of 2^29"""
    rng = np.random.default_rng(seed)
    mz = np.sort(rng.uniform(100.0, 2000.0, count))
    wide = rng.integers(-2 ** 29, 2 ** 29, count)                       # second differences up to 2^31: heads 0 and 1
    edge = np.resize(np.array([0, -1, 0, 0, 1, -1, -1, 2 ** 29, -2 ** 29, 0, 15, 16, -16, -17, 255, -256]), count)
    return {"ascending": (1000.0, linear_ints(mz, 1000.0)), "descending": (1000.0, linear_ints(mz[::-1], 1000.0)),
            "shuffled": (1000.0, linear_ints(rng.permutation(mz), 1000.0)),
            "fine": (100000.0, linear_ints(rng.permutation(mz), 100000.0)), "wide": (3.5, wide), "edge": (1.0, edge),
            "zeros": (21.0, np.zeros(count, np.int64)), "minus one": (0.125, np.full(count, -1, np.int64))}


def int_cases(count: int, seed: int):
    """name -> int64[count] for pic: magnitudes of every nibble length and both signs, zeros, -1, the int32 limits"""
    rng = np.random.default_rng(seed)
    mags = rng.integers(0, 2 ** rng.integers(0, 32, count), dtype=np.int64) if count else np.zeros(0, np.int64)
    limits = np.resize(np.array([2 ** 31 - 1, -2 ** 31, 0, -1, 1, 15, 16, -16, -17, 2 ** 27, -2 ** 27 - 1, 2 ** 28 - 1, -2 ** 28]),
                       count)
    return {"positive": mags, "mixed": mags * rng.choice([-1, 1], count), "limits": limits,
            "counts": rng.integers(0, 5000, count), "zeros": np.zeros(count, np.int64), "minus one": np.full(count, -1, np.int64)}


def encoded_spectra(n, seed, plans):
    """n seeded spectra encoded by `plans[i % len]` = (m/z codec, zlib?, intensity codec, zlib?) -> (writer dicts, the values
    a decoder returns)"""
    rng = np.random.default_rng(seed)
    spectra, want = [], []
    for i in range(n):
        mc, mzl, ic, izl = plans[i % len(plans)]
        k = int(rng.integers(0, 40))
        mz = np.sort(rng.uniform(100.0, 1500.0, k))
        if i % 5 == 0:
            mz = rng.permutation(mz)
        if mc == LINEAR:
            y = linear_ints(mz, 10000.0)
            m_stream, m_val = encode_linear_ints(y, 10000.0), y.astype(np.float64) / 10000.0
        else:
            y = np.rint(mz).astype(np.int64)
            m_stream, m_val = encode_pic(y), y.astype(np.float64)
        it = rng.uniform(1.0, 1e4, k)
        if ic == PIC:
            v = np.rint(it).astype(np.int64)
            i_stream, i_val = encode_pic(v), v.astype(np.float32)
        elif ic == SLOF:
            u = slof_ints(it, 3000.0)
            i_stream, i_val = encode_slof_ints(u, 3000.0), slof_values(u, 3000.0).astype(np.float32)
        else:
            v = linear_ints(it, 100.0)
            i_stream, i_val = encode_linear_ints(v, 100.0), (v.astype(np.float64) / 100.0).astype(np.float32)
        spectra.append({"identifier": f"scan={i + 1}", "precursor_mz": float(rng.uniform(400.0, 1200.0)),
                        "precursor_charge": int(rng.integers(1, 4)) if i % 7 else None,
                        "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)),
                        "mz": (mc, m_stream, mzl, k), "intensity": (ic, i_stream, izl, k)})
        want.append((m_val, i_val))
    return spectra, want


PLANS = [(LINEAR, False, PIC, False), (LINEAR, True, SLOF, True), (PIC, False, LINEAR, True),
         (PIC, True, SLOF, False), (LINEAR, True, PIC, True), (LINEAR, False, LINEAR, False)]



def _text(stream: bytes, compress: bool) -> str:
    return base64.b64encode(zlib.compress(stream, 6) if compress else stream).decode("ascii")


_TERMS = {LINEAR: ("MS:1002312", "MS:1002746", "MS-Numpress linear prediction compression"),
          PIC: ("MS:1002313", "MS:1002747", "MS-Numpress positive integer compression"),
          SLOF: ("MS:1002314", "MS:1002748", "MS-Numpress short logged float compression")}


def array_params(codec: int, compress: bool, kind: str, extra: str = "") -> str:
    """the cvParams of one numpress binaryDataArray: a float-width term (ignored by readers), the plain or the zlib-combined
    numpress term, the array kind"""
    plain, combined, name = _TERMS[codec]
    what = ("MS:1000514", "m/z array") if kind == "mz" else ("MS:1000515", "intensity array")
    return (W._cv("MS:1000523", "64-bit float") + W._cv(combined if compress else plain, name + (" followed by zlib" if compress else ""))
            + extra + W._cv(*what))


def write_mzml(path, spectra, extra_params=None):
    """spectra: dicts with the fields of `peakfile_writer` except the peaks, which come as `mz` / `intensity` = (codec, stream,
    zlib?, count).  `extra_params`: identifier -> cvParam text added to the m/z array (contradictory terms)."""
    parts = ['<?xml version="1.0" encoding="utf-8"?>\n<mzML xmlns="http://psi.hupo.org/ms/mzml" version="1.1.0">\n'
             '<run id="r"><spectrumList count="%d">\n' % len(spectra)]
    for idx, s in enumerate(spectra):
        ch = s.get("precursor_charge")
        out = [f'<spectrum index="{idx}" id={quoteattr(s["identifier"])} defaultArrayLength="{s["mz"][3]}">'
               f'{W._cv("MS:1000511", "ms level", 2)}<scanList count="1"><scan>'
               f'{W._cv("MS:1000016", "scan start time", s["retention_time"])}</scan></scanList>'
               '<precursorList count="1"><precursor><selectedIonList count="1"><selectedIon>'
               f'{W._cv("MS:1000744", "selected ion m/z", repr(float(s["precursor_mz"])))}'
               f'{W._cv("MS:1000041", "charge state", ch) if ch is not None else ""}'
               '</selectedIon></selectedIonList></precursor></precursorList><binaryDataArrayList count="2">']
        for kind in ("mz", "intensity"):
            codec, stream, compress, _ = s[kind]
            txt = _text(stream, compress)
            extra = (extra_params or {}).get(s["identifier"], "") if kind == "mz" else ""
            out.append(f'<binaryDataArray encodedLength="{len(txt)}">{array_params(codec, compress, kind, extra)}\n'
                       f'<binary>{txt}</binary></binaryDataArray>')
        out.append('</binaryDataArrayList></spectrum>\n')
        parts.append("".join(out))
    parts.append('</spectrumList></run></mzML>\n')
    with open(path, "w") as f:
        f.write("".join(parts))
