"""MS-Numpress decoders on the host (numpy): linear (MS:1002312), pic (MS:1002313) and slof (MS:1002314).

A stream is the bytes of one mzML binary array after base64 (and after zlib, for the combined terms MS:1002746-8); the decoded
values are float64.  DESIGN.md "MS-Numpress" states the format, written from the published description of MS-Numpress (Teleman et
al., MCP 2014); parity with outside encoders is UNPINNED (no pynumpress / pyteomics and no real file to compare with).  This is
what `PeakChunk.host_values` (the public `get_spectra` path) decodes with, and the oracle of the device decoder
(`csrc/numpress.h`, the numpress stage of `fal_decode_peaks`): linear and pic agree bit for bit, slof to the last bits of `exp`.

  half-byte integer   a signed 32-bit value as a head nibble h and data nibbles: its h (h <= 8) most significant nibbles are 0, or
                      its h - 8 (h > 8) most significant are 0xF; the other nibbles follow, least significant first.  Nibbles are
                      packed high nibble first; a stream of an odd number of nibbles ends with a low nibble of 0.
  pic                 every value one half-byte integer
  linear              fixed point fp (float64, big-endian), y0, y1 (int32, little-endian), then half-byte second differences:
                      y_i = 2 y_{i-1} - y_{i-2} + d_i in wrapping int64; value = y_i / fp
  slof                fp, then one little-endian uint16 u per value: exp(u / fp) - 1

Every error (a bad header length, a fixed point that is not finite and > 0, a stream that ends inside a value) is a ValueError.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from .._lib import PEAK_NUMPRESS_LINEAR, PEAK_NUMPRESS_PIC, PEAK_NUMPRESS_SLOF

_SHIFTS = 4 * np.arange(8, dtype=np.uint64)


def _half_byte_ints(data: bytes) -> np.ndarray:
    """the half-byte integers of a stream -> int64[] (each within int32)"""
    b = np.frombuffer(data, np.uint8)
    n_nib = 2 * len(b)
    if not n_nib:
        return np.zeros(0, np.int64)
    nib = np.empty(n_nib, np.uint8)
    nib[0::2], nib[1::2] = b >> 4, b & 15
    fill = np.where(nib <= 8, nib, nib - 8).astype(np.int64)            # nibbles a head at that position declares filled
    step = (9 - fill).tolist()                                          # head + data nibbles
    stop = n_nib - 1 if nib[-1] == 0 else n_nib                         # the padding nibble ends the stream
    heads, p = [], 0
    while p < n_nib and p != stop:
        q = p + step[p]
        if q > n_nib:
            raise ValueError("MS-Numpress stream ends inside a value")
        heads.append(p)
        p = q
    heads = np.array(heads, np.int64)
    m = 8 - fill[heads]                                                 # data nibbles per value
    k = np.arange(8)
    idx = np.minimum(heads[:, None] + 1 + k[None, :], n_nib - 1)
    d = np.where(k[None, :] < m[:, None], nib[idx], 0).astype(np.uint64)
    v = (d << _SHIFTS[None, :]).sum(axis=1, dtype=np.uint64)
    ones = (np.uint64(0xFFFFFFFF) << (4 * m).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    v = np.where(nib[heads] > 8, v | ones, v)
    return v.astype(np.uint32).view(np.int32).astype(np.int64)


def _fixed_point(data: bytes) -> float:
    (fp,) = struct.unpack(">d", data[:8])
    if not (math.isfinite(fp) and fp > 0):
        raise ValueError(f"MS-Numpress fixed point {fp!r}")
    return fp


def decode_pic(data: bytes) -> np.ndarray:
    return _half_byte_ints(data).astype(np.float64)


def linear_integers(data: bytes):
    """-> (fp, y int64[]): the fixed point and the integers of a linear stream (value = y / fp)"""
    n = len(data)
    if n < 8 or 8 < n < 12 or 12 < n < 16:
        raise ValueError(f"MS-Numpress linear stream of {n} bytes")
    fp = _fixed_point(data)
    y = np.frombuffer(data[8:min(n, 16)], "<i4").astype(np.int64)
    if n > 16:
        d = _half_byte_ints(data[16:])
        with np.errstate(over="ignore"):
            # the recurrence as two wrapping prefix sums: first differences, then values
            e = (y[1] - y[0]) + np.cumsum(d, dtype=np.int64)
            y = np.concatenate([y, y[1] + np.cumsum(e, dtype=np.int64)])
    return fp, y


def decode_linear(data: bytes) -> np.ndarray:
    fp, y = linear_integers(data)
    return y.astype(np.float64) / fp


def decode_slof(data: bytes) -> np.ndarray:
    n = len(data)
    if n < 8 or (n - 8) % 2:
        raise ValueError(f"MS-Numpress slof stream of {n} bytes")
    fp = _fixed_point(data)
    with np.errstate(over="ignore"):                                    # a tiny fixed point: inf, as the formula gives
        return np.exp(np.frombuffer(data[8:], "<u2").astype(np.float64) / fp) - 1.0


_DECODERS = {PEAK_NUMPRESS_LINEAR: decode_linear, PEAK_NUMPRESS_PIC: decode_pic, PEAK_NUMPRESS_SLOF: decode_slof}


def decode(codec: int, data: bytes) -> np.ndarray:
    """one stream of the codec `codec` (a `_lib.PEAK_NUMPRESS_*` value) -> float64[]"""
    return _DECODERS[codec](data)
