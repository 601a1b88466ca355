"""What the mzML and mzXML readers share: spectra as metadata plus payload descriptors.

A reader streams its XML file and keeps, per MS2+ spectrum, the identifier, precursor m/z, charge and retention time, and for
every binary array its base64 text appended to one contiguous byte buffer plus a descriptor row (offset, base64 length, declared
value count, `_lib.PEAK_*` flags).  That is the input of the device decoder (`Context.decode_peaks`, `fal_decode_peaks`); the
host decode below reads the same descriptors and is the public `get_spectra` path (and the tests' oracle of the device decode).
"""
from __future__ import annotations

import base64
import binascii
import collections
import zlib
from typing import Dict, Iterator, List, Optional

import numpy as np

from .._lib import PEAK_BIG_ENDIAN, PEAK_F64, PEAK_NUMPRESS_MASK, PEAK_PAIRS, PEAK_ZLIB
from . import numpress

# a chunk's payload is closed once it holds this many base64 bytes (one device call decodes one chunk)
DEFAULT_CHUNK_BYTES = 1 << 30


class PeakChunk:
    """MS2+ spectra of one peak file (or of one byte-bounded part of it), in file order."""

    def __init__(self):
        self.identifier: List[str] = []
        self.precursor_mz: List[float] = []
        self.precursor_charge: List[Optional[int]] = []
        self.retention_time: List[float] = []
        self._spectra: List[tuple] = []
        self._arrays: List[tuple] = []
        self._buf = bytearray()
        self.skipped = collections.Counter()        # reason -> spectra the reader dropped for a reason outside the file's fault

    def __len__(self):
        return len(self.identifier)

    @property
    def nbytes(self) -> int:
        return len(self._buf)

    def add_array(self, b64: bytes, count: int, flags: int) -> int:
        """append one array's base64 text (8-byte aligned) -> its row in the descriptor table"""
        self._buf.extend(b"\0" * (-len(self._buf) % 8))
        self._arrays.append((len(self._buf), len(b64), int(count), int(flags)))
        self._buf.extend(b64)
        return len(self._arrays) - 1

    def add_spectrum(self, identifier: str, precursor_mz: float, charge: Optional[int], rt: float, mz_array: int,
                     intensity_array: int) -> None:
        self.identifier.append(identifier)
        self.precursor_mz.append(precursor_mz)
        self.precursor_charge.append(charge)
        self.retention_time.append(rt)
        self._spectra.append((mz_array, intensity_array))

    def tables(self):
        """-> payload u8[], arrays i64[m, 4], spectra i64[n, 2]: the arguments of `Context.decode_peaks`"""
        return (np.frombuffer(self._buf, np.uint8) if self._buf else np.zeros(0, np.uint8),
                np.array(self._arrays, np.int64).reshape(-1, 4), np.array(self._spectra, np.int64).reshape(-1, 2))

    def host_values(self, row: int) -> np.ndarray:
        """one array decoded on the host with the stdlib (base64, zlib): its values in their stored precision; an MS-Numpress
        array (base64, zlib if flagged, then the codec of `numpress`) as float64.
        Raises ValueError on bad base64, a bad zlib or numpress stream or a value count other than the declared one."""
        off, ln, count, flags = self._arrays[row]
        try:
            raw = base64.b64decode(bytes(self._buf[off:off + ln]), validate=True)
            if flags & PEAK_ZLIB:
                raw = zlib.decompress(raw)
        except (binascii.Error, zlib.error) as e:
            raise ValueError(str(e)) from e
        if flags & PEAK_NUMPRESS_MASK:
            if flags & (PEAK_F64 | PEAK_BIG_ENDIAN | PEAK_PAIRS):
                raise ValueError("MS-Numpress together with a float width, byte order or pair flag")
            v = numpress.decode(flags & PEAK_NUMPRESS_MASK, raw)
            if len(v) != count:
                raise ValueError(f"{len(v)} MS-Numpress values for {count} declared values")
            return v
        dt = np.dtype(np.float64 if flags & PEAK_F64 else np.float32).newbyteorder(">" if flags & PEAK_BIG_ENDIAN else "<")
        per = 2 if flags & PEAK_PAIRS else 1
        if len(raw) != count * per * dt.itemsize:
            raise ValueError(f"{len(raw)} bytes for {count} declared values")
        return np.frombuffer(raw, dt).astype(dt.newbyteorder("="))

    def host_spectra(self) -> Iterator[Dict]:
        """the chunk's spectra as `mgf_io.get_spectra` dicts, arrays decoded on the host; a spectrum whose arrays do not decode
        is skipped and counted in `skipped`"""
        for i, (ma, ia) in enumerate(self._spectra):
            try:
                if ma == ia:                                            # interleaved m/z-intensity pairs (mzXML)
                    v = self.host_values(ma)
                    mz, it = v[0::2], v[1::2]
                else:
                    mz, it = self.host_values(ma), self.host_values(ia)
                    if len(mz) != len(it):
                        raise ValueError("m/z and intensity arrays differ in length")
            except ValueError as e:
                self.skipped[f"undecodable binary array ({e})"] += 1
                continue
            yield {"identifier": self.identifier[i], "precursor_mz": self.precursor_mz[i],
                   "precursor_charge": self.precursor_charge[i], "retention_time": self.retention_time[i],
                   "mz": mz.astype(np.float64), "intensity": it.astype(np.float32)}
