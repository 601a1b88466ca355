"""mzML reading without pyteomics / lxml (both absent): a streaming stdlib ElementTree pass.

Fields as the reference reads them (falcon/ms_io/mzml_io.py:14-80, pyteomics underneath): spectra with `ms level` (MS:1000511)
> 1; identifier = `spectrum/@id`; precursor m/z = first precursor -> first selectedIon -> MS:1000744; charge = MS:1000041, else
the first MS:1000633, else None; retention time = the first scan's MS:1000016 value as written (its unit is not applied, as the
reference passes pyteomics' value through; PARITY UNPINNED), -1 when absent.  Parameters may come through
`referenceableParamGroupRef` at every level.  A spectrum that lacks a required field is skipped silently, as the reference's
`except (ValueError, KeyError)` does; one with arrays this build does not decode (the MS-Numpress truncation terms
MS:1003089-91, contradictory compression terms) is skipped and counted in `PeakChunk.skipped`.  A parse error part-way logs a
warning and keeps the spectra read before it.

MS-Numpress arrays are read: linear, pic and slof (MS:1002312-4), and the same followed by zlib (MS:1002746-8); the float-width
term of such an array is ignored, its values are float64 (`numpress.py`, DESIGN.md "MS-Numpress"; parity with outside encoders
UNPINNED).  A numpress term next to a second compression term (MS:1000574 zlib or MS:1000576 none) is contradictory and the
spectrum is skipped under the codec's name -- so older files that mark numpress + zlib with two separate terms stay skipped.

Elements are dropped once used, so memory follows the chunk's payload, not the file.  The binary arrays stay base64 text here:
`PeakChunk` carries them to the device decoder (`fal_decode_peaks`) or decodes them on the host (`get_spectra`).

`read_chunks_device` is the same reader with the structure of the spectra scanned on the device (`fal_mzml_index` +
`fal_mzml_parse`, DESIGN.md "mzML on the device"): `read_chunks` / `_spectrum` stay the reader of record for the header, for every
spectrum and every file outside the device's byte grammar, and the oracle of that path.
"""
from __future__ import annotations

import logging
import re
import xml.etree.ElementTree as ET
from typing import Dict, Iterator

import numpy as np

from .._lib import PEAK_F64, PEAK_NUMPRESS_LINEAR, PEAK_NUMPRESS_PIC, PEAK_NUMPRESS_SLOF, PEAK_ZLIB
from .peak_payload import DEFAULT_CHUNK_BYTES, PeakChunk

logger = logging.getLogger("falcon")

MS_LEVEL, SCAN_START, SELECTED_MZ, CHARGE, POSSIBLE_CHARGE = "MS:1000511", "MS:1000016", "MS:1000744", "MS:1000041", "MS:1000633"
MZ_ARRAY, INTENSITY_ARRAY = "MS:1000514", "MS:1000515"
FLOAT32, FLOAT64 = "MS:1000521", "MS:1000523"
NO_COMPRESSION, ZLIB = "MS:1000576", "MS:1000574"
NUMPRESS = {"MS:1002312": "MS-Numpress linear", "MS:1002313": "MS-Numpress pic", "MS:1002314": "MS-Numpress slof"}
# accession -> array flags: the plain numpress terms, and the terms for numpress followed by zlib
_NUMPRESS_FLAGS = {"MS:1002312": PEAK_NUMPRESS_LINEAR, "MS:1002313": PEAK_NUMPRESS_PIC, "MS:1002314": PEAK_NUMPRESS_SLOF,
                   "MS:1002746": PEAK_NUMPRESS_LINEAR | PEAK_ZLIB, "MS:1002747": PEAK_NUMPRESS_PIC | PEAK_ZLIB,
                   "MS:1002748": PEAK_NUMPRESS_SLOF | PEAK_ZLIB}
_NUMPRESS_NAME = dict(NUMPRESS, **{"MS:1002746": NUMPRESS["MS:1002312"], "MS:1002747": NUMPRESS["MS:1002313"],
                                   "MS:1002748": NUMPRESS["MS:1002314"]})     # the skip reason names the codec
# every other compression term of the PSI-MS vocabulary (numpress with truncation): MS:1000572 is "binary data compression type"
_COMPRESSION_TERMS = {"MS:1003089", "MS:1003090", "MS:1003091"}


def _local(tag: str) -> str:
    return tag.rpartition("}")[2]


def _children(el, name):
    return [c for c in el if _local(c.tag) == name]


def _first(el, name):
    for c in el:
        if _local(c.tag) == name:
            return c
    raise KeyError(name)


def _params(el, groups) -> Dict[str, str]:
    """accession -> value of the cvParams of `el`, referenced groups included; the first occurrence of an accession wins"""
    out: Dict[str, str] = {}
    for c in el:
        t = _local(c.tag)
        if t == "cvParam":
            out.setdefault(c.get("accession"), c.get("value"))
        elif t == "referenceableParamGroupRef":
            for acc, val in groups.get(c.get("ref"), ()):
                out.setdefault(acc, val)
    return out


class _Unsupported(Exception):
    pass


def _array(chunk: PeakChunk, bda, groups, default_count: int):
    """one binaryDataArray -> (kind accession or None, descriptor row)"""
    p = _params(bda, groups)
    kind = MZ_ARRAY if MZ_ARRAY in p else INTENSITY_ARRAY if INTENSITY_ARRAY in p else None
    if kind is None:
        return None, -1
    codecs = [acc for acc in _NUMPRESS_FLAGS if acc in p]
    others = [acc for acc in (ZLIB, NO_COMPRESSION, *sorted(_COMPRESSION_TERMS)) if acc in p]
    if codecs and (len(codecs) > 1 or others):                          # contradictory compression terms
        raise _Unsupported(_NUMPRESS_NAME[codecs[0]])
    if others and others[-1] in _COMPRESSION_TERMS:
        raise _Unsupported("unsupported compression")
    if codecs:
        flags = _NUMPRESS_FLAGS[codecs[0]]                              # float64 values whatever the float-width term says
    else:
        flags = PEAK_ZLIB if ZLIB in p else 0
        if FLOAT64 in p:
            flags |= PEAK_F64
        elif FLOAT32 not in p:
            raise _Unsupported("unsupported binary data type")
    count = int(bda.get("arrayLength", default_count))
    text = _first(bda, "binary").text or ""
    return kind, chunk.add_array("".join(text.split()).encode("ascii"), count, flags)


def _spectrum(chunk: PeakChunk, sp, groups) -> None:
    p = _params(sp, groups)
    try:
        if MS_LEVEL not in p or int(p[MS_LEVEL]) <= 1:                  # MS1 (or no level): arrays never touched
            return
        ident = sp.attrib["id"]
        scan = _first(_first(sp, "scanList"), "scan")
        rt = float(_params(scan, groups).get(SCAN_START, -1))
        ion = _first(_first(_first(_first(sp, "precursorList"), "precursor"), "selectedIonList"), "selectedIon")
        ip = _params(ion, groups)
        pmz = float(ip[SELECTED_MZ])
        charge = int(float(ip[CHARGE])) if CHARGE in ip else int(float(ip[POSSIBLE_CHARGE])) if POSSIBLE_CHARGE in ip else None
        default_count = int(sp.get("defaultArrayLength", 0))
        rows = {}
        for bda in _children(_first(sp, "binaryDataArrayList"), "binaryDataArray"):
            kind, row = _array(chunk, bda, groups, default_count)
            if kind is not None:
                rows.setdefault(kind, row)
        chunk.add_spectrum(ident, pmz, charge, rt, rows[MZ_ARRAY], rows[INTENSITY_ARRAY])
    except _Unsupported as e:
        chunk.skipped[str(e)] += 1
    except (ValueError, KeyError, TypeError):
        pass


def _iterparse_chunks(source, filename: str, max_bytes: int) -> Iterator[PeakChunk]:
    """`read_chunks` over `source`, a file name or an object with read(); `filename` is the name the warning gives"""
    groups: Dict[str, list] = {}
    chunk = PeakChunk()
    stack = []
    keep = 0                  # open elements whose subtree is still needed (spectrum, referenceableParamGroup)
    try:
        for ev, el in ET.iterparse(source, events=("start", "end")):
            tag = _local(el.tag)
            if ev == "start":
                stack.append(el)
                keep += tag in ("spectrum", "referenceableParamGroup")
                continue
            stack.pop()
            if tag == "referenceableParamGroup":
                groups[el.get("id")] = [(c.get("accession"), c.get("value")) for c in el if _local(c.tag) == "cvParam"]
                keep -= 1
            elif tag == "spectrum":
                keep -= 1
                _spectrum(chunk, el, groups)
                if chunk.nbytes >= max_bytes:
                    yield chunk
                    chunk = PeakChunk()
            elif keep:
                continue
            if stack:
                stack[-1].remove(el)                                    # used: drop it (the parent holds nothing else)
    except ET.ParseError as e:
        logger.warning("Failed to read file %s: %s", filename, e)
    yield chunk


def read_chunks(filename: str, max_bytes: int = DEFAULT_CHUNK_BYTES) -> Iterator[PeakChunk]:
    """stream an mzML (or indexedmzML) file -> PeakChunks of at most about `max_bytes` of base64 payload each"""
    yield from _iterparse_chunks(filename, filename, max_bytes)


# ---- the device reader (DESIGN.md "mzML on the device") ---------------------------------------------------------------------------
DEVICE_CHUNK_BYTES = 64 << 20        # text of one device call (the tag table takes 7 bytes per text byte)
_HEADER_READ = 1 << 20
_SPECTRUM_OPEN = re.compile(rb"<spectrum[ \t\r\n>/]")
_DECLARATION = re.compile(rb"^(?:\xef\xbb\xbf)?<\?xml([^>]*)\?>")
_ENCODING = re.compile(rb"encoding\s*=\s*[\"']([^\"']*)[\"']")
_CLOSE = b"</spectrum>"


class DeviceChunk:
    """The MS2+ spectra of one stretch of an mzML file, in file order, with `PeakChunk`'s surface: the columns, `skipped`, and
    `tables()` whose payload stays where the device reader left it (a device tensor).  `n_device` / `n_host`: the spectra the
    device decided (kept or MS1) and the ones handed to the host reader."""

    def __init__(self, identifier, precursor_mz, precursor_charge, retention_time, payload, arrays, spectra, skipped, n_device, n_host):
        self.identifier, self.precursor_mz, self.precursor_charge = identifier, precursor_mz, precursor_charge
        self.retention_time, self.skipped, self.n_device, self.n_host = retention_time, skipped, n_device, n_host
        self._tables = (payload, arrays, spectra)

    def __len__(self):
        return len(self.identifier)

    @property
    def nbytes(self) -> int:
        return int(len(self._tables[0]))

    def tables(self):
        """-> payload u8[] (device tensor), arrays i64[m, 4], spectra i64[n, 2]: the arguments of `Context.decode_peaks`"""
        return self._tables


def _device_encoding(head: bytes) -> bool:
    """the XML declaration names no encoding, or UTF-8 / US-ASCII: the bytes the device grammar takes mean what they say"""
    m = _DECLARATION.match(head)
    if m is None:
        return not head.startswith((b"\xff\xfe", b"\xfe\xff"))            # (UTF-16 needs no declaration)
    enc = _ENCODING.search(m.group(1))
    return enc is None or enc.group(1).lower() in (b"utf-8", b"us-ascii")


def _header_groups(header: bytes):
    """the referenceableParamGroups of everything in front of the first spectrum -> `groups` as `read_chunks` builds it; None
    when the header does not parse"""
    groups: Dict[str, list] = {}
    parser = ET.XMLPullParser(events=("end",))
    try:
        parser.feed(header)
        for _, el in parser.read_events():
            if _local(el.tag) == "referenceableParamGroup":
                groups[el.get("id")] = [(c.get("accession"), c.get("value")) for c in el if _local(c.tag) == "cvParam"]
    except ET.ParseError:
        return None
    return groups


class _Chain:
    """read() over byte strings and then an open file: what `ET.iterparse` needs of a source"""

    def __init__(self, parts, f):
        self.parts, self.f = [memoryview(p) for p in parts if len(p)], f

    def read(self, size: int = -1) -> bytes:
        if self.parts:
            if size < 0:
                out = b"".join(self.parts) + self.f.read()
                self.parts = []
                return out
            out = bytes(self.parts[0][:size])
            self.parts[0] = self.parts[0][size:]
            if not len(self.parts[0]):
                self.parts.pop(0)
            return out
        return self.f.read(size)


def _join_payload(payload, used: int, more: np.ndarray):
    """payload[:used] (a device tensor or a host array) with the host bytes `more` behind it"""
    if not len(more):
        return payload[:used]
    if isinstance(payload, np.ndarray):
        return np.concatenate([payload[:used], more])
    import torch
    return torch.cat([payload[:used], torch.from_numpy(more.copy()).to(payload.device)])


def _device_chunk(head, res, groups, filename: str):
    """one scanned stretch -> (DeviceChunk, stopped): the device's OK spectra, every HOST spectrum read by `_spectrum` from
    its own bytes and put at its place in file order, SKIP and host-rejected spectra removed.  stopped: a HOST spectrum did not
    parse -- the host reader's pass ends there with a warning, and so does this one."""
    from .._lib import MZML_ST_HOST, MZML_ST_OK
    from .mgf_io import _identifiers
    status = res["status"]
    n = len(status)
    host = PeakChunk()
    keep = status == MZML_ST_OK
    host_rows = np.flatnonzero(status == MZML_ST_HOST)
    stopped = False
    for i in host_rows:
        a, b = res["span"][i]
        try:
            el = ET.fromstring(bytes(head[a:b]))
        except ET.ParseError as e:
            logger.warning("Failed to read file %s: %s", filename, e)
            keep[i:] = False
            stopped = True
            break
        before = len(host)
        _spectrum(host, el, groups)
        keep[i] = len(host) > before
    rows = np.flatnonzero(keep)
    from_host = status[rows] == MZML_ST_HOST
    text = np.frombuffer(head, np.uint8)
    ident = _identifiers(text, res["id"][rows])
    pmz, rt = res["precursor_mz"][rows].copy(), res["retention_time"][rows].copy()
    charge = res["charge"][rows].astype(object)
    charge[res["charge"][rows] == 0] = None
    arrays = res["arrays"].reshape(n, 2, 4).copy()
    arrays[status != MZML_ST_OK] = 0
    arrays = arrays.reshape(2 * n, 4)
    used = int((arrays[:, 0] + (arrays[:, 1] + 7) // 8 * 8).max(initial=0))
    spectra = np.stack([2 * rows, 2 * rows + 1], axis=1).astype(np.int64)
    more = np.zeros(0, np.uint8)
    if len(host):
        more, host_arrays, host_spectra = host.tables()
        host_arrays = host_arrays.copy()
        host_arrays[:, 0] += used
        arrays = np.concatenate([arrays, host_arrays])
        spectra[from_host] = host_spectra + 2 * n
        ident = ident.astype(object)
        ident[from_host] = host.identifier
        ident = np.array(list(ident), dtype=str)
        pmz[from_host], rt[from_host] = host.precursor_mz, host.retention_time
        charge[from_host] = host.precursor_charge
    chunk = DeviceChunk(ident, pmz, list(charge), rt, _join_payload(res["payload"], used, more), arrays, spectra, host.skipped,
                        n - len(host_rows), len(host_rows))
    return chunk, stopped


def read_chunks_device(filename: str, ctx, max_bytes: int = DEVICE_CHUNK_BYTES):
    """The device reader: everything in front of the first <spectrum ...> stays on the host (its param groups are read with
    ElementTree); the rest is cut directly behind </spectrum> into stretches of about `max_bytes` (a stretch grows when one
    spectrum is larger), each scanned by `ctx.scan_mzml`; spectra with status HOST are read by `_spectrum` from their own
    bytes.  A stretch outside the device grammar, and whatever follows the file's last </spectrum>, goes through the host
    reader's own pass over the header plus the remaining bytes -- a well-formed prefix, at the same line and column, so a
    truncated file gives `read_chunks`' warning and spectra.  A declared encoding other than UTF-8 / US-ASCII, a DOCTYPE, a
    first <spectrum inside a comment or CDATA section, a header that does not parse or a file without spectra is `read_chunks`' as a whole.
    Yields `DeviceChunk`s (and `PeakChunk`s from the host pass); all chunks together are `read_chunks(filename)`'s."""
    with open(filename, "rb") as f:
        buf = bytearray(f.read(_HEADER_READ))
        m, final = None, False
        if _device_encoding(bytes(buf[:4096])):
            searched = 0
            while True:
                m = _SPECTRUM_OPEN.search(buf, max(searched - 16, 0))
                if m is not None or final:
                    break
                searched = len(buf)
                more = f.read(_HEADER_READ)
                final = len(more) == 0
                buf += more
        header = bytes(buf[:m.start()]) if m is not None else b""
        # a DOCTYPE may define entities; behind an open comment or CDATA section the match is no tag
        plain = (m is not None and b"<!DOCTYPE" not in header and header.rfind(b"<!--") <= header.rfind(b"-->") and
                 header.rfind(b"<![CDATA[") <= header.rfind(b"]]>"))
        groups = _header_groups(header) if plain else None
        if groups is None:
            yield from read_chunks(filename)
            return
        del buf[:len(header)]
        lines, column = 0, 0          # of the bytes consumed behind the header: the host pass sees as many line breaks and columns
        final = False
        while True:
            if not final and len(buf) < max_bytes:
                more = f.read(max(max_bytes - len(buf), 1 << 16))
                final = len(more) == 0
                buf += more
                continue
            cut = buf.rfind(_CLOSE, 0, max(max_bytes, len(_CLOSE)))
            if cut < 0:
                cut = buf.find(_CLOSE)             # one spectrum larger than the stretch
            if cut < 0:
                if final:
                    break                          # what is left has no complete spectrum: the host pass
                more = f.read(max(max_bytes, 1 << 16))
                final = len(more) == 0
                buf += more
                continue
            cut += len(_CLOSE)
            if cut >= 0x7FFFFFFF:
                break                              # one spectrum beyond the device's 2^31 - 2 bytes: the host pass
            head = buf[:cut]
            res = ctx.scan_mzml(head)
            if res["flags"]:
                break
            chunk, stopped = _device_chunk(head, res, groups, filename)
            yield chunk
            if stopped:
                return
            last = head.rfind(b"\n")
            lines += head.count(b"\n")
            tail = head[last + 1:]
            column = (column if last < 0 else 0) + len(tail) - sum(tail.count(bytes([c])) for c in range(0x80, 0xC0))
            del buf[:cut]
        filler = b"\n" * lines + b" " * column
        yield from _iterparse_chunks(_Chain([header, filler, bytes(buf)], f), filename, DEFAULT_CHUNK_BYTES)


def get_spectra(source: str) -> Iterator[Dict]:
    """Yield dicts like mgf_io.get_spectra: identifier, precursor_mz, precursor_charge (int or None), retention_time,
    mz f64[], intensity f32[] (arrays decoded on the host)."""
    for chunk in read_chunks(source):
        yield from chunk.host_spectra()
