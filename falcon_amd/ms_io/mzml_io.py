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
"""
from __future__ import annotations

import logging
import xml.etree.ElementTree as ET
from typing import Dict, Iterator

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


def read_chunks(filename: str, max_bytes: int = DEFAULT_CHUNK_BYTES) -> Iterator[PeakChunk]:
    """stream an mzML (or indexedmzML) file -> PeakChunks of at most about `max_bytes` of base64 payload each"""
    groups: Dict[str, list] = {}
    chunk = PeakChunk()
    stack = []
    keep = 0                  # open elements whose subtree is still needed (spectrum, referenceableParamGroup)
    try:
        for ev, el in ET.iterparse(filename, events=("start", "end")):
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


def get_spectra(source: str) -> Iterator[Dict]:
    """Yield dicts like mgf_io.get_spectra: identifier, precursor_mz, precursor_charge (int or None), retention_time,
    mz f64[], intensity f32[] (arrays decoded on the host)."""
    for chunk in read_chunks(source):
        yield from chunk.host_spectra()
