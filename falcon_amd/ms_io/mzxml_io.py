"""mzXML reading without pyteomics / lxml (both absent): a streaming stdlib ElementTree pass.

Fields as the reference reads them (falcon/ms_io/mzxml_io.py:14-74, pyteomics underneath): scans with `msLevel` > 1, found at
any depth (MS2 scans nest inside their MS1 scan); identifier = `scan/@num` (pyteomics sets `id` to it); precursor m/z = text
of the first `precursorMz`, charge = its `precursorCharge`, else None; retention time = `retentionTime` ("PT...S") in minutes,
as pyteomics reports it (PARITY UNPINNED), -1 when absent.  One `peaks` element per scan: `precision` 32 / 64, network byte
order, m/z-intensity pairs interleaved, `compressionType` none / zlib; its value count is the scan's `peaksCount`.  A scan that
lacks a required field is skipped silently (the reference's `except (ValueError, KeyError)`); one whose peaks this build does
not decode is skipped and counted in `PeakChunk.skipped`.  A parse error part-way logs a warning and keeps what was read.
"""
from __future__ import annotations

import logging
import re
import xml.etree.ElementTree as ET
from typing import Dict, Iterator

from .._lib import PEAK_BIG_ENDIAN, PEAK_F64, PEAK_PAIRS, PEAK_ZLIB
from .peak_payload import DEFAULT_CHUNK_BYTES, PeakChunk

logger = logging.getLogger("falcon")

_DURATION = re.compile(r"^\s*-?P(?:(\d+(?:\.\d*)?)D)?(?:T(?:(\d+(?:\.\d*)?)H)?(?:(\d+(?:\.\d*)?)M)?(?:(\d+(?:\.\d*)?)S)?)?\s*$")


def _local(tag: str) -> str:
    return tag.rpartition("}")[2]


def _minutes(duration: str) -> float:
    """xs:duration -> minutes ("PT90.5S" -> 1.5083...)"""
    m = _DURATION.match(duration)
    if not m or not any(m.groups()):
        raise ValueError(f"bad retention time {duration!r}")
    d, h, mi, s = (float(g) if g else 0.0 for g in m.groups())
    v = d * 1440.0 + h * 60.0 + mi + s / 60.0
    return -v if duration.strip().startswith("-") else v


class _Unsupported(Exception):
    pass


def _scan(chunk: PeakChunk, sc) -> None:
    level = sc.get("msLevel")
    try:
        if level is None or int(level) <= 1:
            return
        ident = sc.attrib["num"]
        rt = _minutes(sc.get("retentionTime")) if sc.get("retentionTime") is not None else -1.0
        pre = peaks = None
        for c in sc:
            t = _local(c.tag)
            if t == "precursorMz" and pre is None:
                pre = c
            elif t == "peaks" and peaks is None:
                peaks = c
        if pre is None or peaks is None:
            raise KeyError("precursorMz / peaks")
        pmz = float((pre.text or "").strip())
        charge = int(pre.get("precursorCharge")) if pre.get("precursorCharge") is not None else None
        count = int(sc.attrib["peaksCount"])
        flags = PEAK_PAIRS | PEAK_BIG_ENDIAN
        precision = peaks.get("precision", "32")
        if precision == "64":
            flags |= PEAK_F64
        elif precision != "32":
            raise _Unsupported(f"peaks precision {precision}")
        if peaks.get("byteOrder", "network") != "network":
            raise _Unsupported("peaks byte order other than network")
        if peaks.get("pairOrder", peaks.get("contentType", "m/z-int")) != "m/z-int":
            raise _Unsupported("peaks content other than m/z-int pairs")
        comp = peaks.get("compressionType", "none")
        if comp == "zlib":
            flags |= PEAK_ZLIB
        elif comp != "none":
            raise _Unsupported(f"{comp} compression")
        row = chunk.add_array("".join((peaks.text or "").split()).encode("ascii"), count, flags)
        chunk.add_spectrum(ident, pmz, charge, rt, row, row)
    except _Unsupported as e:
        chunk.skipped[str(e)] += 1
    except (ValueError, KeyError, TypeError):
        pass


def read_chunks(filename: str, max_bytes: int = DEFAULT_CHUNK_BYTES) -> Iterator[PeakChunk]:
    """stream an mzXML file -> PeakChunks of at most about `max_bytes` of base64 payload each"""
    chunk = PeakChunk()
    stack = []
    scans = 0                 # open scan elements: their direct children are still needed
    try:
        for ev, el in ET.iterparse(filename, events=("start", "end")):
            tag = _local(el.tag)
            if ev == "start":
                stack.append(el)
                scans += tag == "scan"
                continue
            stack.pop()
            if tag == "scan":
                scans -= 1
                _scan(chunk, el)                                        # a nested scan ends (and goes) before its parent
                if chunk.nbytes >= max_bytes:
                    yield chunk
                    chunk = PeakChunk()
            elif scans:
                continue
            if stack:
                stack[-1].remove(el)
    except ET.ParseError as e:
        logger.warning("Failed to read file %s: %s", filename, e)
    yield chunk


def get_spectra(source: str) -> Iterator[Dict]:
    """Yield dicts like mgf_io.get_spectra (arrays decoded on the host)."""
    for chunk in read_chunks(source):
        yield from chunk.host_spectra()
