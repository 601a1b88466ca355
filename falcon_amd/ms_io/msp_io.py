"""MSP spectral libraries (`--library`): the text format NIST, MoNA and MassBank distribute, GNPS offers next to MGF and matchms
writes as `save_as_msp`.  `read_annotation_library` has the contract of `mgf_io.read_annotation_library`; without `ctx` it is the
host reader of record, with `ctx` the device path (`read_annotation_chunks`; DESIGN.md "MSP on the device"), which mirrors it
bit for bit and defers to it wherever it cannot decide.

The grammar, stated once:

Lines
  - Lines are stripped of space, tab, CR and LF.
  - A line is `key: value`.  The key is what stands before the first `:`, stripped and compared without case.  The value is
    what stands behind it, stripped.
Entries
  - An entry begins at a line whose key is exactly `name`.  It ends before the next such line, or at the end of the file.
  - Blank lines do not end an entry.  Anything before the first `Name:` line is ignored.
  - Entries count from 1 per file, skipped ones included.
Header lines
  - From the `Name:` line up to the first line whose key is `num peaks`, every non-blank line is a header line.
  - The last line of a key wins.  A line without `:` is ignored.
Peak text
  - Every non-blank line behind `Num Peaks:` inside the entry is peak text (a second `Num Peaks:` line included).
  - The line is cut at its first `"` (NIST peak annotations are quoted and may hold `;`); the rest is split at `;`.
  - Every segment that is non-empty after stripping is one peak: its first whitespace-separated token is m/z (`float()`), its
    second is intensity (`float()`, or 0.0 when absent); further tokens are ignored.
  - A token `float()` rejects marks the entry malformed.
Columns
  - Precursor: the first whitespace-separated token of `precursormz`, else `precursor_mz`, else `pepmass` (an empty value
    counts as absent).
  - Charge: `charge` through `mgf_io._parse_charge`; 0 when the key is absent, empty, or that function rejects the value.
  - Name: `name`.  Identifier: `spectrumid`, else `db#`, else `accession`, else `<file base name>:<entry number>`.
  - Adduct: `precursor_type`, else `adduct`.  Ionmode: `ion_mode`, else `ionmode`.  `smiles` and `inchikey` by their own keys.
Skipped, and counted in `skipped`
  - No usable precursor: missing, unparsable, not finite, or <= 0.
  - No `Num Peaks:` line; a `Num Peaks` value `int()` rejects; a peak count different from that value.
  - A malformed peak token.
Not handled
  - MoNA's `SMILES=` / `InChIKey=` inside `Comments:`; deriving a charge from `Precursor_type`; peak separators other than space,
    tab and `;`.  Agreement with NIST's, MoNA's or matchms' own readers is not pinned: the tests' texts are hand-written in
    those three styles.
"""
from __future__ import annotations

import io
import os
import re
from typing import Optional

import numpy as np

from . import mgf_io
from .mgf_io import ANNOTATION_KEYS, DEFAULT_CHUNK_BYTES, EntryChunk

_WS = " \t\r\n"
PRECURSOR_KEYS = ("precursormz", "precursor_mz", "pepmass")
IDENTIFIER_KEYS = ("spectrumid", "db#", "accession")
ADDUCT_KEYS = ("precursor_type", "adduct")
IONMODE_KEYS = ("ion_mode", "ionmode")
# the header keys the device reader asks for (its parse call reads the precursor aliases, charge and num peaks itself)
LIBRARY_KEYS = ("name",) + IDENTIFIER_KEYS + ADDUCT_KEYS + IONMODE_KEYS + ("smiles", "inchikey")


def _first(params, keys) -> str:
    """`params[a] or params[b] or ...` over `keys`, "" when none holds a non-empty value"""
    for k in keys:
        if params.get(k):
            return params[k]
    return ""


def _annotation_entry(params, mzs, its, bad, fn, entry):
    """the per-entry rule: an entry's header values and peaks -> its dict, None when it is skipped"""
    try:
        pmz = float(_first(params, PRECURSOR_KEYS).split()[0])
        declared = int(params["num peaks"])
    except (ValueError, KeyError, IndexError):
        return None
    if bad or declared != len(mzs) or not pmz > 0.0 or not np.isfinite(pmz):
        return None
    try:
        charge = mgf_io._parse_charge(params["charge"]) if params.get("charge") else 0
    except (ValueError, IndexError):
        charge = 0
    return {"identifier": _first(params, IDENTIFIER_KEYS) or f"{os.path.basename(fn)}:{entry}", "precursor_mz": pmz,
            "precursor_charge": charge, "retention_time": -1.0, "mz": np.asarray(mzs, np.float64),
            "intensity": np.asarray(its, np.float32), "name": params.get("name", ""), "filename": fn,
            "adduct": _first(params, ADDUCT_KEYS), "smiles": params.get("smiles", ""), "inchikey": params.get("inchikey", ""),
            "ionmode": _first(params, IONMODE_KEYS)}


def _annotation_entries(lines, fn, entry: int = 0):
    """the entries of MSP text `lines` (a file, or one entry's own text) of file `fn` -> (entry number, dict or None for a
    skipped entry), numbered from `entry` + 1"""
    params, mzs, its, bad, in_peaks = None, [], [], False, False
    for line in lines:
        line = line.strip(_WS)
        if not line:
            continue
        key, colon, value = line.partition(":")
        key = key.strip(_WS).lower()
        if colon and key == "name":
            if params is not None:
                entry += 1
                yield entry, _annotation_entry(params, mzs, its, bad, fn, entry)
            params, mzs, its, bad, in_peaks = {"name": value.strip(_WS)}, [], [], False, False
        elif params is None:
            continue
        elif not in_peaks:
            if colon:
                params[key] = value.strip(_WS)
                in_peaks = key == "num peaks"
        else:
            for segment in line.split('"', 1)[0].split(";"):
                if not segment.strip(_WS):
                    continue
                tok = segment.split()
                try:
                    mzs.append(float(tok[0]))
                    its.append(float(tok[1]) if len(tok) > 1 else 0.0)
                except (ValueError, IndexError):
                    bad = True
    if params is not None:
        entry += 1
        yield entry, _annotation_entry(params, mzs, its, bad, fn, entry)


def read_annotation_library(filenames, counts: Optional[dict] = None, ctx=None):
    """The entries of MSP library files, in order, as `mgf_io.read_annotation_library` returns an MGF library's: dicts with
    `identifier`, `precursor_mz`, `precursor_charge` (0: none), `retention_time` -1.0, `mz` f64, `intensity` f32, `name`,
    `filename`, and `adduct`, `smiles`, `inchikey`, `ionmode` as strings ("" when absent); the module docstring states the
    grammar and the skip rules.  `counts` (a dict) receives `entries` and `skipped`.  Without `ctx` the host reader; with `ctx`
    (a `device.Context`) the files are read on the device (`read_annotation_chunks`): the same entries and counts, as a list of
    `EntryChunk`s -- `mgf_io.chunk_entries` makes the dicts of them -- and `counts` also receives `host`."""
    if ctx is not None:
        return read_annotation_chunks(filenames, ctx, counts)
    out, n_entries, n_skipped = [], 0, 0
    for fn in filenames:
        entry = 0
        with open(fn, "r") as f:
            for entry, spec in _annotation_entries(f, fn):
                if spec is None:
                    n_skipped += 1
                else:
                    out.append(spec)
        n_entries += entry
    if counts is not None:
        counts.update(entries=n_entries, skipped=n_skipped)
    return out


_NAME_LINE = re.compile(rb"^[ \t]*[Nn][Aa][Mm][Ee][ \t]*:", re.M)


def _cut(buf, final: bool) -> int:
    """bytes of `buf` in front of its last `Name:` line that does not begin the buffer (the reader is between two entries
    there); 0: none; everything when `final`"""
    if final:
        return len(buf)
    window = 1 << 16
    while True:
        lo = max(len(buf) - window, 0)
        if lo:                                        # (the window begins at a line start)
            lo = buf.find(b"\n", lo) + 1
            if lo == 0:
                lo = len(buf)
        at = [m.start() + lo for m in _NAME_LINE.finditer(bytes(buf[lo:])) if m.start() + lo > 0]
        if at:
            return at[-1]
        if lo == 0 or window >= len(buf):
            return 0
        window *= 4


def _first_column(text, keys) -> np.ndarray:
    """`_first` over whole columns: per entry the first non-empty string among text[k] for k in keys"""
    out = text[keys[-1]]
    for k in reversed(keys[:-1]):
        out = np.where(text[k] != "", text[k], out)
    return out


def read_annotation_chunks(filenames, ctx, counts: Optional[dict] = None, max_bytes: int = DEFAULT_CHUNK_BYTES) -> list:
    """`read_annotation_library` on the device: every file cut in front of `Name:` lines into stretches of about `max_bytes`
    (`mgf_io._stretches` with this module's `_cut`), each through `ctx.parse_msp` with `LIBRARY_KEYS`, the string columns
    through `ctx.text_rows`, the column and skip rules of `_annotation_entry` applied to whole arrays.  An entry with status HOST
    or a HOST key is read again from its own bytes by `_annotation_entries` and patched into its slot (a device / host peak
    count mismatch raises); a stretch outside the device grammar hands the rest of its file to that rule, the entry number
    carried over.  -> EntryChunks, the peaks left on the device; `counts` as the host reader's, plus `host`: the entries the
    host rule read."""
    from .._lib import MGF_KEY_HOST, MSP_ST_HOST
    strings = ("identifier", "name") + ANNOTATION_KEYS
    chunks, n_entries, n_skipped, n_host = [], 0, 0, 0
    for fn in filenames:
        entry = 0
        for head, res in mgf_io._stretches(fn, ctx, max_bytes, cut=_cut, parser=ctx.parse_msp, keys=LIBRARY_KEYS):
            if head is None:
                specs = []
                for entry, spec in _annotation_entries(res, fn, entry):
                    n_host += 1
                    if spec is None:
                        n_skipped += 1
                    else:
                        specs.append(spec)
                if specs:
                    chunks.append(mgf_io._host_entry_chunk(specs, mgf_io._ANNOTATION_COLUMNS, fn))
                break
            n = len(res["status"])
            number = entry + 1 + np.arange(n)
            entry += n
            text = {k: mgf_io._text_column(ctx, head, res["text"], res["key_span"], j) for j, k in enumerate(LIBRARY_KEYS)}
            ident = _first_column(text, IDENTIFIER_KEYS)
            cols = dict(identifier=ident, precursor_mz=res["precursor_mz"].copy(),
                        precursor_charge=np.where(res["has_charge"], res["charge"], 0).astype(np.int32),
                        retention_time=np.full(n, -1.0), name=text["name"], adduct=_first_column(text, ADDUCT_KEYS),
                        smiles=text["smiles"], inchikey=text["inchikey"], ionmode=_first_column(text, IONMODE_KEYS))
            dropped = ~(cols["precursor_mz"] > 0.0)          # (a decided precursor is finite)
            host = np.flatnonzero((res["status"] == MSP_ST_HOST) | (res["key_state"] == MGF_KEY_HOST).any(axis=1))
            unnamed = np.flatnonzero(ident == "")
            if len(host) or len(unnamed):                    # (strings of any length are patched in: object columns meanwhile)
                for k in strings:
                    cols[k] = cols[k].astype(object)
                for i in unnamed:
                    cols["identifier"][i] = f"{os.path.basename(fn)}:{number[i]}"
            if len(host):
                indptr = res["indptr"].cpu().numpy()
                pos, mzs, its = [], [], []
                for i in host:
                    a, b = res["span"][i]
                    (_, s), = _annotation_entries(io.StringIO(bytes(head[a:b]).decode("ascii")), fn, int(number[i]) - 1)
                    dropped[i] = s is None
                    if s is None:
                        continue
                    size = int(indptr[i + 1] - indptr[i])
                    if len(s["mz"]) != size:
                        raise RuntimeError(f"MSP entry at bytes {a}-{b}: {size} peaks on the device, {len(s['mz'])} on the host")
                    order = np.argsort(s["mz"], kind="stable")
                    pos.append(np.arange(indptr[i], indptr[i + 1]))
                    mzs.append(s["mz"][order])
                    its.append(s["intensity"][order])
                    for k in cols:
                        cols[k][i] = s[k]
                mgf_io._patch_peaks(res, pos, mzs, its)
            for k in strings:
                cols[k][dropped] = ""
                if cols[k].dtype == object:
                    cols[k] = np.array(list(cols[k]), dtype=str)
            cols["precursor_mz"][dropped], cols["precursor_charge"][dropped] = 0.0, 0
            n_skipped, n_host = n_skipped + int(dropped.sum()), n_host + len(host)
            chunks.append(EntryChunk(res["indptr"], res["mz"], res["intensity"], cols, dropped, len(host), "device", fn))
        n_entries += entry
    if counts is not None:
        counts.update(entries=n_entries, skipped=n_skipped, host=n_host)
    return chunks
