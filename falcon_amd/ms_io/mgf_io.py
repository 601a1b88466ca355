"""MGF reading / writing without pyteomics (absent here).

Fields as the reference reads them (falcon/ms_io/mgf_io.py:33-66): TITLE, PEPMASS (first
token), CHARGE (optional; "2+", "3+", "2" ...), RTINSECONDS (default -1), then the peak
list.  Malformed spectra are skipped silently, as mgf_io.py:27-30 does.  Writing follows
mgf_io.py:85-116 (TITLE, PEPMASS, CHARGE, RTINSECONDS, peaks).
"""
from __future__ import annotations

import io
import locale
import os
from typing import Dict, Iterable, Iterator, Optional

import numpy as np

DEFAULT_CHUNK_BYTES = 256 << 20      # text of one device call (the line table is sized by it: DESIGN.md "MGF on the device")


def _parse_charge(txt: str):
    t = txt.strip().split()[0].split(",")[0].split("and")[0].strip()
    sign = -1 if t.endswith("-") else 1
    t = t.rstrip("+-")
    return sign * int(t)


def get_spectra(source) -> Iterator[Dict]:
    """Yield dicts: identifier, precursor_mz, precursor_charge (int or None), retention_time,
    mz f64[], intensity f32[]."""
    close = False
    if isinstance(source, str):
        f, close = open(source, "r"), True
    else:
        f = source
    try:
        params, mzs, its, inside = {}, [], [], False
        for line in f:
            line = line.strip()
            if not line or line[0] in "#;!/":
                continue
            if line == "BEGIN IONS":
                params, mzs, its, inside = {}, [], [], True
            elif line == "END IONS":
                if inside:
                    try:
                        if "__bad__" in params:          # a peak line that did not parse: the spectrum is skipped
                            raise ValueError("malformed peak line")
                        yield {
                            "identifier": params["title"],
                            "precursor_mz": float(params["pepmass"].split()[0]),
                            "precursor_charge": _parse_charge(params["charge"]) if "charge" in params else None,
                            "retention_time": float(params.get("rtinseconds", -1)),
                            "mz": np.asarray(mzs, np.float64),
                            "intensity": np.asarray(its, np.float32),
                        }
                    except (ValueError, KeyError, IndexError):
                        pass
                inside = False
            elif inside:
                if "=" in line and not (line[0].isdigit() or line[0] == "."):
                    k, v = line.split("=", 1)
                    params[k.strip().lower()] = v.strip()
                else:
                    tok = line.split()
                    try:
                        mzs.append(float(tok[0]))
                        its.append(float(tok[1]) if len(tok) > 1 else 0.0)
                    except ValueError:
                        params["__bad__"] = True
    finally:
        if close:
            f.close()


class MgfLibraryError(ValueError):
    """a representative MGF (`--assign_to`) without a usable CLUSTER= id; the message names the file and the entry"""


def get_library_spectra(filename: str) -> Iterator[Dict]:
    """The spectra of a representative MGF (what `--export_representatives` writes): `get_spectra`'s dicts plus `cluster`, the
    integer of the entry's CLUSTER= line.  Every BEGIN IONS .. END IONS entry goes through `get_spectra` itself (an entry it
    skips is skipped here); an entry it accepts without CLUSTER=, or with a value that is no integer, raises MgfLibraryError."""
    with open(filename, "r") as f:
        lines, inside, entry = [], False, 0
        for line in f:
            t = line.strip()
            if t == "BEGIN IONS":
                lines, inside = [line], True
                continue
            if not inside:
                continue
            lines.append(line)
            if t != "END IONS":
                continue
            inside = False
            entry += 1
            got = list(get_spectra(io.StringIO("".join(lines))))
            if len(got) != 1:
                continue
            value = None
            for l in lines[1:-1]:
                l = l.strip()
                if l and l[0] not in "#;!/" and "=" in l and not (l[0].isdigit() or l[0] == "."):
                    k, v = l.split("=", 1)
                    if k.strip().lower() == "cluster":
                        value = v.strip()
            where = f"{filename}: entry {entry} (TITLE={got[0]['identifier']})"
            if value is None:
                raise MgfLibraryError(f"{where} has no CLUSTER= line: not a file of cluster representatives")
            try:
                got[0]["cluster"] = int(value)
            except ValueError:
                raise MgfLibraryError(f"{where}: CLUSTER={value} is not an integer") from None
            yield got[0]


def read_library(filenames, ctx=None):
    """every spectrum of the representative MGFs `filenames`, in order, each with `cluster` and `filename`; the same cluster id
    twice (inside one file or across them) raises MgfLibraryError.  With `ctx` (a `device.Context`) the files are read on the
    device (`read_library_chunks`): the same spectra and the same first error, as a list of `EntryChunk`s -- `chunk_entries`
    makes the dicts of them."""
    if ctx is not None:
        return read_library_chunks(filenames, ctx)
    out, seen = [], {}
    for fn in filenames:
        for k, s in enumerate(get_library_spectra(fn)):
            if s["cluster"] in seen:
                raise MgfLibraryError(f"{fn}: spectrum {k + 1} (TITLE={s['identifier']}) repeats CLUSTER={s['cluster']} of "
                                      f"{seen[s['cluster']]}")
            seen[s["cluster"]] = f"{fn} (TITLE={s['identifier']})"
            s["filename"] = fn
            out.append(s)
    return out


ANNOTATION_KEYS = ("adduct", "smiles", "inchikey", "ionmode")


LIBRARY_KEYS = ("spectrumid", "name", "compound_name") + ANNOTATION_KEYS      # the header keys the device reader asks for


def _annotation_entry(params, mzs, its, bad, fn, entry):
    """the per-entry rule of `read_annotation_library`: an entry's header values and peaks -> its dict, None when it is skipped"""
    try:
        pmz = float(params["pepmass"].split()[0])
        charge = _parse_charge(params["charge"]) if params.get("charge") else 0
    except (ValueError, KeyError, IndexError):
        bad = True
    if bad or not pmz > 0.0 or not np.isfinite(pmz):
        return None
    spec = {"identifier": params.get("spectrumid") or params.get("title") or f"{os.path.basename(fn)}:{entry}",
            "precursor_mz": pmz, "precursor_charge": charge,
            "retention_time": -1.0, "mz": np.asarray(mzs, np.float64), "intensity": np.asarray(its, np.float32),
            "name": params.get("name") or params.get("compound_name") or "", "filename": fn}
    spec.update({k: params.get(k, "") for k in ANNOTATION_KEYS})
    return spec


def _annotation_entries(lines, fn, entry: int = 0):
    """the entries of library text `lines` (a file, or one entry's own text) of file `fn` -> (entry number, dict or None for a
    skipped entry), numbered from `entry` + 1"""
    params, mzs, its, inside, bad = {}, [], [], False, False
    for line in lines:
        line = line.strip()
        if not line or line[0] in "#;!/":
            continue
        if line == "BEGIN IONS":
            params, mzs, its, inside, bad = {}, [], [], True, False
        elif line == "END IONS":
            if not inside:
                continue
            inside = False
            entry += 1
            yield entry, _annotation_entry(params, mzs, its, bad, fn, entry)
        elif inside:
            if "=" in line and not (line[0].isdigit() or line[0] == "."):
                k, v = line.split("=", 1)
                params[k.strip().lower()] = v.strip()
            else:
                tok = line.split()
                try:
                    mzs.append(float(tok[0]))
                    its.append(float(tok[1]) if len(tok) > 1 else 0.0)
                except ValueError:
                    bad = True


def read_annotation_library(filenames, counts: Optional[dict] = None, ctx=None):
    """The entries of reference spectral library MGFs (`--library`; GNPS style), in order: `get_spectra`'s dicts --
    `precursor_charge` 0 for an entry without CHARGE= or with CHARGE=0 -- plus `name` (NAME=, else COMPOUND_NAME=, else ""),
    `filename`, and `adduct`, `smiles`, `inchikey`, `ionmode` as strings ("" when absent).  `identifier` is SPECTRUMID=, else
    TITLE=, else `<file name>:<entry number>` (the file's base name; entries count from 1, skipped ones included).  An entry
    with no usable precursor (PEPMASS missing, unparsable or <= 0) or with a malformed peak line is skipped; `counts` (a dict)
    receives `entries` and `skipped`.  Without `ctx` a host reader; with `ctx` (a `device.Context`) the files are read on the
    device (`read_annotation_chunks`): the same entries and counts, as a list of `EntryChunk`s -- `chunk_entries` makes the
    dicts of them."""
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


def raw_csr(specs):
    """spectra of one peak file -> raw CSR (mz f64, intensity f32, indptr i64), peaks sorted by m/z inside every spectrum
    (stable), which is what spectrum_utils does when the reference constructs an MsmsSpectrum"""
    sizes = np.array([len(s["mz"]) for s in specs], np.int64)
    indptr = np.zeros(len(specs) + 1, np.int64)
    np.cumsum(sizes, out=indptr[1:])
    mz = np.concatenate([np.asarray(s["mz"], np.float64) for s in specs]) if len(specs) else np.zeros(0)
    it = np.concatenate([np.asarray(s["intensity"], np.float32) for s in specs]) if len(specs) else np.zeros(0, np.float32)
    order = np.lexsort((mz, np.repeat(np.arange(len(specs)), sizes)))
    return mz[order], it[order], indptr


class MgfChunk:
    """The spectra of one stretch of an MGF file, in file order: the raw CSR `indptr` / `mz` / `intensity` (device tensors from
    the device reader, host arrays where the host reader read the stretch) and the host columns `identifier` (str),
    `precursor_mz` f64, `precursor_charge` i32 (0: none), `retention_time` f64.  `dropped`: spectra the host reader rejects
    (their rows stay, so that the CSR is the device's; they are no spectra and are not counted).  `n_host`: spectra the host
    reader decided; `reader`: "device", or "host" for a stretch outside the device grammar."""

    def __init__(self, indptr, mz, intensity, identifier, precursor_mz, precursor_charge, retention_time, dropped, n_host, reader):
        self.indptr, self.mz, self.intensity = indptr, mz, intensity
        self.identifier, self.precursor_mz, self.precursor_charge = identifier, precursor_mz, precursor_charge
        self.retention_time, self.dropped, self.n_host, self.reader = retention_time, dropped, n_host, reader

    def __len__(self):
        return len(self.precursor_mz)


def _host_chunk(specs) -> MgfChunk:
    mz, it, indptr = raw_csr(specs)
    return MgfChunk(indptr, mz, it, np.array([str(s["identifier"]) for s in specs], dtype=str),
                    np.array([s["precursor_mz"] for s in specs], np.float64),
                    np.array([int(s["precursor_charge"]) if s.get("precursor_charge") else 0 for s in specs], np.int32),
                    np.array([s["retention_time"] for s in specs], np.float64), np.zeros(len(specs), bool), len(specs), "host")


def _cut(buf, final: bool) -> int:
    """bytes of `buf` up to and including the last complete line that strips to END IONS (the reader is outside a spectrum
    behind it); 0: none; everything when `final`"""
    if final:
        return len(buf)
    end = len(buf)
    while True:
        pos = buf.rfind(b"END IONS", 0, end)
        if pos < 0:
            return 0
        stop = buf.find(b"\n", pos)
        begin = buf.rfind(b"\n", 0, pos) + 1
        if stop >= 0 and bytes(buf[begin:stop]).strip(b" \t\r") == b"END IONS":
            return stop + 1
        end = pos


_TITLE_WIDTH = 256       # identifiers up to this length are gathered as one fixed-width array; longer ones one by one


def _identifiers(text: np.ndarray, title: np.ndarray) -> np.ndarray:
    """the title byte ranges of a chunk -> str array, without a Python loop over the spectra"""
    n = len(title)
    if n == 0:
        return np.zeros(0, dtype=str)
    lo, size = title[:, 0], title[:, 1] - title[:, 0]
    w = int(min(max(size.max(initial=0), 1), _TITLE_WIDTH))
    col = np.arange(w)
    chars = text[np.minimum(lo[:, None] + col, max(len(text) - 1, 0))] if len(text) else np.zeros((n, w), np.uint8)
    chars = np.where(col < size[:, None], chars, 0).astype(np.uint8)
    out = np.ascontiguousarray(chars).view(f"S{w}").reshape(n)
    long = np.flatnonzero(size > w)
    if len(long):
        out = out.astype(object)
        for i in long:
            out[i] = text[title[i, 0]:title[i, 1]].tobytes()
        return np.array([b.decode("ascii") for b in out], dtype=str)
    return np.char.decode(out, "ascii")


def _device_chunk(ctx, buf, res) -> MgfChunk:
    """one parsed stretch: identifiers from the title ranges, and every HOST spectrum read again by `get_spectra` from its own
    byte range and patched into its slot"""
    import torch
    from .._lib import MGF_ST_HOST
    text = np.frombuffer(buf, np.uint8)
    n = len(res["status"])
    ident = _identifiers(text, res["title"])
    pmz, rt = res["precursor_mz"].copy(), res["retention_time"].copy()
    charge = np.where(res["has_charge"], res["charge"], 0).astype(np.int32)
    dropped = np.zeros(n, bool)
    host = np.flatnonzero(res["status"] == MGF_ST_HOST)
    if len(host):
        ident = ident.astype(object)
        indptr = res["indptr"].cpu().numpy()
        pos, mzs, its = [], [], []
        for i in host:
            a, b = res["span"][i]
            got = list(get_spectra(io.StringIO(bytes(buf[a:b]).decode("ascii"))))
            size = int(indptr[i + 1] - indptr[i])
            if len(got) != 1:                      # the host reader rejects it: no spectrum
                dropped[i], ident[i], pmz[i], charge[i], rt[i] = True, "", 0.0, 0, -1.0
                continue
            s = got[0]
            if len(s["mz"]) != size:
                raise RuntimeError(f"MGF spectrum at bytes {a}-{b}: {size} peak lines on the device, {len(s['mz'])} on the host")
            order = np.argsort(s["mz"], kind="stable")
            pos.append(np.arange(indptr[i], indptr[i + 1]))
            mzs.append(s["mz"][order])
            its.append(s["intensity"][order])
            ident[i], pmz[i], rt[i] = str(s["identifier"]), s["precursor_mz"], s["retention_time"]
            charge[i] = int(s["precursor_charge"]) if s["precursor_charge"] else 0
        ident = np.array(list(ident), dtype=str) if n else np.zeros(0, dtype=str)
        _patch_peaks(res, pos, mzs, its)
    return MgfChunk(res["indptr"], res["mz"], res["intensity"], ident, pmz, charge, rt, dropped, len(host), "device")


def _patch_peaks(res, pos, mzs, its) -> None:
    """the host reader's peaks of re-read spectra (sorted by m/z) into their slots `pos` of a parsed stretch's device CSR"""
    import torch
    if pos and sum(len(p) for p in pos):
        at = torch.from_numpy(np.concatenate(pos)).to(res["mz"].device)
        res["mz"][at] = torch.from_numpy(np.concatenate(mzs)).to(res["mz"].device)
        res["intensity"][at] = torch.from_numpy(np.concatenate(its)).to(res["mz"].device)


def _stretches(filename: str, ctx, max_bytes: int, cut=None, parser=None, **parse):
    """The file as bytes, cut directly behind END IONS lines into stretches of about `max_bytes` (a stretch grows when one
    spectrum is larger), each parsed by `ctx.parse_mgf(stretch, **parse)` -> (stretch bytes, result) for every stretch with
    spectra.  A stretch outside the device grammar ends it with (None, the rest of the file -- that stretch included --
    behind the same text layer as `open(filename)`).  `cut` / `parser`: another format's cut rule (`_cut`'s contract) and
    parse call (`msp_io`: in front of a Name: line, `ctx.parse_msp`)."""
    cut, parser = cut or _cut, parser or ctx.parse_mgf
    with open(filename, "rb") as f:
        buf = bytearray()
        final = False
        while not final:
            more = f.read(max(max_bytes - len(buf), max_bytes // 2, 1))
            final = len(more) == 0
            buf += more
            if not final and len(buf) < max_bytes:
                continue
            at = cut(buf, final)
            if at == 0:
                continue                           # one spectrum larger than the stretch: read on
            head = buf[:at]
            res = parser(head, **parse)
            if res["flags"]:
                yield None, io.TextIOWrapper(io.BytesIO(bytes(buf) + f.read()))
                return
            if len(res["status"]):
                yield head, res
            del buf[:at]


def read_chunks(filename: str, ctx, max_bytes: int = DEFAULT_CHUNK_BYTES) -> Iterator[MgfChunk]:
    """The device reader: the file's stretches (`_stretches`), each parsed by `ctx.parse_mgf`; spectra with status HOST are
    read again by `get_spectra`.  A stretch outside the device grammar (a byte the device does not take) ends
    the device path: the rest of the file is read by `get_spectra` through the same text layer as `open(filename)`,
    exceptions included.  The spectra of all chunks together are `get_spectra(filename)`'s."""
    for head, res in _stretches(filename, ctx, max_bytes):
        if head is None:
            yield _host_chunk(list(get_spectra(res)))
            return
        yield _device_chunk(ctx, head, res)


class EntryChunk:
    """The entries of one stretch of a library or representative MGF, in file order: the raw CSR `indptr` / `mz` / `intensity`
    (device tensors from the device reader, host arrays where the host rule read the stretch), `filename`, and `columns`, a
    dict of host arrays by entry -- `identifier` (str), `precursor_mz` f64, `precursor_charge` i32 (0: none),
    `retention_time` f64, and the reader's own (`name`, `adduct`, `smiles`, `inchikey`, `ionmode`; or `cluster`
    i64).  `dropped`: entries the host rule skips (their rows stay, so that the CSR is the device's).  `n_host`:
    entries the host rule decided; `reader`: "device", or "host" for a stretch outside the device grammar."""

    def __init__(self, indptr, mz, intensity, columns, dropped, n_host, reader, filename):
        self.indptr, self.mz, self.intensity, self.columns = indptr, mz, intensity, columns
        self.dropped, self.n_host, self.reader, self.filename = dropped, n_host, reader, filename

    def __len__(self):
        return len(self.dropped)


def chunk_entries(chunks) -> list:
    """`EntryChunk`s -> the dicts the host readers return for the same files, entry by entry (dropped ones left out), with
    the peaks of every entry sorted by m/z as `raw_csr` sorts them"""
    out = []
    for c in chunks:
        host = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (c.indptr, c.mz, c.intensity)]
        indptr, mz, it = host
        for i in np.flatnonzero(~c.dropped):
            s = {k: v[i].item() for k, v in c.columns.items()}
            s.update(mz=mz[indptr[i]:indptr[i + 1]], intensity=it[indptr[i]:indptr[i + 1]], filename=c.filename)
            out.append(s)
    return out


def _text_column(ctx, buf, d_text, span, column: int = 0) -> np.ndarray:
    """the byte ranges span[:, column] (device i64[n, k, 2] or host i64[n, 2]) of a stretch -> str array: `ctx.text_rows` rows of
    the longest range's width, at most `_TITLE_WIDTH`; the few longer ones are taken from the host's copy `buf` one by one"""
    n = len(span)
    if n == 0:
        return np.zeros(0, dtype=str)
    span = ctx.to_dev(span)
    view = span[:, column] if span.dim() == 3 else span
    w = int(min(max(int((view[:, 1] - view[:, 0]).max().item()), 1), _TITLE_WIDTH))
    rows, long = ctx.text_rows(d_text, span, column, w)
    out = np.ascontiguousarray(rows.cpu().numpy()).view(f"S{w}").reshape(n).astype(f"U{w}")
    at = long.nonzero().reshape(-1)
    if len(at):
        out = out.astype(object)
        for i, (a, b) in zip(at.cpu().numpy(), view[at].cpu().numpy()):
            out[i] = bytes(buf[a:b]).decode("ascii")
        out = np.array(list(out), dtype=str)
    return out


def _host_entry_chunk(specs, extra, fn) -> EntryChunk:
    """the dicts of entries the host rule read -> an EntryChunk of host arrays; `extra`: (column, dtype) of the reader's own"""
    mz, it, indptr = raw_csr(specs)
    cols = dict(identifier=np.array([str(s["identifier"]) for s in specs], dtype=str),
                precursor_mz=np.array([s["precursor_mz"] for s in specs], np.float64),
                precursor_charge=np.array([int(s["precursor_charge"]) if s.get("precursor_charge") else 0 for s in specs], np.int32),
                retention_time=np.array([s["retention_time"] for s in specs], np.float64))
    cols.update({k: np.array([s[k] for s in specs], dtype=dt) for k, dt in extra})
    return EntryChunk(indptr, mz, it, cols, np.zeros(len(specs), bool), len(specs), "host", fn)


_ANNOTATION_COLUMNS = tuple((k, str) for k in ("name",) + ANNOTATION_KEYS)


def read_annotation_chunks(filenames, ctx, counts: Optional[dict] = None, max_bytes: int = DEFAULT_CHUNK_BYTES) -> list:
    """`read_annotation_library` on the device: every file's stretches (`_stretches`) through `ctx.parse_mgf` with the title
    optional and `LIBRARY_KEYS`, the string columns through `ctx.text_rows`, the skip and fall-through rules of
    `_annotation_entry` applied to whole columns.  An entry with status HOST or a HOST key is read again from its own bytes by
    `_annotation_entries`; a stretch outside the device grammar hands the rest of its file to that rule, the entry number
    carried over.  -> EntryChunks, the peaks left on the device; `counts` as the host reader's, plus `host`: the entries the
    host rule read."""
    from .._lib import MGF_KEY_HOST, MGF_ST_HOST
    chunks, n_entries, n_skipped, n_host = [], 0, 0, 0
    for fn in filenames:
        entry = 0
        for head, res in _stretches(fn, ctx, max_bytes, optional_title=True, keys=LIBRARY_KEYS):
            if head is None:
                specs = []
                for entry, spec in _annotation_entries(res, fn, entry):
                    n_host += 1
                    if spec is None:
                        n_skipped += 1
                    else:
                        specs.append(spec)
                if specs:
                    chunks.append(_host_entry_chunk(specs, _ANNOTATION_COLUMNS, fn))
                break
            n = len(res["status"])
            number = entry + 1 + np.arange(n)
            entry += n
            state = res["key_state"]
            text = {k: _text_column(ctx, head, res["text"], res["key_span"], j) for j, k in enumerate(LIBRARY_KEYS)}
            title = _text_column(ctx, head, res["text"], res["title"])
            # `a or b or c` of the host rule, on columns (an absent key has the range (0, 0): the empty string)
            ident = np.where(text["spectrumid"] != "", text["spectrumid"], title)
            cols = dict(identifier=ident, precursor_mz=res["precursor_mz"].copy(),
                        precursor_charge=np.where(res["has_charge"], res["charge"], 0).astype(np.int32),
                        retention_time=np.full(n, -1.0), name=np.where(text["name"] != "", text["name"], text["compound_name"]),
                        **{k: text[k] for k in ANNOTATION_KEYS})
            dropped = ~(cols["precursor_mz"] > 0.0)          # (a decided PEPMASS is finite)
            host = np.flatnonzero((res["status"] == MGF_ST_HOST) | (state == MGF_KEY_HOST).any(axis=1))
            unnamed = np.flatnonzero(ident == "")
            if len(host) or len(unnamed):                    # (strings of any length are patched in: object columns meanwhile)
                for k in ("identifier", "name") + ANNOTATION_KEYS:
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
                        raise RuntimeError(f"MGF entry at bytes {a}-{b}: {size} peak lines on the device, {len(s['mz'])} on the host")
                    order = np.argsort(s["mz"], kind="stable")
                    pos.append(np.arange(indptr[i], indptr[i + 1]))
                    mzs.append(s["mz"][order])
                    its.append(s["intensity"][order])
                    for k in cols:
                        cols[k][i] = s[k]
                _patch_peaks(res, pos, mzs, its)
            for k in ("identifier", "name") + ANNOTATION_KEYS:
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


def _host_library_entries(lines, fn, entry: int):
    """`get_library_spectra`'s rule over the text `lines` of file `fn` without its errors -> (entry number, `get_spectra`'s dict
    with `cluster`: the stripped value of the last CLUSTER= line or None; None for an entry `get_spectra` rejects)"""
    block, inside = [], False
    for line in lines:
        t = line.strip()
        if t == "BEGIN IONS":
            block, inside = [line], True
            continue
        if not inside:
            continue
        block.append(line)
        if t != "END IONS":
            continue
        inside = False
        entry += 1
        got = list(get_spectra(io.StringIO("".join(block))))
        if len(got) != 1:
            yield entry, None
            continue
        value = None
        for l in block[1:-1]:
            l = l.strip()
            if l and l[0] not in "#;!/" and "=" in l and not (l[0].isdigit() or l[0] == "."):
                k, v = l.split("=", 1)
                if k.strip().lower() == "cluster":
                    value = v.strip()
        got[0]["cluster"] = value
        yield entry, got[0]


def read_library_chunks(filenames, ctx, counts: Optional[dict] = None, max_bytes: int = DEFAULT_CHUNK_BYTES) -> list:
    """`read_library` on the device: every file's stretches (`_stretches`) through `ctx.parse_mgf` (title required, as
    `get_spectra`) with the key `cluster` as an integer; spectra with status HOST are read again by `get_spectra`
    (`_device_chunk`), a CLUSTER= value outside the integer fast form goes to `int()`.  The problems -- an accepted entry
    without CLUSTER=, with a value that is no integer, or with an id an earlier entry holds -- are found on whole columns; the
    first one in file order raises MgfLibraryError with the host reader's message.  A stretch outside the device grammar
    hands the rest of its file to the host rule, the entry number carried over.  -> EntryChunks with the column `cluster`
    (`precursor_charge` 0: none); `counts` receives `entries` and `host`, the entries the host rule read."""
    from .._lib import MGF_KEY_ABSENT, MGF_KEY_INT, MGF_KEY_PRESENT
    chunks, n_host, n_entries = [], 0, 0
    seen_ids, seen_where = np.zeros(0, np.int64), []          # every id so far; per stretch (file, its first id's place, identifiers)
    for fn in filenames:
        entry = accepted = 0
        for head, res in _stretches(fn, ctx, max_bytes, keys={"cluster": MGF_KEY_INT}):
            if head is None:
                got = list(_host_library_entries(res, fn, entry))
                entry = got[-1][0] if got else entry
                got = [(e, s) for e, s in got if s is not None]
                specs = [s for _, s in got]
                chunk = _host_entry_chunk(specs, (), fn)
                number, ids = np.array([e for e, _ in got], np.int64), np.zeros(len(got), np.int64)
                values = {i: s["cluster"] for i, s in enumerate(specs)}           # every value through int(); None: no CLUSTER= line
            else:
                n = len(res["status"])
                number = entry + 1 + np.arange(n)
                entry += n
                c = _device_chunk(ctx, head, res)
                chunk = EntryChunk(c.indptr, c.mz, c.intensity, dict(identifier=c.identifier, precursor_mz=c.precursor_mz,
                                                                    precursor_charge=c.precursor_charge, retention_time=c.retention_time),
                                   c.dropped, c.n_host, "device", fn)
                state, span, ids = res["key_state"][:, 0], res["key_span"].cpu().numpy()[:, 0], res["key_value"][:, 0].copy()
                decided = (state == MGF_KEY_PRESENT) & (span[:, 1] > span[:, 0])
                values = {int(i): None if state[i] == MGF_KEY_ABSENT else bytes(head[span[i, 0]:span[i, 1]]).decode("ascii")
                          for i in np.flatnonzero(~decided & ~c.dropped)}
            n_host += chunk.n_host
            ident, rows = chunk.columns["identifier"], np.flatnonzero(~chunk.dropped)
            problem = None                                                        # (row, message): the first one in file order
            for i in sorted(values):
                where = f"{fn}: entry {number[i]} (TITLE={ident[i]})"
                if values[i] is None:
                    problem = (i, f"{where} has no CLUSTER= line: not a file of cluster representatives")
                    break
                try:
                    ids[i] = int(values[i])
                except ValueError:
                    problem = (i, f"{where}: CLUSTER={values[i]} is not an integer")
                    break
            good = rows if problem is None else rows[rows < problem[0]]
            both = np.concatenate([seen_ids, ids[good]])
            _, first, inverse = np.unique(both, return_index=True, return_inverse=True)
            repeat = np.flatnonzero(first[inverse] != np.arange(len(both)))
            if len(repeat):
                i, holder = int(good[repeat[0] - len(seen_ids)]), int(first[inverse[repeat[0]]])
                if holder >= len(seen_ids):
                    held = f"{fn} (TITLE={ident[good[holder - len(seen_ids)]]})"
                else:
                    held = next(f"{f} (TITLE={names[holder - at]})" for f, at, names in reversed(seen_where) if at <= holder)
                k = accepted + int(np.searchsorted(rows, i))
                problem = (i, f"{fn}: spectrum {k + 1} (TITLE={ident[i]}) repeats CLUSTER={ids[i]} of {held}")
            if problem is not None:
                raise MgfLibraryError(problem[1])
            seen_where.append((fn, len(seen_ids), ident[rows]))
            seen_ids, accepted = both, accepted + len(rows)
            chunk.columns["cluster"] = np.where(chunk.dropped, 0, ids)
            if len(chunk):
                chunks.append(chunk)
        n_entries += entry
    if counts is not None:
        counts.update(entries=n_entries, host=n_host)
    return chunks


def write_spectra(filename: str, spectra: Iterable[Dict]) -> None:
    with open(filename, "w") as out:
        for s in spectra:
            out.write("BEGIN IONS\n")
            out.write(f"TITLE={s['identifier']}\n")
            out.write(f"PEPMASS={s['precursor_mz']}\n")
            ch = s.get("precursor_charge")
            if ch is not None and not (isinstance(ch, float) and np.isnan(ch)):
                ch = int(ch)
                out.write(f"CHARGE={abs(ch)}{'-' if ch < 0 else '+'}\n")
            if s.get("retention_time") is not None:
                out.write(f"RTINSECONDS={s['retention_time']}\n")
            if "cluster" in s:
                out.write(f"CLUSTER={s['cluster']}\n")
            for m, i in zip(s["mz"], s["intensity"]):
                out.write(f"{m} {i}\n")
            out.write("END IONS\n\n")


_PLAIN = "BEGIN IONS\nTITLE=PEPMASS CHARGE RTINSECONDS CLUSTER END 0123456789.e+-naif"     # every character the writer emits itself


def title_blob(titles, encoding: Optional[str] = None):
    """str array -> (u8 blob of the encoded titles back to back, i64 offsets[n + 1]), without a Python loop over the entries: one
    join and one encode, the offsets from the separators' positions in the blob.  None when the text layer of
    `open(filename, "w")` would not write plain bytes (an encoding that is no superset of ASCII, a platform that translates
    newlines), when a title contains a newline, or when a title cannot be encoded (the host writer then raises)."""
    n = len(titles)
    encoding = encoding or locale.getpreferredencoding(False)
    try:
        if os.linesep != "\n" or _PLAIN.encode(encoding) != _PLAIN.encode("ascii"):
            return None
        joined = "\n".join(np.asarray(titles, dtype=str).tolist()).encode(encoding)
    except (UnicodeEncodeError, LookupError):
        return None
    raw = np.frombuffer(joined, np.uint8)
    sep = np.flatnonzero(raw == 0x0A)
    if len(sep) != max(n - 1, 0):
        return None
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:n] = sep - np.arange(n - 1)                  # (title k begins behind separator k - 1, less the k - 1 taken out before it)
    ptr[n] = len(raw) - len(sep) if n else 0
    return raw[raw != 0x0A] if len(sep) else raw, ptr


def entry_dicts(mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster, titles):
    """the columns of `write_representatives` (host arrays or tensors) -> the dicts `write_spectra` takes, entry by entry"""
    host = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster)]
    mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster = host
    for k, r in enumerate(rows):
        a, b = indptr[r], indptr[r + 1]
        yield {"identifier": str(titles[k]), "precursor_mz": float(precursor_mz[k]), "precursor_charge": int(charge[k]) if charge[k] else None,
               "retention_time": float(retention_time[k]), "mz": mz[a:b], "intensity": intensity[a:b], "cluster": int(cluster[k])}


def _f32(a):
    return a.float() if hasattr(a, "cpu") else np.asarray(a, np.float32)


def write_representatives(filename: str, ctx, mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster, titles,
                          max_bytes: int = DEFAULT_CHUNK_BYTES, append: bool = False) -> str:
    """The device writer: the file `write_spectra` writes for n entries, byte for byte, formatted by `ctx.format_mgf` (DESIGN.md
    "MGF out of the device").  Peaks CSR mz / intensity (float32), indptr; rows[k]: the CSR row whose peaks entry k carries;
    precursor_mz / retention_time (float32), charge (int, 0: no CHARGE line), cluster (int) per entry -- numpy arrays or device
    tensors -- and `titles`, a str array (or what `title_blob` made of one).  The titles are encoded as `open(filename, "w")`
    encodes them; where that cannot be mirrored (`title_blob`) the whole file is `write_spectra`'s.  `append`: add to the file instead of replacing it.
    -> "device" or "host": the writer that wrote it."""
    blob = titles if isinstance(titles, tuple) else title_blob(titles)
    if blob is None:
        if append:
            raise ValueError("write_representatives: the host writer cannot append")
        # (float32 columns, as the device formats them)
        write_spectra(filename, entry_dicts(_f32(mz), _f32(intensity), indptr, rows, _f32(precursor_mz), _f32(retention_time), charge,
                                            cluster, titles))
        return "host"
    with open(filename, "ab" if append else "wb") as out:
        for chunk in ctx.format_mgf(mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster, blob[0], blob[1],
                                    max_bytes=max_bytes, copy=False):
            out.write(memoryview(chunk))
    return "device"
