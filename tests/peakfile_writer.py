"""Test-side writers of mzML (plain / indexed, 32 / 64-bit, none / zlib, with or without referenceable param groups) and mzXML
(nested or flat scans, 32 / 64-bit, none / zlib) from spectrum dicts (`identifier`, `precursor_mz`, `precursor_charge`,
`retention_time`, `mz`, `intensity`), plus seeded synthetic spectra.  Only what the readers of falcon_amd.ms_io need is written.

`ms1_every` k > 0 puts an MS1 spectrum in front of every k-th MS2 (the MS2 scans nest inside it in mzXML).  `numpress` /
`bad_base64`: identifiers whose m/z array is marked MS-Numpress / carries a character outside the base64 alphabet.
"""
from __future__ import annotations

import base64
import zlib
from xml.sax.saxutils import quoteattr

import numpy as np


def synthetic_spectra(n: int, seed: int, max_peaks: int = 60, unsorted_every: int = 0):
    """n seeded MS2 spectra; every `unsorted_every`-th has shuffled peaks with tied m/z values"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(0, max_peaks + 1))
        mz = np.sort(rng.uniform(101.0, 1500.0, k))
        if unsorted_every and i % unsorted_every == 0 and k > 3:
            mz[1] = mz[0]
            mz[-1] = mz[0]
            mz = rng.permutation(mz)
        out.append({"identifier": f"scan={i + 1}", "precursor_mz": float(rng.uniform(400.0, 1200.0)),
                    "precursor_charge": int(rng.integers(1, 4)) if i % 7 else None,
                    "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)),
                    "mz": mz, "intensity": rng.uniform(1.0, 1e4, k).astype(np.float32)})
    return out


def _b64(values: np.ndarray, dtype: str, compress, level: int = 6, strategy=None) -> str:
    raw = np.ascontiguousarray(values, dtype=dtype).tobytes()
    if compress:
        if strategy is None:
            raw = zlib.compress(raw, level)
        else:
            c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
            raw = c.compress(raw) + c.flush()
    return base64.b64encode(raw).decode("ascii")


_MS = 'cvRef="MS"'


def _cv(acc, name, value=""):
    return f'<cvParam {_MS} accession="{acc}" name="{name}" value="{value}"/>'


def write_mzml(path, spectra, mz_bits=64, int_bits=32, zlib_arrays=True, indexed=False, param_groups=False, ms1_every=0,
               numpress=(), bad_base64=(), charge_term="MS:1000041"):
    prec = {32: ("MS:1000521", "32-bit float"), 64: ("MS:1000523", "64-bit float")}
    comp = ("MS:1000574", "zlib compression") if zlib_arrays else ("MS:1000576", "no compression")
    parts = ['<?xml version="1.0" encoding="utf-8"?>\n']
    if indexed:
        parts.append('<indexedmzML xmlns="http://psi.hupo.org/ms/mzml">\n')
    parts.append('<mzML xmlns="http://psi.hupo.org/ms/mzml" version="1.1.0">\n')
    if param_groups:
        parts.append('<referenceableParamGroupList count="3">'
                     f'<referenceableParamGroup id="ms2">{_cv("MS:1000511", "ms level", 2)}</referenceableParamGroup>'
                     f'<referenceableParamGroup id="mzs">{_cv(*prec[mz_bits])}{_cv(*comp)}{_cv("MS:1000514", "m/z array")}'
                     '</referenceableParamGroup>'
                     f'<referenceableParamGroup id="ints">{_cv(*prec[int_bits])}{_cv(*comp)}{_cv("MS:1000515", "intensity array")}'
                     '</referenceableParamGroup></referenceableParamGroupList>\n')
    parts.append('<run id="r"><spectrumList count="%d">\n' % len(spectra))
    idx = 0

    def spectrum(sid, level, s):
        nonlocal idx
        n = len(s["mz"])
        mz_dt, it_dt = ("<f8" if mz_bits == 64 else "<f4"), ("<f8" if int_bits == 64 else "<f4")
        mz_txt = _b64(s["mz"], mz_dt, zlib_arrays)
        if sid in bad_base64:
            mz_txt = mz_txt[:4] + "*" + mz_txt[5:]
        mz_extra = _cv("MS:1002312", "MS-Numpress linear prediction compression") if sid in numpress else ""
        lvl = (f'<referenceableParamGroupRef ref="ms2"/>' if param_groups and level == 2 else _cv("MS:1000511", "ms level", level))
        out = [f'<spectrum index="{idx}" id={quoteattr(sid)} defaultArrayLength="{n}">{lvl}'
               f'<scanList count="1"><scan>{_cv("MS:1000016", "scan start time", s["retention_time"])}</scan></scanList>']
        idx += 1
        if level > 1:
            ch = s.get("precursor_charge")
            chp = _cv(charge_term, "charge state", ch) if ch is not None else ""
            out.append('<precursorList count="1"><precursor><selectedIonList count="1"><selectedIon>'
                       f'{_cv("MS:1000744", "selected ion m/z", repr(float(s["precursor_mz"])))}{chp}'
                       '</selectedIon></selectedIonList></precursor></precursorList>')
        out.append('<binaryDataArrayList count="2">')
        for txt, kind, bits, extra in ((mz_txt, "mzs", mz_bits, mz_extra),
                                       (_b64(s["intensity"], it_dt, zlib_arrays), "ints", int_bits, "")):
            if param_groups:
                params = f'<referenceableParamGroupRef ref="{kind}"/>'
            else:
                name = ("MS:1000514", "m/z array") if kind == "mzs" else ("MS:1000515", "intensity array")
                params = _cv(*prec[bits]) + _cv(*comp) + _cv(*name)
            out.append(f'<binaryDataArray encodedLength="{len(txt)}">{params}{extra}\n<binary>{txt}</binary></binaryDataArray>')
        out.append('</binaryDataArrayList></spectrum>\n')
        return "".join(out)

    for i, s in enumerate(spectra):
        if ms1_every and i % ms1_every == 0:
            ms1 = {"mz": np.linspace(300.0, 1800.0, 50), "intensity": np.ones(50, np.float32), "retention_time": s["retention_time"]}
            parts.append(spectrum(f"ms1_{i}", 1, ms1))
        parts.append(spectrum(s["identifier"], 2, s))
    parts.append('</spectrumList></run></mzML>\n')
    if indexed:
        parts.append('<indexList count="1"><index name="spectrum">')
        parts.extend(f'<offset idRef="scan={k}">0</offset>' for k in range(len(spectra)))
        parts.append('</index></indexList><indexListOffset>0</indexListOffset></indexedmzML>\n')
    with open(path, "w") as f:
        f.write("".join(parts))


def write_mzxml(path, spectra, bits=32, zlib_arrays=True, nested=True, ms1_every=5, rt_minutes=False):
    """identifiers must be scan numbers; retention_time is written as PT<seconds>S (so the reader reports seconds / 60)"""
    dt = ">f8" if bits == 64 else ">f4"
    parts = ['<?xml version="1.0" encoding="ISO-8859-1"?>\n<mzXML xmlns="http://sashimi.sourceforge.net/schema_revision/mzXML_3.2">\n'
             '<msRun>\n']
    open_ms1 = False
    num = 10 ** 7

    def peaks(s):
        pairs = np.empty(2 * len(s["mz"]), np.float64)
        pairs[0::2], pairs[1::2] = s["mz"], s["intensity"]
        txt = _b64(pairs, dt, zlib_arrays)
        comp = "zlib" if zlib_arrays else "none"
        return (f'<peaks precision="{bits}" byteOrder="network" pairOrder="m/z-int" compressionType="{comp}" '
                f'compressedLen="0">{txt}</peaks>')

    for i, s in enumerate(spectra):
        if ms1_every and i % ms1_every == 0:
            if open_ms1:
                parts.append('</scan>\n')
            num += 1
            ms1 = {"mz": np.linspace(300.0, 1800.0, 40), "intensity": np.ones(40)}
            parts.append(f'<scan num="{num}" msLevel="1" peaksCount="40" retentionTime="PT{s["retention_time"]}S">{peaks(ms1)}')
            if not nested:
                parts.append('</scan>\n')
            open_ms1 = nested
        ch = s.get("precursor_charge")
        cha = f' precursorCharge="{ch}"' if ch is not None else ""
        parts.append(f'<scan num="{s["identifier"]}" msLevel="2" peaksCount="{len(s["mz"])}" '
                     f'retentionTime="PT{s["retention_time"]}S"><precursorMz precursorIntensity="1.0"{cha}>'
                     f'{repr(float(s["precursor_mz"]))}</precursorMz>{peaks(s)}</scan>\n')
    if open_ms1:
        parts.append('</scan>\n')
    parts.append('</msRun>\n</mzXML>\n')
    with open(path, "w") as f:
        f.write("".join(parts))
