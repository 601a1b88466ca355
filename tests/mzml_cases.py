"""Inputs of the mzML device-reader tests (`test_mzmlscan_cpu.py` on the host build, `test_gpu_mzmlscan.py` on the device): the
clean corpus, the odd cases as byte-level edits of `peakfile_writer`'s output with the status each must get, seeded mutations, and
the comparison of a reader's chunks."""
from __future__ import annotations

import itertools
import os
import re

import numpy as np

from tests import numpress_cases as NC
from tests import peakfile_writer as W

OK, SKIP, HOST = 0, 1, 2
CLOSE = b"</spectrum>"


def corpus_spectra(n=300, seed=11, max_peaks=60):
    """n seeded spectra whose identifiers have every length from 1 to n bytes"""
    spectra = W.synthetic_spectra(n, seed, max_peaks)
    for i, s in enumerate(spectra):
        s["identifier"] = np.base_repr(i, 36).lower().ljust(i + 1, "x")
    return spectra


CORPUS_VARIANTS = [(mz_bits, int_bits, zl, indexed) for mz_bits, int_bits in ((64, 32), (32, 64)) for zl in (True, False)
                   for indexed in (True, False)]


def write_corpus(path, variant, n=300):
    mz_bits, int_bits, zl, indexed = variant
    W.write_mzml(path, corpus_spectra(n), mz_bits=mz_bits, int_bits=int_bits, zlib_arrays=zl, indexed=indexed, ms1_every=3)


def write_numpress_corpus(path, n=60):
    spectra, _ = NC.encoded_spectra(n, 5, NC.PLANS)
    NC.write_mzml(path, spectra)


def split_file(data: bytes):
    """-> header (up to the first <spectrum ), the spectra (each up to and including its </spectrum>), footer"""
    first = data.index(b"<spectrum ")
    end = data.rindex(CLOSE) + len(CLOSE)
    pieces = data[first:end].split(CLOSE)[:-1]
    return data[:first], [p + CLOSE for p in pieces], data[end:]


def _cv(acc, value=None, name="x"):
    v = "" if value is None else f' value="{value}"'
    return f'<cvParam cvRef="MS" accession="{acc}" name="{name}"{v}/>'.encode()


LEVEL = b'<cvParam cvRef="MS" accession="MS:1000511" name="ms level" value="2"/>'
CHARGE = b'<cvParam cvRef="MS" accession="MS:1000041" name="charge state" value="2"/>'
ZLIB = b'<cvParam cvRef="MS" accession="MS:1000574" name="zlib compression" value=""/>'
GROUPS = (b'<referenceableParamGroupList count="1"><referenceableParamGroup id="g">' + _cv("MS:1000000", "1") +
          b'</referenceableParamGroup></referenceableParamGroupList>\n')


def _sub(sp: bytes, old: bytes, new: bytes, count=1) -> bytes:
    assert old in sp, old
    return sp.replace(old, new, count)


def _level_value(v):
    return lambda sp: _sub(sp, LEVEL, LEVEL.replace(b'value="2"', b'value="' + v + b'"'))


def _charge_value(v):
    return lambda sp: _sub(sp, CHARGE, CHARGE.replace(b'value="2"', b'value="' + v + b'"'))


def _first_array(sp: bytes):
    a = sp.index(b"<binaryDataArray ")
    b = sp.index(b"</binaryDataArray>") + len(b"</binaryDataArray>")
    return a, b


def _no_peaks(sp: bytes) -> bytes:
    """both arrays empty, uncompressed, as <binary/>"""
    sp = sp.replace(ZLIB, _cv("MS:1000576", "", "no compression"))
    sp = re.sub(rb'defaultArrayLength="\d+"', b'defaultArrayLength="0"', sp)
    return re.sub(rb"<binary>[^<]*</binary>", b"<binary/>", sp)


def _array_length(sp: bytes) -> bytes:
    n = re.search(rb'defaultArrayLength="(\d+)"', sp).group(1)
    sp = re.sub(rb'defaultArrayLength="\d+"', b'defaultArrayLength="999"', sp)
    return sp.replace(b"<binaryDataArray ", b'<binaryDataArray arrayLength="' + n + b'" ')


def _break_binary(sp: bytes) -> bytes:
    m = re.search(rb"<binary>([^<]{8,})</binary>", sp)
    at = m.start(1) + 4
    return sp[:at] + b"\n " + sp[at:]


def _second(tag: bytes, inner: bytes):
    """a second <tag> element with `inner` behind the first one"""
    close = b"</" + tag + b">"
    return lambda sp: _sub(sp, close, close + b"<" + tag + b">" + inner + close)


def _permuted_level(order):
    attrs = [b'cvRef="MS"', b'accession="MS:1000511"', b'name="ms level"', b'value="2"']
    return lambda sp: _sub(sp, LEVEL, b"<cvParam " + b" ".join(attrs[i] for i in order) + b"/>")


REF = b'<referenceableParamGroupRef ref="g"/>'

# name -> (edit of one MS2 spectrum written with charge 2 and zlib arrays, the status the device must give it)
MS2_CASES = dict(
    [(f"attribute order {''.join(map(str, o))}", (_permuted_level(o), OK)) for o in itertools.permutations(range(4))] + [
        ("plain", (lambda sp: sp, OK)),
        ("> inside a value", (lambda sp: _sub(sp, b'name="ms level"', b'name="ms > level"'), OK)),
        ("' quotes", (lambda sp: _sub(sp, LEVEL, LEVEL.replace(b'value="2"', b"value='2'")), HOST)),
        ("spaces around =", (lambda sp: _sub(sp, LEVEL, LEVEL.replace(b'value="2"', b'value = "2"')), HOST)),
        ("&amp; in the id", (lambda sp: re.sub(rb' id="([^"]*)"', rb' id="\1&amp;b"', sp, 1), HOST)),
        ("UTF-8 in the id", (lambda sp: re.sub(rb' id="([^"]*)"', ' id="\\1\u00e9"'.encode("utf-8"), sp, 1), HOST)),
        ("level 2.0", (_level_value(b"2.0"), HOST)), ("level +2", (_level_value(b"+2"), HOST)),
        ("level ' 2'", (_level_value(b" 2"), HOST)), ("level 2e0", (_level_value(b"2e0"), HOST)),
        ("level 3", (_level_value(b"3"), OK)), ("level 1", (_level_value(b"1"), SKIP)), ("level 0", (_level_value(b"0"), SKIP)),
        ("no level", (lambda sp: _sub(sp, LEVEL, b""), SKIP)),
        ("charge 2.0", (_charge_value(b"2.0"), OK)), ("charge +2", (_charge_value(b"+2"), OK)),
        ("charge ' 2'", (_charge_value(b" 2"), HOST)), ("charge 2e0", (_charge_value(b"2e0"), OK)),
        ("charge -3.9", (_charge_value(b"-3.9"), OK)), ("charge 0", (_charge_value(b"0"), HOST)),
        ("charge x", (_charge_value(b"x"), HOST)),
        ("possible charge only", (lambda sp: _sub(sp, b"MS:1000041", b"MS:1000633"), OK)),
        ("both charge terms", (lambda sp: _sub(sp, CHARGE, _cv("MS:1000633", 3) + CHARGE), OK)),
        ("no charge", (lambda sp: _sub(sp, CHARGE, b""), OK)),
        ("same accessions under isolationWindow / activation",
         (lambda sp: _sub(_sub(sp, b"<precursor><selectedIonList", b"<precursor><isolationWindow>" + _cv("MS:1000744", "1.5") +
                               b"</isolationWindow><selectedIonList"),
                          b"</selectedIonList></precursor>", b"</selectedIonList><activation>" + _cv("MS:1000041", 9) +
                          _cv("MS:1000511", 1) + b"</activation></precursor>"), OK)),
        ("second scan", (_second(b"scan", _cv("MS:1000016", "7.5")), OK)),
        ("second precursor", (_second(b"precursor", b"<selectedIonList><selectedIon>" + _cv("MS:1000744", "99.5") +
                                      b"</selectedIon></selectedIonList>"), OK)),
        ("second selectedIon", (_second(b"selectedIon", _cv("MS:1000744", "98.5") + _cv("MS:1000041", 7)), OK)),
        ("second scanList", (_second(b"scanList", b"<scan>" + _cv("MS:1000016", "8.5") + b"</scan>"), OK)),
        ("repeated accession", (lambda sp: _sub(sp, CHARGE, CHARGE + _cv("MS:1000041", 5)), OK)),
        ("no scanList", (lambda sp: re.sub(rb"<scanList.*</scanList>", b"", sp), HOST)),
        ("no scan start time", (lambda sp: re.sub(rb'<cvParam [^>]*MS:1000016[^>]*/>', b"", sp), OK)),
        ("scan start time without value", (lambda sp: re.sub(rb'(<cvParam [^>]*MS:1000016[^>]*) value="[^"]*"', rb"\1", sp), HOST)),
        ("selected ion m/z without value", (lambda sp: re.sub(rb'(<cvParam [^>]*MS:1000744[^>]*) value="[^"]*"', rb"\1", sp), HOST)),
        ("no selected ion m/z", (lambda sp: re.sub(rb'<cvParam [^>]*MS:1000744[^>]*/>', b"", sp), HOST)),
        ("no id", (lambda sp: re.sub(rb' id="[^"]*"', b"", sp, 1), HOST)),
        ("cvParam with a close tag", (lambda sp: _sub(sp, LEVEL, LEVEL[:-2] + b"></cvParam>"), OK)),
        ("arrayLength over the default", (_array_length, OK)),
        ("<binary/>", (_no_peaks, OK)),
        ("third array of another kind",
         (lambda sp: _sub(sp, b"</binaryDataArrayList>", b'<binaryDataArray encodedLength="0">' + _cv("MS:1000523") + _cv("MS:1000576") +
                          _cv("MS:1000516") + b"<binary></binary></binaryDataArray></binaryDataArrayList>"), OK)),
        ("two m/z arrays", (lambda sp: sp[:_first_array(sp)[1]] + sp[slice(*_first_array(sp))] + sp[_first_array(sp)[1]:], HOST)),
        ("no intensity array", (lambda sp: _sub(sp, b"MS:1000515", b"MS:1000516"), HOST)),
        ("numpress alone", (lambda sp: _sub(sp, ZLIB, _cv("MS:1002312")), OK)),
        ("numpress followed by zlib, one term", (lambda sp: _sub(sp, ZLIB, _cv("MS:1002747")), OK)),
        ("numpress next to zlib", (lambda sp: _sub(sp, ZLIB, ZLIB + _cv("MS:1002314")), HOST)),
        ("two numpress terms", (lambda sp: _sub(sp, ZLIB, _cv("MS:1002312") + _cv("MS:1002313")), HOST)),
        ("truncation term", (lambda sp: _sub(sp, ZLIB, ZLIB + _cv("MS:1003089")), HOST)),
        ("zlib next to no compression", (lambda sp: _sub(sp, ZLIB, ZLIB + _cv("MS:1000576")), HOST)),
        ("no float width", (lambda sp: re.sub(rb'<cvParam [^>]*MS:1000523[^>]*/>', b"", sp, 1), HOST)),
        ("no binary element", (lambda sp: re.sub(rb"<binary>[^<]*</binary>", b"", sp, 1), HOST)),
        ("whitespace in the binary text", (_break_binary, HOST)),
        ("group ref in the spectrum", (lambda sp: _sub(sp, LEVEL, LEVEL + REF), HOST)),
        ("group ref in the scan", (lambda sp: _sub(sp, b"<scan>", b"<scan>" + REF), HOST)),
        ("group ref in the selectedIon", (lambda sp: _sub(sp, b"<selectedIon>", b"<selectedIon>" + REF), HOST)),
        ("group ref in a binaryDataArray", (lambda sp: _sub(sp, b"\n<binary>", REF + b"\n<binary>"), HOST)),
        ("userParam with an entity", (lambda sp: _sub(sp, LEVEL, LEVEL + b'<userParam name="a" value="b&lt;c"/>'), HOST)),
    ])
MS1_CASES = {"MS1": (lambda sp: sp, SKIP), "MS1 with a group ref": (lambda sp: _sub(sp, b"<scanList", REF + b"<scanList"), HOST)}


def odd_file(path, seed=3):
    """one mixed file of all the cases, MS1 cases between them -> (names, expected statuses) in file order"""
    names = list(MS2_CASES)
    spectra = W.synthetic_spectra(len(names), seed, 30)
    for k, s in enumerate(spectra):
        s["identifier"], s["precursor_charge"] = f"case {k}", 2
        if len(s["mz"]) < 3:
            s["mz"], s["intensity"] = np.array([200.0, 300.5, 401.25]), np.array([1.0, 2.0, 3.0], np.float32)
    W.write_mzml(path, spectra, ms1_every=len(names) // 2)
    with open(path, "rb") as f:
        header, pieces, footer = split_file(f.read())
    header = header.replace(b'<run id="r">', GROUPS + b'<run id="r">')
    out, order, expected = [], [], []
    ms1 = itertools.cycle(MS1_CASES.items())
    ms2 = iter(MS2_CASES.items())
    for p in pieces:
        name, (edit, status) = next(ms1) if b'id="ms1_' in p else next(ms2)
        out.append(edit(p))
        order.append(name)
        expected.append(status)
    with open(path, "wb") as f:
        f.write(header + b"".join(out) + footer)
    return order, expected


def mutations(path, seed=17):
    """(name, text from the first <spectrum on, index of the spectrum that must be HOST or None when a flag or a lost spectrum is
    the outcome) for seeded byte mutations of a small file: every kind of grammar violation in a tag of one spectrum, and cuts at
    every offset of the last spectrum"""
    W.write_mzml(path, W.synthetic_spectra(6, seed, 12), ms1_every=4)
    with open(path, "rb") as f:
        _, pieces, _ = split_file(f.read())
    rng = np.random.default_rng(seed)
    out = []
    kinds = {"quote": (b'"', b"'"), "entity": (b'="', b'="&#65;'), "high byte": (b'="', b'="\xc3\xa9'), "no >": (b"/>", b"/ "),
             "stray <": (b'="', b'="<'), "space before =": (b'="', b' ="'), "control byte": (b'="', b'="\x01'),
             "comment": (b"<cvParam", b"<!-- c --><cvParam"), "prefixed name": (b"<cvParam", b"<x:cvParam"),
             "processing instruction": (b"<cvParam", b"<?pi?><cvParam"), "unbalanced close": (b"</scan>", b"</scan></scan>"),
             "nested spectrum": (b"<scanList", b"<spectrum id=\"n\"><scanList"), "lost close": (CLOSE, b"")}
    for name, (old, new) in kinds.items():
        for _ in range(3):
            t = int(rng.integers(0, len(pieces)))
            sp = pieces[t]
            places = [m.start() for m in re.finditer(re.escape(old), sp)]
            at = places[int(rng.integers(0, len(places)))]
            mutated = sp[:at] + new + sp[at + len(old):]
            out.append((f"{name} in spectrum {t} at {at}", b"".join(pieces[:t] + [mutated] + pieces[t + 1:]), t))
    last = pieces[-1]
    for cut in range(len(last)):
        out.append((f"cut at {cut}", b"".join(pieces[:-1]) + last[:cut], None))
    return out, len(pieces)


def chunk_rows(chunks):
    """the spectra of a reader's chunks -> list of (identifier, precursor m/z, charge, retention time, (m/z base64, count, flags),
    (intensity base64, count, flags)), and the skipped counters summed"""
    rows, skipped = [], {}
    for c in chunks:
        for k, v in c.skipped.items():
            skipped[k] = skipped.get(k, 0) + v
        if not len(c):
            continue
        payload, arrays, spectra = c.tables()
        payload = payload.cpu().numpy() if hasattr(payload, "cpu") else np.asarray(payload)
        for i, (ma, ia) in enumerate(spectra):
            arr = tuple((payload[arrays[r, 0]:arrays[r, 0] + arrays[r, 1]].tobytes(), int(arrays[r, 2]), int(arrays[r, 3])) for r in (ma, ia))
            assert all(arrays[r, 0] % 8 == 0 for r in (ma, ia))
            rows.append((str(c.identifier[i]), float(c.precursor_mz[i]).hex(), c.precursor_charge[i] and int(c.precursor_charge[i]),
                         float(c.retention_time[i]).hex()) + arr)
    return rows, skipped


def size(path):
    return os.path.getsize(path)
