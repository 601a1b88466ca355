"""The device MGF reader (`Context.parse_mgf` = `fal_mgf_index` + `fal_mgf_parse`, and `mgf_io.read_chunks` on top of it) against
the host reader `mgf_io.get_spectra` + `falcon._raw_csr`: indptr, m/z, intensity, precursor m/z, charge and retention time bit
for bit, identifiers equal; exactly the expected spectra go back to the host reader; text outside the device grammar is read by
the host reader; malformed text never writes outside a slot; and the CLI gives byte-identical outputs with either reader."""
import ctypes as C
import io
import logging
import os

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io import mgf_io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---- corpus ----------------------------------------------------------------------------------------------------------------
def _number(rng, x, form=None):
    form = int(rng.integers(8)) if form is None else form
    if form == 0:
        return repr(float(x))
    if form == 1:
        return repr(float(np.float32(x)))
    if form == 2:
        return "%.4f" % x
    if form == 3:
        return "%.6e" % x
    if form == 4:
        return str(int(x))
    if form == 5:
        return "+" + repr(float(x))
    if form == 6:
        return ("%.3f" % (x % 1.0))[1:] if x % 1.0 >= 0.001 else "5."       # ".123", "5."
    return "%.6E" % x


def _clean_spectrum(rng, i, n_peaks=None, eol=None):
    """one spectrum inside the device grammar and inside the fast forms, as a list of lines without line ends"""
    sp = lambda: rng.choice(["", "", " ", "  ", "\t"])                       # noqa: E731
    n_peaks = int(rng.integers(0, 201)) if n_peaks is None else n_peaks
    title = rng.choice([f"scan={i}", f"run a={i} b = {i * 7}", f"{i}", f"spectrum {i} (x)  y"])
    head = [rng.choice(["TITLE=", "Title = ", "title\t=", "TITLE= "]) + title + sp(),
            rng.choice(["PEPMASS=", "pepmass = "]) + _number(rng, rng.uniform(300, 1500)) + rng.choice(["", " 1234.5", "\t7"])]
    if rng.integers(4):
        head.append("CHARGE=" + rng.choice(["2+", "3+", "1-", "2", "4+ "]))
    if rng.integers(4):
        head.append(rng.choice(["RTINSECONDS=", "rtinseconds= "]) + _number(rng, rng.uniform(0, 7200)))
    if rng.integers(3) == 0:
        head.append(f"SCANS={i}")
    if rng.integers(5) == 0:                                                  # duplicates: the last one wins
        head.insert(0, "TITLE=overwritten")
        head.insert(0, "PEPMASS=1.0")
        head.insert(0, "CHARGE=7+")
    order = rng.permutation(len(head)) if rng.integers(2) and "TITLE=overwritten" not in head else np.arange(len(head))
    head = [head[k] for k in order]
    mz = rng.uniform(100, 1500, n_peaks)
    if rng.integers(3):
        mz.sort()
    if n_peaks > 3 and rng.integers(2):
        mz[rng.integers(n_peaks)] = mz[rng.integers(n_peaks)]                 # tied m/z keep their input order
    # (the per-peak choices drawn at once: a generator call per peak and choice would dominate the test)
    pad = ["", "", " ", "  ", "\t"]
    forms, val = rng.integers(8, size=(n_peaks, 2)), rng.uniform(0.5, 1e6, n_peaks)
    pick = rng.integers(0, [20, 4, 6, 5, 5], size=(n_peaks, 5))       # second token?, separator, third column?, padding
    peaks = []
    for k, m in enumerate(mz):
        line = _number(rng, m, int(forms[k, 0]))
        if pick[k, 0]:
            line += [" ", "\t", "   ", " \t "][pick[k, 1]] + _number(rng, val[k], int(forms[k, 1]))
            if pick[k, 2] == 0:
                line += " 2+"
        peaks.append(pad[pick[k, 3]] + line + pad[pick[k, 4]])
    body = head + peaks
    if rng.integers(4) == 0:                                                  # a header behind the peaks
        body.append("USER03=late")
    for _ in range(int(rng.integers(3))):
        body.insert(int(rng.integers(len(body) + 1)), rng.choice(["", "# note", ";x", "!y", "/z", "   "]))
    return [sp() + "BEGIN IONS" + sp()] + body + [sp() + "END IONS" + sp()]


def _join(rng, lines, last_newline=True):
    out = "".join(l + ("\r\n" if rng.integers(3) == 0 else "\n") for l in lines)
    return out if last_newline else out.rstrip("\r\n")


def _corpus(n, seed, last_newline=False):
    rng = np.random.default_rng(seed)
    lines = ["# file header", "MASS=Monoisotopic", "COM=run 1", ""]
    for i in range(n):
        lines += _clean_spectrum(rng, i)
        if i < n - 1:
            lines += [rng.choice(["", "", "# between", "SEARCH=MIS"])] * int(rng.integers(3))
    return _join(rng, lines, last_newline).encode("ascii")


def _host(text: bytes):
    from falcon_amd.falcon import _raw_csr
    specs = list(mgf_io.get_spectra(io.StringIO(text.decode("ascii"))))
    return specs, _raw_csr(specs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _assert_specs(specs, csr, indptr, mz, it, ident, pmz, charge, rt):
    """device results (host arrays) == host reader's, bit for bit"""
    assert len(pmz) == len(specs)
    assert np.array_equal(indptr, csr[2])
    assert np.array_equal(_bits(mz), _bits(csr[0])) and mz.dtype == np.float64
    assert np.array_equal(_bits(it), _bits(csr[1])) and it.dtype == np.float32
    assert list(ident) == [s["identifier"] for s in specs]
    assert np.array_equal(_bits(pmz), _bits(np.array([s["precursor_mz"] for s in specs], np.float64)))
    assert np.array_equal(_bits(rt), _bits(np.array([s["retention_time"] for s in specs], np.float64)))
    assert list(charge) == [s["precursor_charge"] for s in specs]


def _assert_parse(text, res, specs, csr, rows=None):
    """a parse_mgf result (its rows `rows`, default all) == the host reader's spectra"""
    rows = np.arange(len(res["status"])) if rows is None else rows
    ip = res["indptr"].cpu().numpy()
    assert ip[0] == 0
    mz, it = res["mz"].cpu().numpy(), res["intensity"].cpu().numpy()
    pos = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    sub = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(ip[rows + 1] - ip[rows], out=sub[1:])
    ident = [text[a:b].decode("ascii") for a, b in res["title"][rows]]
    charge = [int(c) if h else None for c, h in zip(res["charge"][rows], res["has_charge"][rows])]
    _assert_specs(specs, csr, sub, mz[pos], it[pos], ident, res["precursor_mz"][rows], charge, res["retention_time"][rows])


def _read(ctx, path, **kw):
    """mgf_io.read_chunks of a file -> host arrays of all its spectra (dropped rows removed), chunks"""
    chunks = list(mgf_io.read_chunks(path, ctx, **kw))
    cols = dict(sizes=[], mz=[], it=[], ident=[], pmz=[], charge=[], rt=[])
    for c in chunks:
        ip = c.indptr.cpu().numpy() if hasattr(c.indptr, "cpu") else c.indptr
        mz = c.mz.cpu().numpy() if hasattr(c.mz, "cpu") else c.mz
        it = c.intensity.cpu().numpy() if hasattr(c.intensity, "cpu") else c.intensity
        keep = np.flatnonzero(~c.dropped)
        pos = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in keep]) if len(keep) else np.zeros(0, np.int64)
        cols["sizes"].append(ip[keep + 1] - ip[keep])
        cols["mz"].append(mz[pos])
        cols["it"].append(it[pos])
        cols["ident"] += list(c.identifier[keep])
        cols["pmz"].append(c.precursor_mz[keep])
        cols["charge"].append(c.precursor_charge[keep])
        cols["rt"].append(c.retention_time[keep])
    cat = lambda k, dt: np.concatenate(cols[k]).astype(dt, copy=False) if cols[k] else np.zeros(0, dt)        # noqa: E731
    sizes = cat("sizes", np.int64)
    indptr = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=indptr[1:])
    return dict(indptr=indptr, mz=cat("mz", np.float64), it=cat("it", np.float32), ident=cols["ident"], pmz=cat("pmz", np.float64),
                charge=cat("charge", np.int32), rt=cat("rt", np.float64)), chunks


def _assert_read(got, specs, csr):
    charge = [s["precursor_charge"] if s["precursor_charge"] else 0 for s in specs]          # (None and 0: both "unknown" downstream)
    _assert_specs(specs, csr, got["indptr"], got["mz"], got["it"], got["ident"], got["pmz"],
                  [None if s["precursor_charge"] is None else int(c) for c, s in zip(got["charge"], specs)], got["rt"])
    assert list(got["charge"]) == charge


@pytest.fixture(scope="module")
def clean():
    text = _corpus(2000, 7)
    specs, csr = _host(text)
    assert len(specs) == 2000 and not text.endswith(b"\n") and b"\r\n" in text and b"\t" in text
    return text, specs, csr


# ---- 1. randomised clean corpus ---------------------------------------------------------------------------------------------
def test_clean_corpus_equals_the_host_reader(ctx, clean):
    text, specs, csr = clean
    res = ctx.parse_mgf(text)
    assert res["flags"] == 0 and res["lines"] == text.count(b"\n") + 1
    assert not res["status"].any()
    _assert_parse(text, res, specs, csr)
    # the whole spectrum's byte range: from BEGIN IONS to the end of its END IONS line
    for a, b in res["span"][[0, 1, 999, 1999]]:
        seg = text[a:b].strip()
        assert seg.startswith(b"BEGIN IONS") and seg.endswith(b"END IONS") and seg.count(b"BEGIN IONS") == 1
    assert res["span"][-1][1] == len(text)


# ---- 2. HOST and structural cases -----------------------------------------------------------------------------------------
def _s(title, *lines, pep="PEPMASS=500.5", end=True):
    return "\n".join(["BEGIN IONS"] + ([f"TITLE={title}"] if title else []) + ([pep] if pep else []) + list(lines) +
                     (["END IONS"] if end else [])) + "\n"


# (text, statuses of the spectra the device emits for it, how many of those the host reader accepts)
CASES = [
    (_s("nan", "100.0 1", "nan 2", "300.0 3"), [1], 1),
    (_s("underscore", "1_0 5", "20.5 1"), [1], 1),
    (_s("charges", "CHARGE=2+ and 3+", "100.0 1"), [1], 1),
    (_s(None, "100.0 1"), [1], 0),
    (_s("no pepmass", "100.0 1", pep=None), [1], 0),
    (_s("empty pepmass", "100.0 1", pep="PEPMASS="), [1], 0),
    (_s("text peak", "100.0 1", "abc def"), [1], 0),
    (_s("25 digits", "1234567890123456789012345e-22 4", "200.0 1"), [1], 1),
    (_s("rt range", "RTINSECONDS=12-13", "100.0 1"), [1], 0),
    (_s("outer", "100.0 1", end=False) + _s("inner", "200.0 2"), [0], 1),
    ("END IONS\n", [], 0),
    (_s("no peaks"), [0], 1),
    (_s("exponent", "1e40 1"), [1], 1),
    (_s("one token", "123.25"), [0], 1),
    (_s("equals in peak", "1.5=3"), [1], 0),
    (_s("plus key", "+1.5=2", "100.0 1"), [0], 1),
]


def _spliced():
    rng = np.random.default_rng(11)
    parts, want = [], []
    for k, (case, status, _) in enumerate(CASES):
        for j in range(2):
            parts.append(_join(rng, _clean_spectrum(rng, 100 * k + j, n_peaks=int(rng.integers(0, 70)))))
            want.append(0)
        parts.append(case)
        want += status
    parts.append(_join(rng, _clean_spectrum(rng, 9999, n_peaks=5)))
    want.append(0)
    parts.append(_s("unterminated", "100.0 1", end=False))                    # dropped, by both readers
    return "".join(parts).encode("ascii"), np.array(want, np.int32)


def test_host_and_structural_cases(ctx, tmp_path):
    text, want = _spliced()
    specs, csr = _host(text)
    assert len(specs) == 2 * len(CASES) + 1 + sum(c[2] for c in CASES)
    res = ctx.parse_mgf(text)
    assert res["flags"] == 0
    assert np.array_equal(res["status"], want * _lib.MGF_ST_HOST)
    # the spectra the device decided are the host reader's, untouched by their neighbours
    decided = np.flatnonzero(res["status"] == 0)
    ids = [text[a:b].decode() for a, b in res["title"][decided]]
    by_id = {s["identifier"]: s for s in specs}
    from falcon_amd.falcon import _raw_csr
    sub = [by_id[i] for i in ids]
    _assert_parse(text, res, sub, _raw_csr(sub), rows=decided)
    # a HOST spectrum's slot has the size of its peak lines
    ip = res["indptr"].cpu().numpy()
    host_rows = np.flatnonzero(res["status"] != 0)
    assert list(np.diff(ip)[host_rows][:3]) == [3, 2, 1]
    path = tmp_path / "cases.mgf"
    path.write_bytes(text)
    got, chunks = _read(ctx, str(path))
    assert len(chunks) == 1 and chunks[0].reader == "device" and chunks[0].n_host == int(want.sum())
    assert int(chunks[0].dropped.sum()) == int(want.sum()) - sum(c[2] for c in CASES if c[1] == [1])
    _assert_read(got, specs, csr)
    assert np.isnan(got["mz"]).sum() == 1


# ---- 3. grammar flag --------------------------------------------------------------------------------------------------------
def _outcome(fn):
    try:
        return "ok", fn()
    except Exception as e:          # noqa: BLE001 -- the readers must fail alike
        return type(e).__name__, None


@pytest.mark.parametrize("what,old,new", [("non-ascii", b"TITLE=scan=6", "TITLE=scan=6 é".encode("utf-8")),
                                          ("lone CR", b"TITLE=scan=6", b"TITLE=scan=6\rSCANS=1"), ("form feed", b"TITLE=scan=6", b"TITLE=scan=6\x0c")])
def test_text_outside_the_grammar_is_the_host_readers(ctx, tmp_path, what, old, new):
    rng = np.random.default_rng(5)
    lines = []
    for i in range(8):
        lines += ["BEGIN IONS", f"TITLE=scan={i}", "PEPMASS=400.25", "CHARGE=2+"] + [f"{100 + 7 * k}.5 {k + 1}" for k in range(6)] + ["END IONS"]
    text = _join(rng, lines).encode("ascii")
    assert text.count(old) == 1
    bad = text.replace(old, new)
    assert ctx.parse_mgf(text)["flags"] == 0
    assert ctx.parse_mgf(bad)["flags"] & _lib.MGF_FLAG_BYTES
    path = tmp_path / "bad.mgf"
    path.write_bytes(bad)
    from falcon_amd.falcon import _raw_csr
    want = _outcome(lambda: list(mgf_io.get_spectra(str(path))))
    got = _outcome(lambda: _read(ctx, str(path), max_bytes=600))                # the flagged stretch is not the first one
    assert got[0] == want[0]
    if want[0] == "ok":
        assert len(want[1]) == 8 and got[1][1][-1].reader == "host" and got[1][1][0].reader == "device"
        _assert_read(got[1][0], want[1], _raw_csr(want[1]))


def test_a_cr_at_the_end_of_the_text_is_outside_the_grammar(ctx):
    assert ctx.parse_mgf(b"BEGIN IONS\nEND IONS\r")["flags"] & _lib.MGF_FLAG_BYTES
    assert ctx.parse_mgf(b"\n" * 4000)["flags"] & _lib.MGF_FLAG_LINES            # more than one line per 4 bytes
    assert ctx.parse_mgf(b"BEGIN IONS\r\nEND IONS\r\n")["flags"] == 0


# ---- 4. edge shapes ---------------------------------------------------------------------------------------------------------
def test_empty_and_single(ctx, tmp_path):
    res = ctx.parse_mgf(b"")
    assert res["flags"] == 0 and len(res["status"]) == 0 and res["indptr"].cpu().tolist() == [0]
    res = ctx.parse_mgf(b"# nothing here\n\nPEPMASS=3\n")
    assert len(res["status"]) == 0
    text = _s("only", "CHARGE=3+", "RTINSECONDS=77.5", "200.5 3", "100.25 1").encode()
    specs, csr = _host(text)
    res = ctx.parse_mgf(text)
    assert list(res["status"]) == [0]
    _assert_parse(text, res, specs, csr)
    assert res["mz"].cpu().tolist() == [100.25, 200.5] and res["intensity"].cpu().tolist() == [1.0, 3.0]
    path = tmp_path / "empty.mgf"
    path.write_bytes(b"")
    assert list(mgf_io.read_chunks(str(path), ctx)) == []


def test_one_spectrum_of_20000_peaks_with_every_line_length(ctx):
    rng = np.random.default_rng(3)
    mz = np.sort(rng.uniform(50, 5000, 20000))
    mz[5000:5040] = mz[5000:5040][::-1]                                        # a stretch out of order: the ranking path
    lines = []
    for k, m in enumerate(mz):
        lines.append(" " * int(rng.integers(0, 40)) + _number(rng, m) + " " * int(rng.integers(1, 30)) + _number(rng, 1 + k % 977) +
                     "\t" * int(rng.integers(0, 9)))
    text = _join(rng, ["BEGIN IONS", "TITLE=big", "PEPMASS=777.125"] + lines + ["END IONS"]).encode()
    specs, csr = _host(text)
    res = ctx.parse_mgf(text)
    assert list(res["status"]) == [0] and res["indptr"].cpu().tolist() == [0, 20000]
    _assert_parse(text, res, specs, csr)


def test_a_10000_character_title_is_parsed_or_left_to_the_host(ctx, tmp_path):
    rng = np.random.default_rng(4)
    text = (_join(rng, _clean_spectrum(rng, 1, 9)) + _s("t" * 10000, "100.5 2") + _s("x" * 4000, "100.5 2") +
            _join(rng, _clean_spectrum(rng, 2, 9))).encode()
    specs, csr = _host(text)
    res = ctx.parse_mgf(text)
    assert list(res["status"]) == [0, _lib.MGF_ST_HOST, 0, 0]                   # (longer than the kernels' 4096-byte line limit)
    path = tmp_path / "title.mgf"
    path.write_bytes(text)
    got, _ = _read(ctx, str(path))
    _assert_read(got, specs, csr)
    assert got["ident"][1] == "t" * 10000 and got["ident"][2] == "x" * 4000


# ---- 5. chunking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("oversized", [False, True])
def test_chunked_reading_equals_one_chunk(ctx, tmp_path, oversized):
    rng = np.random.default_rng(9)
    lines = []
    for i in range(200):
        lines += _clean_spectrum(rng, i, n_peaks=int(rng.integers(0, 40)) if not (oversized and i == 120) else 600) + ["", "# gap END IONS"]
    text = _join(rng, lines).encode()
    specs, csr = _host(text)
    assert len(specs) == 200
    path = tmp_path / "chunks.mgf"
    path.write_bytes(text)
    one, chunks1 = _read(ctx, str(path))
    many, chunks = _read(ctx, str(path), max_bytes=4096)
    assert len(chunks1) == 1 and len(chunks) > 10 and all(c.reader == "device" and c.n_host == 0 for c in chunks)
    _assert_read(one, specs, csr)
    _assert_read(many, specs, csr)


# ---- 6. guarded outputs -----------------------------------------------------------------------------------------------------
def _guarded_parse(ctx, text: bytes, guard=256):
    """fal_mgf_index + fal_mgf_parse with every output followed by 0xA5 bytes -> (counts, all guards intact?)"""
    import torch
    d_text = ctx.to_dev(np.frombuffer(bytearray(text), np.uint8)) if text else ctx.empty((0,), torch.uint8)
    n, nnz, flags, _ = ctx.mgf_index(d_text)
    sizes = dict(indptr=8 * (n + 1), mz=8 * nnz, it=4 * nnz, pmz=8 * n, charge=4 * n, has=4 * n, rt=8 * n, title=16 * n, span=16 * n, status=4 * n)
    bufs = {k: torch.full((v + guard,), 0xA5, dtype=torch.uint8, device=ctx.tdev) for k, v in sizes.items()}
    p = {k: C.c_void_p(b.data_ptr()) for k, b in bufs.items()}
    _lib.check(ctx.lib.fal_mgf_parse(ctx._h, C.c_void_p(d_text.data_ptr()) if text else None, len(text), n, nnz, p["indptr"], p["mz"],
                                     p["it"], p["pmz"], p["charge"], p["has"], p["rt"], p["title"], p["span"], p["status"]), "fal_mgf_parse")
    ctx.sync()
    intact = all(bool((b[sizes[k]:] == 0xA5).all().item()) for k, b in bufs.items())
    indptr = bufs["indptr"][:sizes["indptr"]].view(torch.int64).cpu().numpy()
    return (n, nnz, flags), intact, indptr


def test_malformed_text_never_writes_outside_a_slot(ctx, clean):
    text = clean[0]
    rng = np.random.default_rng(1)
    garbage = bytes(rng.choice(np.frombuffer(b"BEGIN IONS\nEND IONS\n=.+-e0123456789 \t\r\nTITLE=PEPMASS=x", np.uint8), 30000))
    words = [b"BEGIN IONS\n", b"END IONS\n", b"1.5 2\n", b"TITLE=\n", b"PEPMASS=\n", b"=\n", b"9" * 30 + b"\n", b"\n", b"CHARGE=+\n", b"1e999 .\n"]
    soup = b"".join(words[k] for k in rng.integers(0, len(words), 6000))
    for t in (text[:len(text) // 2 - 3], text[7:50001], garbage, soup, b"BEGIN IONS", b"END IONS\n" * 50, b"BEGIN IONS\n" * 50 + b"END IONS"):
        (n, nnz, flags), intact, indptr = _guarded_parse(ctx, t)
        assert intact
        assert indptr[0] == 0 and indptr[-1] == nnz and (np.diff(indptr) >= 0).all()
        if not flags:                                  # inside the grammar: still the host reader's structure
            res = ctx.parse_mgf(t)
            keep = res["status"] == 0
            specs = list(mgf_io.get_spectra(io.StringIO(t.decode("ascii"))))
            assert keep.sum() <= len(specs) <= len(keep)


def test_parse_refuses_a_text_it_did_not_index(ctx):
    import torch
    a, b = ctx.to_dev(np.frombuffer(bytearray(_s("a", "1 2").encode()), np.uint8)), ctx.to_dev(np.frombuffer(bytearray(b"# other text\n"), np.uint8))
    n, nnz, _, _ = ctx.mgf_index(a)
    assert (n, nnz) == (1, 1)
    with pytest.raises(_lib.FalconHipError, match="fal_mgf_index"):
        ctx.mgf_parse(b, n, nnz)
    out = ctx.mgf_parse(a, n, nnz)
    assert out[0].cpu().tolist() == [0, 1] and torch.equal(out[1].cpu(), torch.tensor([1.0], dtype=torch.float64))


# ---- 7. CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_outputs_do_not_depend_on_the_reader(tmp_path, caplog):
    from falcon_amd import synth
    from falcon_amd.falcon import main
    from falcon_amd.ms_io import ms_io
    d = synth.generate(1500, seed=5)
    specs = []
    for i in range(1500):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        specs.append({"identifier": f"scan={i}", "precursor_mz": float(d["precursor_mz"][i]), "precursor_charge": int(d["precursor_charge"][i]),
                      "retention_time": float(d["retention_time"][i]), "mz": d["mz"][a:b].astype(np.float64), "intensity": d["intensity"][a:b]})
    mgf = str(tmp_path / "in.mgf")
    ms_io.write_spectra(mgf, specs)
    with open(mgf, "a") as f:                         # a low-quality spectrum, one for the host reader, and one it rejects
        f.write(_s("short", "CHARGE=2+", "100.0 1") + _s("host", "CHARGE=2+ and 3+", *[f"{150 + 40 * k}.25 {k + 1}" for k in range(12)]) +
                _s("rejected", "abc"))
    outs, counts = {}, {}
    for reader in ("device", "host"):
        out = str(tmp_path / f"res_{reader}")
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="falcon"):
            assert main([mgf, out, "--eps", "0.3", "--export_representatives", "--work_dir", str(tmp_path / f"work_{reader}")] +
                        ([] if reader == "device" else ["--mgf_reader", "host"])) == 0
        msgs = [r.getMessage() for r in caplog.records]
        counts[reader] = [m for m in msgs if m.startswith("Read ") and "spectra from" in m and "peak files" in m] + \
                         [m for m in msgs if m.startswith("Skipped ") and "low-quality" in m]
        assert f"mgf_reader = {reader}" in msgs
        assert any("parsed on the device" in m for m in msgs) == (reader == "device")
        outs[reader] = (open(out + ".csv", "rb").read().replace(f"work_{reader}".encode(), b"work"), open(out + ".mgf", "rb").read())
    assert len(counts["device"]) == 2 and counts["device"] == counts["host"]
    assert outs["device"][0] == outs["host"][0] and outs["device"][1] == outs["host"][1]
    assert b"mgf_reader" not in outs["device"][0] and b",host," in outs["device"][0]
