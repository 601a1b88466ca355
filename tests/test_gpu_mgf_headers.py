"""`fal_mgf_headers`, `fal_text_rows` and `fal_mgf_parse_ex` at the C ABI against a plain Python restatement of the key rule, and the
library / representative readers and loaders on top of them against the host readers that were there before: every field equal,
floats by their bits, the same first error, byte-identical CLI outputs under either reader."""
import ctypes as C
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io import mgf_io
from tests import mgf_library_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
SPAN, INT = _lib.MGF_KEY_SPAN, _lib.MGF_KEY_INT
ABSENT, PRESENT, HOST = _lib.MGF_KEY_ABSENT, _lib.MGF_KEY_PRESENT, _lib.MGF_KEY_HOST


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------
def expected_headers(text: bytes, keys: dict):
    """the host readers' line loop over `text` -> span i64[n, k, 2], value i64[n, k], state i32[n, k] as fal_mgf_headers states them"""
    names = list(keys)
    out, cur, inside, pos = [], None, False, 0
    for raw in text.split(b"\n"):
        start, pos = pos, pos + len(raw) + 1
        line = raw.strip(b" \t\r\n")
        if not line or line[:1] in (b"#", b";", b"!", b"/"):
            continue
        if line == b"BEGIN IONS":
            cur, inside = {}, True
        elif line == b"END IONS":
            if inside:
                out.append(cur)
            inside = False
        elif inside and b"=" in line and not (line[:1].isdigit() or line[:1] == b"."):
            k, v = line.split(b"=", 1)
            k = k.strip(b" \t\r\n").lower().decode("ascii")
            if k in keys:
                lo = start + raw.index(b"=") + 1 + (len(v) - len(v.lstrip(b" \t\r\n")))
                cur[k] = (lo, lo + len(v.strip(b" \t\r\n")), len(line) > 4096)
    n = len(out)
    span, value, state = np.zeros((n, len(names), 2), np.int64), np.zeros((n, len(names)), np.int64), np.zeros((n, len(names)), np.int32)
    for s, found in enumerate(out):
        for j, k in enumerate(names):
            if k not in found:
                continue
            lo, hi, long = found[k]
            span[s, j] = lo, hi
            state[s, j] = PRESENT
            if long:
                state[s, j] = HOST
            elif keys[k] == INT and hi > lo:
                if re.fullmatch(rb"[+-]?[0-9]{1,18}", text[lo:hi]):
                    value[s, j] = int(text[lo:hi])
                else:
                    state[s, j] = HOST
    return span, value, state


def _text_dev(ctx, text: bytes):
    import torch
    return ctx.to_dev(np.frombuffer(bytearray(text), np.uint8)) if text else ctx.empty((0,), torch.uint8)


def _key_args(keys: dict):
    raw = [k.encode("ascii") for k in keys]
    ptr = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=ptr[1:])
    blob = np.frombuffer(b"".join(raw) + b"\0", np.uint8).copy()
    kinds = np.array(list(keys.values()) + [0], np.int32)
    return blob, ptr, kinds


def _guarded(ctx, sizes: dict):
    import torch
    bufs = {k: torch.full((v + GUARD,), 0xA5, dtype=torch.uint8, device=ctx.tdev) for k, v in sizes.items()}
    return bufs, {k: C.c_void_p(b.data_ptr()) for k, b in bufs.items()}


def _intact(bufs, sizes):
    return all(bool((b[sizes[k]:] == 0xA5).all().item()) for k, b in bufs.items())


def headers_rc(ctx, d_text, n_bytes, n, keys: dict):
    """fal_mgf_headers with every output followed by 0xA5 bytes -> (return code, span, value, state, guards intact and -- after
    an error -- nothing written at all)"""
    import torch
    k = len(keys)
    blob, ptr, kinds = _key_args(keys)
    sizes = dict(span=16 * n * k, value=8 * n * k, state=4 * n * k)
    bufs, p = _guarded(ctx, sizes)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)                              # noqa: E731
    rc = ctx.lib.fal_mgf_headers(ctx._h, C.c_void_p(d_text.data_ptr()) if n_bytes else None, n_bytes, n, as_p(blob), as_p(ptr), as_p(kinds), k,
                                 p["span"], p["value"], p["state"])
    ctx.sync()
    intact = _intact(bufs, sizes) if rc == 0 else all(bool((b == 0xA5).all().item()) for b in bufs.values())
    span = bufs["span"][:sizes["span"]].view(torch.int64).cpu().numpy().reshape(n, k, 2)
    value = bufs["value"][:sizes["value"]].view(torch.int64).cpu().numpy().reshape(n, k)
    state = bufs["state"][:sizes["state"]].view(torch.int32).cpu().numpy().reshape(n, k)
    return rc, span, value, state, intact


def check_headers(ctx, text: bytes, keys: dict, n_want=None):
    d_text = _text_dev(ctx, text)
    n, _, flags, _ = ctx.mgf_index(d_text)
    want = expected_headers(text, keys)
    assert flags == 0 and n == len(want[0]) and (n_want is None or n == n_want)
    rc, span, value, state, intact = headers_rc(ctx, d_text, len(text), n, keys)
    assert rc == 0 and intact
    assert np.array_equal(state, want[2])
    assert np.array_equal(span, want[0])
    assert np.array_equal(value, want[1])
    return span, value, state


LIB_KEYS = {k: SPAN for k in mgf_io.LIBRARY_KEYS}
PEAKS = [f"{100 + k}.5 {k + 1}" for k in range(200)]


def _spec(lines):
    return "\n".join(["BEGIN IONS", "PEPMASS=500.5"] + list(lines) + ["END IONS", ""]) + "\n"


def _at(pos, line, total=None, filler=PEAKS):
    """a spectrum whose line `pos` behind BEGIN IONS (from 0) is `line`, filler lines around it"""
    total = pos + 3 if total is None else total
    body = [filler[k % len(filler)] for k in range(total)]
    body[pos - 1] = line                                # (PEPMASS is line 0)
    return _spec(body)


def spliced_text():
    parts = [_at(p, f"NAME=at line {p}") for p in (61, 62, 63, 64, 65, 127, 128, 129)]
    parts.append(_spec(["NAME=first turn", "SMILES=only in the first turn"] + PEAKS[:70] + ["name = second turn wins ", "ADDUCT=only in the second"]))
    parts.append(_spec(["NAME=kept: the later turns hold no key"] + PEAKS[:150]))
    wide = ["# " + "x" * 98] * 40                                                 # 64 lines of more than 4096 bytes: not staged
    parts.append(_spec(wide + ["INCHIKEY=among wide lines", "SMILES=C=O"] + wide + ["NAME=behind them"]))
    parts.append(_spec(["NAME=" + "x" * 4091, "SMILES=short"]))                        # 4096 bytes: the longest line the kernels take
    parts.append(_spec(["NAME=" + "x" * 4092, "SMILES=short"]))                        # 4097: the host's
    parts.append(_spec(["NAME=" + "x" * 4092, "NAME=the last one is short"]))
    parts.append(_spec(["NAME=", "SMILES= ", "ADDUCT=\t", "NAMES=no", "1=2", "=x"]))
    parts.append(_spec(PEAKS[:5]))
    parts.append(_spec([f"{k.upper()} = value of {k}" for k in mgf_io.LIBRARY_KEYS]))
    parts.append("BEGIN IONS\nNAME=lost with the unterminated entry\n" + _spec(["SPECTRUMID=inner"]))
    parts.append("NAME=outside an entry\n" + _spec(["# NAME=comment", "IONMODE=Positive"]))
    return "".join(parts).encode("ascii")


def check_spliced(ctx):
    text = spliced_text()
    span, value, state = check_headers(ctx, text, LIB_KEYS)
    name = list(LIB_KEYS).index("name")
    got = [text[a:b].decode() if st != ABSENT else None for (a, b), st in zip(span[:, name], state[:, name])]
    assert got[:8] == [f"at line {p}" for p in (61, 62, 63, 64, 65, 127, 128, 129)] and got[8] == "second turn wins"
    assert got[10] == "behind them" and state[11, name] == PRESENT and state[12, name] == HOST and state[13, name] == PRESENT
    assert got[14] == "" and state[14, name] == PRESENT and not state[15].any() and (state[16] == PRESENT).all()
    assert got[17] is None and got[18] is None
    # one key, and an INT key beside SPAN keys
    check_headers(ctx, text, {"name": SPAN})
    ints = ["0", "007", "-3", "+7", "9" * 18, "9" * 19, "-0", "", "1_0", "1 2", "+", "0x5", " 12 ", "5\r"]
    text = "".join(_spec([f"CLUSTER={v}", f"NAME=n{j}"] + ([] if j % 3 else ["cluster = 44"])) for j, v in enumerate(ints)).encode("ascii")
    _, value, state = check_headers(ctx, text, {"cluster": INT, "name": SPAN}, len(ints))
    assert list(value[:, 0]) == [44, 7, -3, 44, 10 ** 18 - 1, 0, 44, 0, 0, 44, 0, 0, 44, 5]
    assert list(state[:, 0]) == [1, 1, 1, 1, 1, 2, 1, 1, 2, 1, 2, 2, 1, 1]


def check_sixteen_keys(ctx):
    keys = {f"key{j:02d}": (INT if j % 2 else SPAN) for j in range(15)}
    keys["k" * 32] = SPAN
    rng = np.random.default_rng(5)
    parts = []
    for s in range(40):
        lines = [f"{k.upper() if s % 2 else k}={j * 100 + s}" for j, k in enumerate(keys) if s == 0 or rng.integers(3)]
        lines = [lines[i] for i in rng.permutation(len(lines))] + PEAKS[:int(rng.integers(0, 90))]
        parts.append(_spec(lines))
    _, _, state = check_headers(ctx, "".join(parts).encode("ascii"), keys)
    assert (state[0] == PRESENT).all() and (state == ABSENT).any()


def check_sizes(ctx):
    for n in (1, 255, 256, 257, 1025, 16389):                                    # block turns; past 16384 a wave takes a second spectrum
        text = "".join(_spec([f"NAME=n{s}"] + ([f"SMILES=C{s}"] if s % 3 else []) + PEAKS[:s % 4]) for s in range(n)).encode("ascii")
        check_headers(ctx, text, {"smiles": SPAN, "name": SPAN}, n)
    for text in (b"", b"# nothing\nNAME=x\n"):
        d_text = _text_dev(ctx, text)
        n, _, flags, _ = ctx.mgf_index(d_text)
        assert (n, flags) == (0, 0)
        rc, span, _, _, intact = headers_rc(ctx, d_text, len(text), 0, LIB_KEYS)
        assert rc == 0 and intact and span.shape == (0, 7, 2)


def check_bad_arguments(ctx):
    text = _spec(["NAME=a"]).encode()
    d_text, other = _text_dev(ctx, text), _text_dev(ctx, b"# other text\n")
    n = ctx.mgf_index(d_text)[0]
    assert n == 1
    bad = [{f"key{j}": SPAN for j in range(17)}, {"k" * 33: SPAN}, {"title": SPAN}, {"name": SPAN, "pepmass": SPAN}, {"Name": SPAN},
           {"name": 2}, {"name": SPAN, "smiles": SPAN, "name ": SPAN}, {"a=b": SPAN}]
    for keys in bad:
        rc, *_, untouched = headers_rc(ctx, d_text, len(text), n, keys)
        assert rc == _lib.FAL_EINVAL and untouched, keys
    assert headers_rc(ctx, d_text, len(text), n, {})[0] == _lib.FAL_EINVAL
    for args in ((other, len(text), n), (d_text, len(text) - 1, n), (d_text, len(text), n + 1)):
        rc, *_, untouched = headers_rc(ctx, *args, {"name": SPAN})
        assert rc == _lib.FAL_EINVAL and untouched and b"fal_mgf_index" in ctx.lib.fal_last_error()
    rc, span, _, state, intact = headers_rc(ctx, d_text, len(text), n, {"name": SPAN})          # the index is still good
    assert rc == 0 and intact and state[0, 0] == PRESENT and text[span[0, 0, 0]:span[0, 0, 1]] == b"a"
    ctx.trim()
    rc, *_, untouched = headers_rc(ctx, d_text, len(text), n, {"name": SPAN})
    assert rc == _lib.FAL_EINVAL and untouched
    with pytest.raises(_lib.FalconHipError):
        ctx.mgf_headers(d_text, n, ["name"])
    n, nnz = ctx.mgf_index(d_text)[:2]                                           # before fal_mgf_parse, and behind it
    first = [t.cpu().numpy() for t in ctx.mgf_headers(d_text, n, ["name"])]
    ctx.mgf_parse(d_text, n, nnz)
    again = [t.cpu().numpy() for t in ctx.mgf_headers(d_text, n, ["name"])]
    assert all(np.array_equal(a, b) for a, b in zip(first, again)) and first[2][0, 0] == PRESENT


def test_headers_on_spliced_spectra(ctx):
    check_spliced(ctx)


def test_headers_with_all_sixteen_keys(ctx):
    check_sixteen_keys(ctx)


def test_headers_at_the_block_and_grid_turns(ctx):
    check_sizes(ctx)


def test_headers_refuse_bad_tables_and_foreign_texts(ctx):
    check_bad_arguments(ctx)


def test_headers_on_malformed_text_stay_inside_their_outputs(ctx):
    rng = np.random.default_rng(1)
    words = [b"BEGIN IONS\n", b"END IONS\n", b"1.5 2\n", b"NAME=\n", b"name = x\n", b"=\n", b"SMILES" * 9 + b"\n", b"\n", b"NAME\n", b"NAME=" + b"y" * 5000 + b"\n"]
    soup = b"".join(words[k] for k in rng.integers(0, len(words), 4000))
    garbage = bytes(rng.choice(np.frombuffer(b"BEGIN IONS\nEND IONS\n= NAMEname\t\r\n", np.uint8), 20000))
    for t in (soup, garbage, b"BEGIN IONS\nNAME=x", b"BEGIN IONS\n" * 40 + b"NAME=x\nEND IONS", b"END IONS\n" * 40):
        d_text = _text_dev(ctx, t)
        n, _, flags, _ = ctx.mgf_index(d_text)
        if flags:
            continue
        rc, span, _, state, intact = headers_rc(ctx, d_text, len(t), n, {"name": SPAN, "smiles": INT})
        assert rc == 0 and intact
        want = expected_headers(t, {"name": SPAN, "smiles": INT})
        assert np.array_equal(state, want[2]) and np.array_equal(span, want[0])


# ---- fal_text_rows ----------------------------------------------------------------------------------------------------------------
def rows_rc(ctx, d_text, n_bytes, span: np.ndarray, column, width):
    import torch
    n = len(span)
    stride = span.shape[1] if span.ndim == 3 else 1
    sizes = dict(rows=n * width, long=4 * n)
    bufs, p = _guarded(ctx, sizes)
    d_span = ctx.to_dev(np.ascontiguousarray(span, np.int64)) if n else ctx.empty((1,), torch.int64)
    rc = ctx.lib.fal_text_rows(ctx._h, C.c_void_p(d_text.data_ptr()) if n_bytes else None, n_bytes, C.c_void_p(d_span.data_ptr()), stride, column,
                               n, width, p["rows"], p["long"])
    ctx.sync()
    rows = bufs["rows"][:sizes["rows"]].cpu().numpy().reshape(n, width)
    long = bufs["long"][:sizes["long"]].view(torch.int32).cpu().numpy()
    return rc, rows, long, _intact(bufs, sizes)


def check_text_rows(ctx):
    rng = np.random.default_rng(2)
    text = bytes(rng.integers(0x21, 0x7F, 5003).astype(np.uint8))
    d_text = _text_dev(ctx, text)
    nb = len(text)
    for width in (1, 16, 17, 256):
        for n in (0, 1, 257):
            size = np.array([[0, width, width + 1, 1, width - 1 if width > 1 else 0, 3 * width][k % 6] for k in range(n)], np.int64)
            lo = rng.integers(0, nb - 3 * width, n)                              # (any alignment)
            lo[::5] |= 1
            if n:
                lo[-1] = nb - size[-1]                                            # the last range ends with the text
            span = np.zeros((n, 3, 2), np.int64)
            span[:, 1, 0], span[:, 1, 1] = lo, lo + size
            span[:, 0], span[:, 2] = -7, nb + 99                                  # the other columns are never read
            rc, rows, long, intact = rows_rc(ctx, d_text, nb, span, 1, width)
            assert rc == 0 and intact, (width, n)
            want = np.zeros((n, width), np.uint8)
            for k in range(n):
                part = text[lo[k]:lo[k] + min(size[k], width)]
                want[k, :len(part)] = np.frombuffer(part, np.uint8)
            assert np.array_equal(rows, want) and np.array_equal(long, (size > width).astype(np.int32)), (width, n)
    # ranges outside the text: a zero row each, FAL_EINVAL behind the launch, the good rows written
    span = np.array([[0, 4], [-1, 3], [nb - 2, nb + 1], [9, 5], [nb, nb], [nb - 4, nb]], np.int64)
    rc, rows, long, intact = rows_rc(ctx, d_text, nb, span, 0, 4)
    assert rc == _lib.FAL_EINVAL and intact and b"outside the text" in ctx.lib.fal_last_error()
    assert rows.tolist() == [list(text[:4]), [0] * 4, [0] * 4, [0] * 4, [0] * 4, list(text[-4:])] and not long.any()
    for width, column in ((0, 0), (257, 0), (4, 1), (4, -1)):
        rc, rows, _, intact = rows_rc(ctx, d_text, nb, span[:1], column, width)
        assert rc == _lib.FAL_EINVAL and intact and (rows == 0xA5).all()
    # the Python layer: strings of a column, the long ones from the host's copy
    spans = np.array([[0, 5], [10, 10], [20, 20 + 300], [nb - 256, nb]], np.int64)
    assert list(mgf_io._text_column(ctx, text, d_text, spans)) == [text[a:b].decode() for a, b in spans]


def test_text_rows(ctx):
    check_text_rows(ctx)


# ---- fal_mgf_parse_ex -----------------------------------------------------------------------------------------------------------
def _parse_corpus():
    """random spectra inside the device grammar in several header and number forms, every fourth without TITLE, and some the host
    reader decides whatever the option says"""
    rng = np.random.default_rng(23)
    num = lambda x: [repr(float(x)), "%.4f" % x, "%.6e" % x, str(int(x)), "+" + repr(float(x))][int(rng.integers(5))]      # noqa: E731
    parts, titled, clean = [], [], []
    for i in range(400):
        head = [rng.choice(["PEPMASS=", "pepmass = "]) + num(rng.uniform(300, 1500)) + rng.choice(["", " 1234.5"])]
        if i % 4:
            head.append(rng.choice(["TITLE=", "Title = "]) + f"scan {i} x={i}")
        if rng.integers(3):
            head.append("CHARGE=" + rng.choice(["2+", "3+", "1-", "2"]))
        if rng.integers(3):
            head.append("RTINSECONDS=" + num(rng.uniform(0, 7200)))
        bad = i % 10 == 7
        if bad:
            head.append(rng.choice(["CHARGE=2+ and 3+", "RTINSECONDS=1-2", "PEPMASS=", "1_0 5"]))
        head = [head[k] for k in rng.permutation(len(head))] if not bad else head
        mz = rng.uniform(100, 1500, int(rng.integers(0, 80)))
        body = head + [num(m) + rng.choice([" ", "\t"]) + num(rng.uniform(1, 1e6)) for m in mz]
        parts.append("\n".join(["BEGIN IONS"] + body + ["END IONS", ""]) + ("\r\n" if i % 5 == 0 else "\n"))
        titled.append(i % 4 != 0)
        clean.append(not bad)
    return "".join(parts).encode("ascii"), np.array(titled), np.array(clean)


def test_parse_ex_is_parse_unless_the_title_is_optional(ctx):
    text, titled, clean = _parse_corpus()
    d_text = _text_dev(ctx, text)
    n, nnz, flags, _ = ctx.mgf_index(d_text)
    assert flags == 0 and n == 400
    names = ["indptr", "mz", "intensity", "precursor_mz", "charge", "has_charge", "retention_time", "title", "span", "status"]
    plain = dict(zip(names, (t.cpu().numpy() for t in ctx.mgf_parse(d_text, n, nnz))))
    # fal_mgf_parse_ex with no bit set: the same bytes in every output
    import torch
    m = max(n, 1)
    outs = [ctx.empty((n + 1,), torch.int64), ctx.empty((nnz,), torch.float64), ctx.empty((nnz,), torch.float32), ctx.empty((m,), torch.float64),
            ctx.empty((m,), torch.int32), ctx.empty((m,), torch.int32), ctx.empty((m,), torch.float64), ctx.empty((m, 2), torch.int64),
            ctx.empty((m, 2), torch.int64), ctx.empty((m,), torch.int32)]
    _lib.check(ctx.lib.fal_mgf_parse_ex(ctx._h, C.c_void_p(d_text.data_ptr()), len(text), n, nnz, *[C.c_void_p(t.data_ptr()) for t in outs], 0),
               "fal_mgf_parse_ex")
    for k, t in zip(names, outs):
        assert plain[k].tobytes() == t.cpu().numpy().tobytes(), k
    assert ctx.lib.fal_mgf_parse_ex(ctx._h, C.c_void_p(d_text.data_ptr()), len(text), n, nnz, *[C.c_void_p(t.data_ptr()) for t in outs], 2) == _lib.FAL_EINVAL
    # the bit set: only the status of the spectra without TITLE differs
    opt = dict(zip(names, (t.cpu().numpy() for t in ctx.mgf_parse(d_text, n, nnz, _lib.MGF_OPT_TITLE))))
    for k in names[:-1]:
        assert plain[k].tobytes() == opt[k].tobytes(), k
    assert np.array_equal(plain["status"] != 0, ~titled | ~clean)
    assert np.array_equal(opt["status"] != 0, ~clean)
    assert not opt["title"][~titled].any() and (~titled & clean).sum() > 50
    res = ctx.parse_mgf(text, optional_title=True, keys=["scans"])
    assert np.array_equal(res["status"], opt["status"]) and res["key_state"].shape == (400, 1) and not res["key_state"].any()


# ---- the library reader -------------------------------------------------------------------------------------------------------------
def _outcome(fn):
    try:
        return "ok", fn()
    except Exception as e:          # noqa: BLE001 -- the readers must fail alike
        return type(e).__name__, None


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    files = K.write_corpus(tmp_path_factory.mktemp("library"))
    counts = {}
    kind, specs = _outcome(lambda: mgf_io.read_annotation_library(files, counts))
    return files, kind, (K.canonical(specs) if kind == "ok" else None), counts


@pytest.mark.parametrize("max_bytes", [None, 3000], ids=["one stretch", "stretches"])
def test_the_library_reader_equals_the_host_reader(ctx, corpus, max_bytes):
    files, kind, want, want_counts = corpus
    counts = {}
    kw = {} if max_bytes is None else dict(max_bytes=max_bytes)
    if max_bytes is None:
        got_kind, chunks = _outcome(lambda: mgf_io.read_annotation_library(files, counts, ctx=ctx))
    else:                                             # stretches cut between entries; the 5000-byte NAME= line exceeds one
        got_kind, chunks = _outcome(lambda: mgf_io.read_annotation_chunks(files, ctx, counts, **kw))
    assert got_kind == kind
    if kind != "ok":
        return
    got = K.canonical(mgf_io.chunk_entries(chunks))
    assert len(got) == len(want) == 286
    for g, w in zip(got, want):
        assert g == w, (dict(g)["identifier"], dict(w)["identifier"])
    assert {k: counts[k] for k in ("entries", "skipped")} == want_counts == dict(entries=292, skipped=6)
    in_two = [c for c in chunks if c.filename == files[1]]
    assert in_two[-1].reader == "host" and all(c.reader == "device" for c in chunks if c.filename == files[0])
    if max_bytes is not None:                         # the stretches in front of the name outside the grammar are the device's
        assert len(chunks) > 40 and in_two[0].reader == "device" and sum(c.reader == "host" for c in chunks) == 1
    assert all(hasattr(c.mz, "cpu") for c in chunks if c.reader == "device")              # the peaks stay on the device


def test_a_clean_library_needs_no_host_read(ctx, tmp_path, monkeypatch):
    """no TITLE, all seven keys, repr() numbers: the device path reads no entry again on the host"""
    path = str(tmp_path / "clean.mgf")
    with open(path, "w") as f:
        f.write(K.clean_text(300, 4))
    want = K.canonical(mgf_io.read_annotation_library([path]))
    calls = []
    rule = mgf_io._annotation_entry
    monkeypatch.setattr(mgf_io, "_annotation_entry", lambda *a: calls.append(a[-1]) or rule(*a))
    for kw in ({}, dict(max_bytes=5000)):
        counts = {}
        chunks = mgf_io.read_annotation_chunks([path], ctx, counts, **kw)
        assert counts == dict(entries=300, skipped=0, host=0) and sum(c.n_host for c in chunks) == 0 and calls == []
        assert K.canonical(mgf_io.chunk_entries(chunks)) == want
    assert len(mgf_io.read_annotation_library([path])) == 300 and len(calls) == 300      # (the spy sees the host reader)


# ---- the representative reader ------------------------------------------------------------------------------------------------------
def _reps(n, first=1, seed=3, start=0):
    rng = np.random.default_rng(seed)
    return [{"identifier": f"rep {start + i}", "precursor_mz": float(rng.uniform(300, 900)), "precursor_charge": [None, 2, -1][i % 3],
             "retention_time": float(i), "cluster": 5 * i + first, "mz": np.sort(rng.uniform(100, 900, 6)),
             "intensity": rng.uniform(1, 100, 6).astype(np.float32)} for i in range(n)]


def _both_readers(ctx, files, **kw):
    host = _outcome(lambda: K.canonical(mgf_io.read_library(files)))
    counts = {}
    dev = _outcome(lambda: K.canonical(mgf_io.chunk_entries(mgf_io.read_library_chunks(files, ctx, counts, **kw))))
    return host, dev, counts


def test_the_representative_reader_equals_the_host_reader(ctx, tmp_path):
    a, b = str(tmp_path / "reps.mgf"), str(tmp_path / "reps2.mgf")
    mgf_io.write_spectra(a, _reps(300))
    with open(b, "w") as f:
        f.write(K.rep("plus", "+7") + K.rep("underscore", "1_0") + K.rep("rejected", "3", pep=None) + K.rep("last", " 12 ", "CLUSTER=99") +
                K.rep("host spectrum", "13", "CHARGE=2+ and 3+") + K.rep("long line", "14", "USER=" + "u" * 5000) +
                K.rep("long cluster line", " " * 5000 + "15"))
    for kw in ({}, dict(max_bytes=2000)):
        host, dev, counts = _both_readers(ctx, [a, b], **kw)
        assert host[0] == dev[0] == "ok" and len(host[1]) == 306
        for g, w in zip(dev[1], host[1]):
            assert g == w, (dict(g)["identifier"], dict(w)["identifier"])
        assert len(dev[1]) == 306 and counts == dict(entries=307, host=4)                              # rejected, host spectrum, the two long lines
    assert isinstance(mgf_io.read_library([a], ctx=ctx)[0], mgf_io.EntryChunk)


MISSING, NOT_INT, EMPTY = K.rep("no cluster", None), K.rep("not an integer", "1 2"), K.rep("empty", "")
GOOD = [K.rep(f"good {j}", str(100 + j)) for j in range(4)]
REPEAT = K.rep("repeat", "101")
NO_LINE, NO_INT, TWICE = "has no CLUSTER= line", "CLUSTER=1 2 is not an integer", "repeats CLUSTER=101 of"
PROBLEMS = {                                          # the entries of the file, and what the first problem's message holds
    "missing": (GOOD[:2] + [K.rep("rejected", "5", pep=None), MISSING] + GOOD[2:], "entry 4 (TITLE=no cluster) " + NO_LINE),
    "not an integer": (GOOD[:3] + [NOT_INT, GOOD[3]], NO_INT),
    "empty value": ([GOOD[0], EMPTY], "(TITLE=empty): CLUSTER= is not an integer"),
    "repeat": (GOOD + [K.rep("rejected", "101", pep=None), REPEAT], "spectrum 5 (TITLE=repeat) " + TWICE),
    "missing, then not an integer": ([GOOD[0], MISSING, NOT_INT], NO_LINE),
    "not an integer, then missing": ([GOOD[0], NOT_INT, MISSING], NO_INT),
    "repeat, then missing": (GOOD[:2] + [REPEAT, MISSING], TWICE),
    "missing, then repeat": (GOOD[:2] + [MISSING, REPEAT], NO_LINE),
    "repeat, then not an integer": (GOOD[:2] + [REPEAT, NOT_INT], TWICE),
    "not an integer, then repeat": (GOOD[:2] + [NOT_INT, REPEAT], NO_INT),
    "repeat of a value int() decided": ([K.rep("first", "+7"), K.rep("x", "8"), K.rep("again", "0_7")], "repeats CLUSTER=7 of"),
}


@pytest.mark.parametrize("case", sorted(PROBLEMS))
def test_the_first_problem_raises_the_host_readers_message(ctx, tmp_path, case):
    path = str(tmp_path / "reps.mgf")
    with open(path, "w") as f:
        f.write("".join(PROBLEMS[case][0]))
    for kw in ({}, dict(max_bytes=150)):
        with pytest.raises(mgf_io.MgfLibraryError) as want:
            mgf_io.read_library([path])
        with pytest.raises(mgf_io.MgfLibraryError) as got:
            mgf_io.read_library_chunks([path], ctx, **kw)
        assert str(got.value) == str(want.value)
        assert PROBLEMS[case][1] in str(want.value)


def test_a_repeated_id_across_two_files_names_its_first_holder(ctx, tmp_path):
    a, b = str(tmp_path / "one.mgf"), str(tmp_path / "two.mgf")
    mgf_io.write_spectra(a, _reps(20))
    with open(b, "w") as f:
        f.write(K.rep("fresh", "1000") + K.rep("rejected", "1", pep=None) + K.rep("taken", "36"))
    for kw in ({}, dict(max_bytes=400)):
        with pytest.raises(mgf_io.MgfLibraryError) as want:
            mgf_io.read_library([a, b])
        with pytest.raises(mgf_io.MgfLibraryError) as got:
            mgf_io.read_library_chunks([a, b], ctx, **kw)
        assert str(got.value) == str(want.value) == f"{b}: spectrum 2 (TITLE=taken) repeats CLUSTER=36 of {a} (TITLE=rep 7)"


# ---- loaders and CLI -------------------------------------------------------------------------------------------------------------------
LIBRARY_ARGS = ["--library_min_cosine", "0.5", "--library_min_matched_peaks", "4", "--library_top_n", "2", "--library_max_shift", "60"]


def _write_run_and_library(mgf, lib_mgf):
    """six templates of 30 peaks, three noisy copies each -> the input MGF; a GNPS-style library without TITLE: the templates'
    analogues at +14.0157 or the compounds themselves, one unrelated entry, one without a precursor, one the host reader decides"""
    from falcon_amd.ms_io import ms_io
    rng = np.random.default_rng(12)
    specs, lines = [], []
    for t in range(6):
        mz, it = np.sort(rng.uniform(150.0, 850.0, 30)), rng.uniform(100.0, 1e4, 30)
        moves = rng.permutation(30) < 15
        pmz, charge = 940.0 + 3.0 * t, 2 + t % 2
        for _ in range(3):
            m = mz + rng.normal(0.0, 0.002, 30)
            o = np.argsort(m)
            specs.append({"identifier": f"scan={len(specs) + 1}", "precursor_mz": pmz * (1.0 + rng.normal(0, 1e-6)), "precursor_charge": charge,
                          "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)), "mz": m[o],
                          "intensity": (it * rng.uniform(0.9, 1.1, 30))[o].astype(np.float32)})
        shift = 14.0157 if t < 4 else 0.0
        lm = mz + moves * shift
        o = np.argsort(lm)
        lines += ["BEGIN IONS", f"PEPMASS={pmz + shift:.4f}"] + ([f"CHARGE={charge}+"] if t < 4 else ["CHARGE=0"] if t == 4 else [])
        lines += [f'NAME=Compound {t}, "form {t}" M+H', f"SPECTRUMID=CCMSLIB{t:08d}", "ADDUCT=M+H", f"INCHIKEY=KEY-{t}", "IONMODE=Positive", "SMILES=C=O"]
        lines += [f"{a:.4f} {b:.2f}" for a, b in zip(lm[o], (0.01 * it)[o])] + ["END IONS", ""]
    um = np.sort(rng.uniform(150.0, 850.0, 30))
    lines += ["BEGIN IONS", "PEPMASS=946.0", "NAME=unrelated"] + [f"{a:.4f} 10.0" for a in um] + ["END IONS", ""]
    lines += ["BEGIN IONS", "PEPMASS=0", "NAME=no precursor", "100.0 1.0", "END IONS", ""]
    ms_io.write_spectra(mgf, [specs[i] for i in rng.permutation(len(specs))])
    clean = "\n".join(lines) + "\n"
    with open(lib_mgf, "w") as f:
        f.write(clean + "\n".join(["BEGIN IONS", "PEPMASS=950.5", "CHARGE=2+ and 3+", "NAME=host decides"] + [f"{a:.4f} 5.0" for a in um] + ["END IONS", ""]))
    return clean


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() if a.dtype.kind != "U" else a.tolist() == b.tolist()


def test_loaders_and_cli_do_not_depend_on_the_reader(tmp_path, caplog, monkeypatch):
    from falcon_amd import falcon
    from falcon_amd.config import config
    from falcon_amd.device import Context
    mgf, lib_mgf, clean_lib = str(tmp_path / "in.mgf"), str(tmp_path / "gnps_like.mgf"), str(tmp_path / "clean.mgf")
    clean = _write_run_and_library(mgf, lib_mgf)
    with open(clean_lib, "w") as f:
        f.write(clean)
    calls = []
    rule = mgf_io._annotation_entry
    monkeypatch.setattr(mgf_io, "_annotation_entry", lambda *a: calls.append(a[-1]) or rule(*a))
    outs, msgs = {}, {}
    for reader in ("device", "host"):
        out = str(tmp_path / f"res_{reader}")
        caplog.clear()
        calls.clear()
        with caplog.at_level(logging.INFO, logger="falcon"):
            assert falcon.main([mgf, out, "--eps", "0.3", "--export_representatives", "--work_dir", str(tmp_path / f"work_{reader}"), "--network",
                                "--network_min_cosine", "0.5", "--network_families", "--library_propagate", "--library", lib_mgf] + LIBRARY_ARGS +
                               ([] if reader == "device" else ["--mgf_reader", "host"])) == 0
        assert sorted(calls) == ([9] if reader == "device" else list(range(1, 10)))          # (the entry the host reader decides)
        msgs[reader] = [r.getMessage() for r in caplog.records if " library spectra " in r.getMessage()]
        names = sorted(f for f in os.listdir(tmp_path) if f.startswith(f"res_{reader}"))
        outs[reader] = {f.replace(f"res_{reader}", "res"): open(tmp_path / f, "rb").read().replace(f"work_{reader}".encode(), b"work")
                        .replace(f"res_{reader}".encode(), b"res") for f in names}
        work = tmp_path / f"work_{reader}" / "spectra"
        outs[reader].update({f: {k: v for k, v in np.load(work / f).items()} for f in sorted(os.listdir(work)) if f.startswith("reference_charge_")})
    assert len(msgs["device"]) == 2 and msgs["device"] == msgs["host"] and "Read 8 library spectra from 1 file(s), skipped 1 " in msgs["host"][0]
    assert sorted(outs["device"]) == sorted(outs["host"]) and any(f.endswith(".library.csv") for f in outs["host"])
    assert sum(f.startswith("reference_charge_") for f in outs["host"]) == 2
    for f, want in outs["host"].items():
        got = outs["device"][f]
        assert got == want if isinstance(want, bytes) else (sorted(got) == sorted(want) and all(_same(got[k], want[k]) for k in want)), f

    # --assign_to: the representatives of the run above
    prev = str(tmp_path / "res_host.mgf")
    for reader in ("device", "host"):
        out = str(tmp_path / f"assigned_{reader}")
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="falcon"):
            assert falcon.main([mgf, out, "--eps", "0.3", "--export_representatives", "--work_dir", str(tmp_path / f"awork_{reader}"),
                                "--assign_to", prev] + ([] if reader == "device" else ["--mgf_reader", "host"])) == 0
        msgs[reader] = [r.getMessage() for r in caplog.records if "representatives" in r.getMessage()]
        names = sorted(f for f in os.listdir(tmp_path) if f.startswith(f"assigned_{reader}"))
        outs[reader] = {f.replace(f"assigned_{reader}", "res"): open(tmp_path / f, "rb").read().replace(f"awork_{reader}".encode(), b"work")
                        for f in names}
        work = tmp_path / f"awork_{reader}" / "spectra"
        outs[reader].update({f: {k: v for k, v in np.load(work / f).items()} for f in sorted(os.listdir(work)) if f.startswith("library_charge_")})
    assert msgs["device"] == msgs["host"] and [m.split()[0] for m in msgs["host"][:2]] == ["Read", "Skipped"]
    assert sorted(outs["device"]) == sorted(outs["host"]) and sum(f.startswith("library_charge_") for f in outs["host"]) == 2
    for f, want in outs["host"].items():
        got = outs["device"][f]
        assert got == want if isinstance(want, bytes) else (sorted(got) == sorted(want) and all(_same(got[k], want[k]) for k in want)), f

    # the loaders themselves, and the spy on a clean library: the host rule is called for no entry
    ctx = Context(0)
    try:
        loaded = {}
        for reader in ("device", "host"):
            which = [] if reader == "device" else ["--mgf_reader", "host"]
            calls.clear()
            spectra_dir = tmp_path / f"loader_{reader}"
            spectra_dir.mkdir()
            config.parse([mgf, str(tmp_path / "unused"), "--library", clean_lib] + which)
            reference = falcon._load_annotation_library(ctx)
            config.parse([mgf, str(tmp_path / "unused"), "--assign_to", prev] + which)
            loaded[reader] = (reference, falcon._load_library(str(spectra_dir), ctx))
            assert len(calls) == (0 if reader == "device" else 8)
        (ref_d, (lib_d, first_d)), (ref_h, (lib_h, first_h)) = loaded["device"], loaded["host"]
        assert list(ref_d) == list(ref_h) and all(_same(ref_d[k], ref_h[k]) for k in ref_h) and len(ref_h["library_id"]) >= 6
        assert first_d == first_h and sorted(lib_d) == sorted(lib_h) == ["2", "3"]
        for z in lib_h:
            assert list(lib_d[z]) == list(lib_h[z]) and all(_same(lib_d[z][k], lib_h[z][k]) for k in lib_h[z]), z
    finally:
        ctx.close()


# ---- the ABI-level checks again with poisoned scratch -----------------------------------------------------------------------------
def run_all(ctx):
    check_spliced(ctx)
    check_sixteen_keys(ctx)
    check_sizes(ctx)
    check_text_rows(ctx)
    check_bad_arguments(ctx)


def test_every_check_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 is read once per process: a fresh child runs the ABI-level checks again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mgfheaders_poison_worker.py")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
