"""`fal_msp_index`, `fal_msp_parse` and `fal_msp_headers` at the C ABI against a plain Python restatement of the MSP grammar
(`tests/msp_cases.py`): floats by their bits, 256 guard bytes behind every output, `nnz_cap` exactly the indexed count.  Then the
reader on top (`msp_io.read_annotation_chunks`) against the host reader field by field, and the CLI: the same `.library.csv` under
either reader, and for one library written as MGF and as MSP."""
import csv
import ctypes as C
import io
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io import mgf_io, msp_io
from tests import mgf_library_cases as K
from tests import msp_cases as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
SPAN, INT = _lib.MGF_KEY_SPAN, _lib.MGF_KEY_INT
ABSENT, PRESENT, HOST = _lib.MGF_KEY_ABSENT, _lib.MGF_KEY_PRESENT, _lib.MGF_KEY_HOST
E = M.entry


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _text_dev(ctx, text: bytes):
    import torch
    return ctx.to_dev(np.frombuffer(bytearray(text), np.uint8)) if text else ctx.empty((0,), torch.uint8)


def _guarded(ctx, sizes: dict):
    import torch
    bufs = {k: torch.full((v + GUARD,), 0xA5, dtype=torch.uint8, device=ctx.tdev) for k, v in sizes.items()}
    return bufs, {k: C.c_void_p(b.data_ptr()) for k, b in bufs.items()}


def _intact(bufs, sizes):
    return all(bool((b[sizes[k]:] == 0xA5).all().item()) for k, b in bufs.items())


def _untouched(bufs):
    return all(bool((b == 0xA5).all().item()) for b in bufs.values())


PARSE_OUTS = (("indptr", np.int64), ("mz", np.float64), ("intensity", np.float32), ("precursor_mz", np.float64), ("charge", np.int32),
              ("has_charge", np.int32), ("span", np.int64), ("status", np.int32))


def parse_rc(ctx, d_text, n_bytes, n, nnz):
    """fal_msp_parse with every output followed by 0xA5 bytes and nnz_cap = nnz -> (return code, outputs as host arrays, guards
    intact and -- after an error -- nothing written at all)"""
    sizes = dict(indptr=8 * (n + 1), mz=8 * nnz, intensity=4 * nnz, precursor_mz=8 * n, charge=4 * n, has_charge=4 * n, span=16 * n, status=4 * n)
    bufs, p = _guarded(ctx, sizes)
    rc = ctx.lib.fal_msp_parse(ctx._h, C.c_void_p(d_text.data_ptr()) if n_bytes else None, n_bytes, n, nnz, *[p[k] for k, _ in PARSE_OUTS])
    ctx.sync()
    ok = _intact(bufs, sizes) if rc == 0 else _untouched(bufs)
    outs = {k: bufs[k][:sizes[k]].cpu().numpy().view(dt) for k, dt in PARSE_OUTS}
    outs["span"] = outs["span"].reshape(n, 2)
    return rc, outs, ok


def check_parse(ctx, text: bytes, n_want=None, host_want=None):
    want = M.expected_parse(text)
    d_text = _text_dev(ctx, text)
    n, nnz, flags, lines = ctx.msp_index(d_text)
    assert (n, nnz, flags, lines) == (want["n"], want["indptr"][-1], 0, text.count(b"\n") + 1)
    assert n_want is None or n == n_want
    rc, got, ok = parse_rc(ctx, d_text, len(text), n, nnz)
    assert rc == 0 and ok
    assert got["indptr"].tolist() == want["indptr"] and got["span"].tolist() == [list(s) for s in want["span"]]
    assert got["status"].tolist() == want["status"]
    assert host_want is None or got["status"].tolist() == host_want
    for i in np.flatnonzero(got["status"] == 0):
        a, b = want["indptr"][i], want["indptr"][i + 1]
        assert got["precursor_mz"][i:i + 1].tobytes() == np.float64(want["precursor_mz"][i]).tobytes(), i
        assert (got["charge"][i], got["has_charge"][i]) == (want["charge"][i], want["has_charge"][i]), i
        assert got["mz"][a:b].tobytes() == want["mz"][i].tobytes() and got["intensity"][a:b].tobytes() == want["intensity"][i].tobytes(), i
    return got


def _lines_entry(name, k, first=0):
    """an entry with k lines behind Num Peaks, one peak each, in falling m/z order (the sort has work to do)"""
    return E(name, num=str(k), peaks=[f"{1000 - (first + j) * 0.5!r} {j + 1}" for j in range(k)], blank=False)


# ---- fal_msp_index / fal_msp_parse -------------------------------------------------------------------------------------------------
def check_rounds(ctx):
    # the wave's 64-line round, and the classify block's 256 lines
    text = "".join(_lines_entry(f"{k} lines", k) for k in (0, 1, 63, 64, 65, 255, 256, 257)).encode()
    check_parse(ctx, text, 8, [0] * 8)
    # a Name: line as the last line of a classify block (line 255) and as the first (line 512)
    text = (_lines_entry("a", 252) + _lines_entry("b", 254) + _lines_entry("c", 3)).encode()
    starts = [i for i, l in enumerate(text.split(b"\n")) if l.startswith(b"Name")]
    assert starts == [0, 255, 512]
    check_parse(ctx, text, 3, [0, 0, 0])
    # the header range over more than one round: 70 header lines, the keys in the second round
    head = [f"Key{j}: value {j}" for j in range(70)]
    check_parse(ctx, E("long header", *head, "Charge: 2-", "PrecursorMZ: 700.125", pm="PrecursorMZ: 1.5").encode(), 1, [0])


def check_sizes(ctx):
    base = (E("one") + E("two", "Charge: 1+")).encode()
    for size in (4095, 4096, 4097):                                              # the mark table's tile
        pad = size - len(base)
        text = b"# " + b"x" * (pad - 3) + b"\n" + base
        assert len(text) == size
        check_parse(ctx, text, 2, [0, 0])
    check_parse(ctx, base.rstrip(b"\n"), 2, [0, 0])                              # no final newline
    check_parse(ctx, b"Name: x", 1, [1])
    check_parse(ctx, b"Name:", 1, [1])
    check_parse(ctx, b"PrecursorMZ: 5\nNum Peaks: 1\n1 2\n", 0)                  # a text without Name:
    check_parse(ctx, b"    \n\t\r\n   ", 0)                                     # blank lines alone
    d_text = _text_dev(ctx, b"")                                                 # an empty text
    assert ctx.msp_index(d_text) == (0, 0, 0, 1)
    rc, got, ok = parse_rc(ctx, d_text, 0, 0, 0)
    assert rc == 0 and ok and got["indptr"].tolist() == [0]
    for n in (255, 256, 257, 1025, 16389):                                       # block turns; past 16384 a wave takes a second entry
        text = "".join(E(f"n{s}", *([f"Charge: {s % 5}"] if s % 3 else []), peaks=M.PEAKS[:s % 4], blank=bool(s % 2)) for s in range(n)).encode()
        check_parse(ctx, text, n, [0] * n)


def check_wide_and_long(ctx):
    note = ' "' + "annotation; " * 8 + '"'                                        # ~100 bytes a line: 64 lines exceed the wave's tile
    wide = [f"{100 + j}.25 {j + 1}{note}" for j in range(70)]
    comments = [f"Comment{j}: " + "c" * 90 for j in range(70)]
    text = (E("wide peak lines", num="70", peaks=wide) + E("wide header lines", *comments, "Charge: 3") + E("behind them")).encode()
    check_parse(ctx, text, 3, [0, 0, 0])
    fit, over = "Comments: " + "x" * 4086, "Comments: " + "x" * 4087             # 4096 bytes: the longest line the kernels take
    assert len(fit) == 4096
    text = (E("fits", fit) + E("header line of 4097 bytes", over) + E("peak line of 4097 bytes", peaks=["1 2 \"" + "x" * 4092]) +
            E("peak line of 4096 bytes", peaks=["1 2 \"" + "x" * 4091]) + E("padded, not long", " " * 5000 + "Charge: 2" + " " * 5000) +
            E("a long line without peaks behind num peaks", num="0", peaks=['"' + "x" * 5000])).encode()
    check_parse(ctx, text, 6, [0, 1, 1, 0, 0, 1])


def check_segments_and_tokens(ctx):
    ten = "; ".join(f"{j}.5 {j}" for j in range(10, 0, -1))
    cases = [
        E("one, two and ten segments", num="13", peaks=["7 1", "5 2; 6 3", ten]),
        E("trailing and double separators", num="5", peaks=["1 2;", "3 4;;5 6", ";;", " ; 7 8 ;\t", "9 1;"]),
        E("quoted separators", num="3", peaks=['3 4 "a; b; c"', '"5 6; 7 8', '1 2; 9 9 "x;y" ; 5 6']),
        E("equal m/z keep their order", num="4", peaks=["5 1; 5 2", "4 9", "5 3"]),
        E("one token, three tokens, tabs", num="3", peaks=["7", "8 2 3", "\t9\t4\t"]),
        E("nan", peaks=["nan 1", "2 2", "3 3"]), E("nan intensity", peaks=["1 nan", "2 2", "3 3"]), E("underscore", peaks=["1_0 1", "2 2", "3 3"]),
        E("twenty digits", peaks=["12345678901234567890 1", "2 2", "3 3"]), E("nineteen digits", peaks=["1234567890123456789 1", "2 2", "3 3"]),
        E("exponent forms", num="4", peaks=["1e2 1E-2; 1.5e+3 2.", ".5 5", "1e28 1"]), E("letters", peaks=["abc 1", "2 2", "3 3"]),
        E("inf precursor", pm="PrecursorMZ: inf"), E("zero precursor", pm="PrecursorMZ: 0"), E("negative precursor", pm="PrecursorMZ: -5"),
        E("empty precursor", pm="PrecursorMZ:"), E("no precursor", pm=None), E("second alias", pm="Precursor_MZ: 2.5"), E("third alias", pm="PEPMASS: 3.5 9"),
        E("first alias present but empty", "Precursor_MZ: 2.5", pm="PrecursorMZ:"), E("the order of the aliases", "PEPMASS: 3.5", "PrecursorMZ: 1.5", pm="Precursor_MZ: 2.5"),
        E("charge forms", "Charge: 2+"), E("negative", "Charge: 3-"), E("signed in front", "Charge: -1"), E("words", "Charge: 2+ and 3+"), E("empty charge", "Charge:"),
        E("last charge wins", "Charge: x", "Charge: 4"),
    ]
    host = [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 1, 1, 0]
    got = check_parse(ctx, "".join(cases).encode(), len(cases), host)
    assert got["precursor_mz"][[13, 14, 17, 18, 20]].tolist() == [0.0, -5.0, 2.5, 3.5, 1.5] and got["charge"][[21, 22, 26]].tolist() == [2, -3, 4]


def check_num_peaks(ctx):
    cases = [E("exact"), E("leading zero", num="03"), E("nine digits", num="000000003"), E("plus", num="+3"), E("two values", num="3 4"),
             E("ten digits", num="0000000003"), E("lower", num="2"), E("higher", num="4"), E("missing", num=None), E("empty", num=""),
             E("a second line is peak text", peaks=["1 2", "Num Peaks: 3", "3 4"]), E("zero of zero", num="0", peaks=[]),
             E("zero of three", num="0"), E("header-shaped peak text", peaks=["1 2", "Comment: x", "3 4"])]
    check_parse(ctx, "".join(cases).encode(), len(cases), [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1])


def check_handle(ctx):
    text = (E("a") + E("b")).encode()
    d_text, other = _text_dev(ctx, text), _text_dev(ctx, (E("c") + E("d")).encode())
    n, nnz = ctx.msp_index(d_text)[:2]
    assert (n, nnz) == (2, 6)
    for args in ((other, len(text), n, nnz), (d_text, len(text) - 1, n, nnz), (d_text, len(text), n + 1, nnz), (d_text, len(text), n - 1, nnz)):
        rc, _, untouched = parse_rc(ctx, *args)
        assert rc == _lib.FAL_EINVAL and untouched and b"fal_msp_index" in ctx.lib.fal_last_error()
    rc, _, untouched = parse_rc(ctx, d_text, len(text), n, nnz - 1)                # a capacity below the indexed count
    assert rc == _lib.FAL_EINVAL and untouched
    rc, got, ok = parse_rc(ctx, d_text, len(text), n, nnz)                         # the index is still good
    assert rc == 0 and ok and got["indptr"].tolist() == [0, 3, 6]
    ctx.trim()
    rc, _, untouched = parse_rc(ctx, d_text, len(text), n, nnz)
    assert rc == _lib.FAL_EINVAL and untouched
    rc, *_, untouched = headers_rc(ctx, d_text, len(text), n, {"name": SPAN})
    assert rc == _lib.FAL_EINVAL and untouched
    with pytest.raises(_lib.FalconHipError):
        ctx.msp_parse(d_text, n, nnz)


def check_side_by_side(ctx):
    """an MGF index and an MSP index of one context, built in either order, then both parses"""
    entries = M.random_entries(40, 9)
    mgf, msp = (t.encode() for t in M.both_formats(entries))
    d_mgf, d_msp = _text_dev(ctx, mgf), _text_dev(ctx, msp)
    for order in ("mgf first", "msp first"):
        if order == "mgf first":
            a, b = ctx.mgf_index(d_mgf), ctx.msp_index(d_msp)
        else:
            b, a = ctx.msp_index(d_msp), ctx.mgf_index(d_mgf)
        assert a[:3] == b[:3] == (40, sum(len(e["peaks"]) for e in entries), 0)
        from_mgf = [t.cpu().numpy() for t in ctx.mgf_parse(d_mgf, a[0], a[1], _lib.MGF_OPT_TITLE)]
        from_msp = [t.cpu().numpy() for t in ctx.msp_parse(d_msp, b[0], b[1])]
        keys = [t.cpu().numpy() for t in ctx.msp_headers(d_msp, b[0], ["name", "smiles"])]
        again = [t.cpu().numpy() for t in ctx.mgf_headers(d_mgf, a[0], ["name", "smiles"])]
        for j in range(6):                                                       # indptr, mz, intensity, precursor, charge, has_charge
            assert from_mgf[j].tobytes() == from_msp[j].tobytes(), (order, j)
        assert not from_mgf[-1].any() and not from_msp[-1].any()
        assert (keys[2] == PRESENT).all() and (again[2] == PRESENT).all()
        assert [msp[x:y] for x, y in keys[0][:, 0]] == [mgf[x:y] for x, y in again[0][:, 0]] == [e["name"].encode() for e in entries]


# ---- fal_msp_headers ---------------------------------------------------------------------------------------------------------------
def _key_args(keys: dict):
    raw = [k.encode("ascii") for k in keys]
    ptr = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=ptr[1:])
    blob = np.frombuffer(b"".join(raw) + b"\0", np.uint8).copy()
    kinds = np.array(list(keys.values()) + [0], np.int32)
    return blob, ptr, kinds


def headers_rc(ctx, d_text, n_bytes, n, keys: dict):
    import torch
    k = len(keys)
    blob, ptr, kinds = _key_args(keys)
    sizes = dict(span=16 * n * k, value=8 * n * k, state=4 * n * k)
    bufs, p = _guarded(ctx, sizes)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)                              # noqa: E731
    rc = ctx.lib.fal_msp_headers(ctx._h, C.c_void_p(d_text.data_ptr()) if n_bytes else None, n_bytes, n, as_p(blob), as_p(ptr), as_p(kinds), k,
                                 p["span"], p["value"], p["state"])
    ctx.sync()
    intact = _intact(bufs, sizes) if rc == 0 else _untouched(bufs)
    span = bufs["span"][:sizes["span"]].view(torch.int64).cpu().numpy().reshape(n, k, 2)
    value = bufs["value"][:sizes["value"]].view(torch.int64).cpu().numpy().reshape(n, k)
    state = bufs["state"][:sizes["state"]].view(torch.int32).cpu().numpy().reshape(n, k)
    return rc, span, value, state, intact


def check_headers(ctx, text: bytes, keys: dict, n_want=None):
    d_text = _text_dev(ctx, text)
    n, _, flags, _ = ctx.msp_index(d_text)
    want = M.expected_headers(text, keys, PRESENT, HOST, INT)
    assert flags == 0 and n == len(want[0]) and (n_want is None or n == n_want)
    rc, span, value, state, intact = headers_rc(ctx, d_text, len(text), n, keys)
    assert rc == 0 and intact
    assert np.array_equal(state, want[2])
    assert np.array_equal(span, want[0])
    assert np.array_equal(value, want[1])
    return span, value, state


LIB_KEYS = {k: SPAN for k in msp_io.LIBRARY_KEYS}
FILL = [f"Filler{j}: {j}" for j in range(200)]


def _at(pos, line):
    """an entry whose line `pos` behind Name: (from 1) is `line`, filler header lines around it"""
    body = [FILL[k] for k in range(pos + 2)]
    body[pos - 1] = line
    return E(f"entry with a key at line {pos}", *body, pm=None)


def check_headers_spliced(ctx):
    parts = [_at(p, f"SMILES: at line {p}") for p in (62, 63, 64, 65, 127, 128, 129)]
    parts.append(E("first turn", "SMILES: only in the first turn", *FILL[:70], "smiles : second turn wins ", "Adduct: only in the second"))
    parts.append(E("kept: the later turns hold no key", *FILL[:150]))
    wide = ["Comment: " + "x" * 91] * 40                                           # 64 lines of more than 4096 bytes: not staged
    parts.append(E("among wide lines", *wide, "InChIKey: among wide lines", "SMILES: C:O", *wide, "Adduct: behind them"))
    parts.append(E("fits", "SMILES: " + "x" * 4088, "Adduct: short"))              # 4096 bytes: the longest line the kernels take
    parts.append(E("the host's", "SMILES: " + "x" * 4089, "Adduct: short"))        # 4097
    parts.append(E("the last one is short", "SMILES: " + "x" * 4089, "SMILES: short"))
    parts.append(E("empty values", "SMILES:", "Adduct: ", "InChIKey:\t", "SMILESS: no", "1: 2", ": x", "no colon"))
    parts.append(E("", pm=None, num=None, peaks=[]))
    parts.append(E("every key", *[f"{k.upper()} : value of {k}" for k in msp_io.LIBRARY_KEYS if k != "name"]))
    parts.append(E("a header-shaped line behind num peaks is no header", "SMILES: in front", peaks=["SMILES: behind", "Adduct: behind", "1 2"]))
    parts.append(E("no num peaks: every line is a header line", "SMILES: a", num=None, peaks=["1 2", "SMILES: the last"]))
    text = "".join(parts).encode()
    span, value, state = check_headers(ctx, ("SMILES: before the first entry\n" + "".join(parts)).encode(), LIB_KEYS)
    names = list(LIB_KEYS)
    smiles, adduct, name = names.index("smiles"), names.index("adduct"), names.index("name")
    full = b"SMILES: before the first entry\n" + text
    got = [full[a:b].decode() if st != ABSENT else None for (a, b), st in zip(span[:, smiles], state[:, smiles])]
    assert got[:7] == [f"at line {p}" for p in (62, 63, 64, 65, 127, 128, 129)] and got[7] == "second turn wins" and got[8] is None
    assert got[9] == "C:O" and state[10, smiles] == PRESENT and state[11, smiles] == HOST and state[12, smiles] == PRESENT and got[12] == "short"
    assert got[13] == "" and state[13, adduct] == PRESENT and (state[14] == [PRESENT] + [ABSENT] * (len(names) - 1)).all() and (state[15] == PRESENT).all()
    assert got[16] == "in front" and state[16, adduct] == ABSENT and got[17] == "the last"
    assert full[span[14, name, 0]:span[14, name, 1]] == b"" and full[span[0, name, 0]:span[0, name, 1]] == b"entry with a key at line 62"
    check_headers(ctx, text, {"smiles": SPAN})
    # keys with a space and with '#', and INT keys beside SPAN keys
    ints = ["0", "007", "-3", "+7", "9" * 18, "9" * 19, "-0", "", "1_0", "1 2", "+", "0x5", " 12 ", "5\r"]
    text = "".join(E(f"n{j}", f"DB#: {v}", *([] if j % 3 else ["db# : 44"]), num=v, peaks=[]) for j, v in enumerate(ints)).encode()
    _, value, state = check_headers(ctx, text, {"db#": INT, "num peaks": INT, "name": SPAN}, len(ints))
    assert list(value[:, 0]) == [44, 7, -3, 44, 10 ** 18 - 1, 0, 44, 0, 0, 44, 0, 0, 44, 5]
    assert list(state[:, 0]) == [1, 1, 1, 1, 1, 2, 1, 1, 2, 1, 2, 2, 1, 1]
    assert list(value[:, 1]) == [0, 7, -3, 7, 10 ** 18 - 1, 0, 0, 0, 0, 0, 0, 0, 12, 5] and list(state[:, 1]) == [1, 1, 1, 1, 1, 2, 1, 1, 2, 2, 2, 2, 1, 1]


def check_headers_arguments(ctx):
    text = E("a").encode()
    d_text = _text_dev(ctx, text)
    n = ctx.msp_index(d_text)[0]
    assert n == 1
    bad = [{f"key{j}": SPAN for j in range(17)}, {"k" * 33: SPAN}, {"Name": SPAN}, {"name": 2}, {"name": SPAN, "smiles": SPAN, "name ": SPAN}, {"a:b": SPAN},
           {"name": SPAN, "name": SPAN, "smiles": SPAN, "smiles ": INT}]
    for keys in bad:
        rc, *_, untouched = headers_rc(ctx, d_text, len(text), n, keys)
        assert rc == _lib.FAL_EINVAL and untouched, keys
    assert headers_rc(ctx, d_text, len(text), n, {})[0] == _lib.FAL_EINVAL
    rc, span, _, state, intact = headers_rc(ctx, d_text, len(text), n, {"a=b": SPAN, "pepmass": SPAN, "charge": INT, "name": SPAN})   # no key is reserved
    assert rc == 0 and intact and state[0].tolist() == [ABSENT, ABSENT, ABSENT, PRESENT] and text[span[0, 3, 0]:span[0, 3, 1]] == b"a"
    keys16 = {f"key{j:02d}": (INT if j % 2 else SPAN) for j in range(15)}
    keys16["k" * 32] = SPAN
    rng = np.random.default_rng(5)
    parts = []
    for s in range(40):
        lines = [f"{k.upper() if s % 2 else k}: {j * 100 + s}" for j, k in enumerate(keys16) if s == 0 or rng.integers(3)]
        parts.append(E(f"s{s}", *[lines[i] for i in rng.permutation(len(lines))]))
    _, _, state = check_headers(ctx, "".join(parts).encode(), keys16)
    assert (state[0] == PRESENT).all() and (state == ABSENT).any()


def check_malformed(ctx):
    rng = np.random.default_rng(1)
    words = [b"Name: x\n", b"name:\n", b"Num Peaks: 2\n", b"num peaks:\n", b"1.5 2\n", b"1 2; 3 4;\n", b";;\n", b"SMILES: C\n", b":\n", b"\n", b"Name\n",
             b"PrecursorMZ: 5\n", b"\"\n", b"SMILES: " + b"y" * 5000 + b"\n", b"1 2;" * 1200 + b"\n"]
    soup = b"".join(words[k] for k in rng.integers(0, len(words), 4000))
    garbage = bytes(rng.choice(np.frombuffer(b"Name: \nNum Peaks: 1\n;;\"12. \t\r\n", np.uint8), 20000))
    for t in (soup, garbage, b"Name: x\nNum Peaks: 1", b"Name:\n" * 700, b"Num Peaks: 1\n" * 40, b":" * 5000, b";" * 5000 + b"\nName: x\nNum Peaks: 0\n" + b"1 2;" * 3000):
        d_text = _text_dev(ctx, t)
        if ctx.msp_index(d_text)[2]:
            continue
        check_parse(ctx, t)
        check_headers(ctx, t, {"name": SPAN, "smiles": INT, "num peaks": INT})
    for t, flag in ((b"Name: caf\xc3\xa9\n", _lib.MGF_FLAG_BYTES), (b"Name: x\rNum Peaks: 0\n", _lib.MGF_FLAG_BYTES), (b"\n" * 4000, _lib.MGF_FLAG_LINES)):
        n, nnz, flags, _ = ctx.msp_index(_text_dev(ctx, t))
        assert flags & flag and (flag != _lib.MGF_FLAG_LINES or (n, nnz) == (0, 0))


def run_all(ctx):
    check_rounds(ctx)
    check_sizes(ctx)
    check_wide_and_long(ctx)
    check_segments_and_tokens(ctx)
    check_num_peaks(ctx)
    check_side_by_side(ctx)
    check_headers_spliced(ctx)
    check_headers_arguments(ctx)
    check_malformed(ctx)
    check_handle(ctx)


def test_parse_at_the_wave_and_block_rounds(ctx):
    check_rounds(ctx)


def test_parse_at_the_tile_sizes_and_on_empty_texts(ctx):
    check_sizes(ctx)


def test_wide_lines_fall_back_to_global_memory_and_long_lines_to_the_host(ctx):
    check_wide_and_long(ctx)


def test_peak_segments_number_forms_and_precursor_aliases(ctx):
    check_segments_and_tokens(ctx)


def test_every_num_peaks_form_and_mismatch(ctx):
    check_num_peaks(ctx)


def test_an_mgf_and_an_msp_index_live_side_by_side(ctx):
    check_side_by_side(ctx)


def test_headers_on_spliced_entries(ctx):
    check_headers_spliced(ctx)


def test_headers_refuse_bad_tables_and_take_sixteen_keys(ctx):
    check_headers_arguments(ctx)


def test_malformed_text_stays_inside_its_outputs(ctx):
    check_malformed(ctx)


def test_parse_refuses_foreign_texts_and_a_trimmed_context(ctx):
    check_handle(ctx)


def test_every_check_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 is read once per process: a fresh child runs the ABI-level checks again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "msp_poison_worker.py")], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the reader --------------------------------------------------------------------------------------------------------------------
def _outcome(fn):
    try:
        return "ok", fn()
    except Exception as e:          # noqa: BLE001 -- the readers must fail alike
        return type(e).__name__, None


def _corpus_text():
    entries = M.random_entries(120, 4)
    hosts = (E("a header line of 5000 bytes", "Comments: " + "x" * 5000) + E("a name of 300 bytes " + "n" * 300, "SMILES: " + "C" * 300) +
             E("float() takes it", peaks=["1_0 1", "2 2", "3 3"]) + E("int() takes it", num="+3") + E("signed charge", "Charge: -2"))
    return (M.NIST + M.MONA + M.both_formats(entries[:60])[1] + "".join(t for t, _ in M.DESIGNED) + hosts + M.MATCHMS +
            M.both_formats(entries[60:])[1])


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    folder = tmp_path_factory.mktemp("msp")
    one, two = str(folder / "lib_one.msp"), str(folder / "lib_two.MSP")
    text = _corpus_text()
    with open(one, "wb") as f:
        f.write(("junk in front of the first entry\n" + text).encode("ascii"))
    second = M.both_formats(M.random_entries(60, 5))[1]
    cut = second.index("Name: compound 30,")
    with open(two, "wb") as f:                                                     # CRLF, a non-ASCII name in the middle, no final newline
        f.write((second[:cut] + E("fallback id in front of it") + E("caféine", "DB#: S100") + E("skipped behind it", pm=None) +
                 E("and the numbering goes on") + second[cut:]).rstrip("\n").replace("\n", "\r\n").encode("utf-8"))
    files = [one, two]
    counts = {}
    kind, specs = _outcome(lambda: msp_io.read_annotation_library(files, counts))
    return files, kind, (K.canonical(specs) if kind == "ok" else None), counts


@pytest.mark.parametrize("max_bytes", [None, 48, 900], ids=["one stretch", "smaller than an entry", "between every two entries"])
def test_the_reader_equals_the_host_reader(ctx, corpus, max_bytes):
    files, kind, want, want_counts = corpus
    counts = {}
    if max_bytes is None:
        got_kind, chunks = _outcome(lambda: msp_io.read_annotation_library(files, counts, ctx=ctx))
    else:
        got_kind, chunks = _outcome(lambda: msp_io.read_annotation_chunks(files, ctx, counts, max_bytes=max_bytes))
    assert got_kind == kind
    if kind != "ok":
        return
    got = K.canonical(mgf_io.chunk_entries(chunks))
    assert len(got) == len(want) > 200
    for g, w in zip(got, want):
        assert g == w, (dict(g)["identifier"], dict(w)["identifier"])
    assert {k: counts[k] for k in ("entries", "skipped")} == want_counts and want_counts["skipped"] == 14 + 1
    assert 0 < counts["host"] < counts["entries"]
    in_two = [c for c in chunks if c.filename == files[1]]
    assert in_two[-1].reader == "host" and all(c.reader == "device" for c in chunks if c.filename == files[0])
    assert any(dict(g)["identifier"] == "lib_two.MSP:31" for g in got) and any(dict(g)["identifier"] == "lib_two.MSP:34" for g in got)
    if max_bytes is not None:                         # the stretches in front of the name outside the grammar are the device's
        assert len(chunks) > 40 and in_two[0].reader == "device" and sum(c.reader == "host" for c in chunks) == 1
    assert all(hasattr(c.mz, "cpu") for c in chunks if c.reader == "device")              # the peaks stay on the device


def test_a_clean_library_needs_no_host_read(ctx, tmp_path, monkeypatch):
    path = str(tmp_path / "clean.msp")
    with open(path, "w") as f:
        f.write(M.both_formats(M.random_entries(300, 6))[1])
    want = K.canonical(msp_io.read_annotation_library([path]))
    calls = []
    rule = msp_io._annotation_entry
    monkeypatch.setattr(msp_io, "_annotation_entry", lambda *a: calls.append(a[-1]) or rule(*a))
    for kw in ({}, dict(max_bytes=5000)):
        counts = {}
        chunks = msp_io.read_annotation_chunks([path], ctx, counts, **kw)
        assert counts == dict(entries=300, skipped=0, host=0) and sum(c.n_host for c in chunks) == 0 and calls == []
        assert K.canonical(mgf_io.chunk_entries(chunks)) == want


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
LIBRARY_ARGS = ["--library_min_cosine", "0.5", "--library_min_matched_peaks", "4", "--library_top_n", "2", "--library_max_shift", "60"]


def _write_run(folder):
    """50 templates of 30 peaks, five noisy copies each -> the input MGF (250 spectra); the library's entries: every second
    template itself or its analogue at +14.0157, plus unrelated ones"""
    from falcon_amd.ms_io import ms_io
    rng = np.random.default_rng(12)
    specs, entries = [], []
    for t in range(50):
        mz, it = np.sort(rng.uniform(150.0, 850.0, 30)), rng.uniform(100.0, 1e4, 30)
        moves = rng.permutation(30) < 15
        pmz, charge = 700.0 + 5.0 * t, 2 + t % 2
        for _ in range(5):
            m = mz + rng.normal(0.0, 0.002, 30)
            o = np.argsort(m)
            specs.append({"identifier": f"scan={len(specs) + 1}", "precursor_mz": pmz * (1.0 + rng.normal(0, 1e-6)), "precursor_charge": charge,
                          "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)), "mz": m[o],
                          "intensity": (it * rng.uniform(0.9, 1.1, 30))[o].astype(np.float32)})
        if t % 2:
            continue
        shift = 14.0157 if t % 4 else 0.0
        lm = np.sort(mz + moves * shift)
        entries.append(dict(pm=f"{pmz + shift:.4f}", charge=charge if t % 3 else 0, name=f"Compound {t}, form {t} M+H", sid=f"CCMSLIB{t:08d}", adduct="M+H",
                            smiles="C=O", inchikey=f"KEY-{t}", ionmode="Positive",
                            peaks=[f"{a:.4f} {b:.2f}" for a, b in zip(lm, (0.01 * it)[np.argsort(mz + moves * shift)])]))
    entries += M.random_entries(20, 8)
    mgf = str(folder / "in.mgf")
    ms_io.write_spectra(mgf, [specs[i] for i in rng.permutation(len(specs))])
    return mgf, entries


def _run(tmp_path, caplog, tag, mgf, libraries, extra=()):
    from falcon_amd import falcon
    out = str(tmp_path / f"res_{tag}")
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="falcon"):
        assert falcon.main([mgf, out, "--eps", "0.3", "--work_dir", str(tmp_path / f"work_{tag}"), "--library", *libraries] + LIBRARY_ARGS + list(extra)) == 0
    read = [r.getMessage() for r in caplog.records if " library spectra from " in r.getMessage()]
    files = {}
    for name in sorted(f for f in os.listdir(tmp_path) if f.startswith(f"res_{tag}.")):
        with open(tmp_path / name, "rb") as f:
            files[name.replace(f"res_{tag}", "res")] = f.read().replace(f"res_{tag}".encode(), b"res").replace(f"work_{tag}".encode(), b"work")
    return files, read


def _without_library_file(text: bytes):
    rows = list(csv.reader(io.StringIO("".join(l + "\n" for l in text.decode().split("\n") if l and not l.startswith("#")))))
    at = rows[0].index("library_file")
    return [[c for j, c in enumerate(r) if j != at] for r in rows]


@pytest.fixture(scope="module")
def run_files(tmp_path_factory):
    folder = tmp_path_factory.mktemp("cli")
    mgf, entries = _write_run(folder)
    as_mgf, as_msp = M.both_formats(entries)
    host_case = E("the host decides", "Charge: -2", pm="PrecursorMZ: 950.5", peaks=[f"{200 + 7 * j}.5 5" for j in range(30)])
    paths = {name: str(folder / name) for name in ("lib.mgf", "lib.msp", "second.MSP")}
    for name, text in (("lib.mgf", as_mgf), ("lib.msp", as_msp), ("second.MSP", as_msp + host_case + E("skipped", pm=None))):
        with open(paths[name], "w") as f:
            f.write(text)
    return mgf, entries, paths


def test_the_cli_reads_an_msp_library_as_it_reads_the_mgf_one(tmp_path, caplog, run_files):
    mgf, entries, paths = run_files
    # the options a library feeds: analog search, the network with families, propagation, the GraphML export
    rest = ["--library_analog", "--network", "--network_min_cosine", "0.5", "--network_families", "--library_propagate", "--network_graphml"]
    from_mgf, _ = _run(tmp_path, caplog, "mgf", mgf, [paths["lib.mgf"]], rest)
    device, read = _run(tmp_path, caplog, "device", mgf, [paths["lib.msp"]], rest + ["--msp_reader", "device"])
    assert len(read) == 1 and f"Read {len(entries)} library spectra from 1 file(s) (0 MGF, 1 MSP), skipped 0 " in read[0]
    host, read_host = _run(tmp_path, caplog, "host", mgf, [paths["lib.msp"]], rest + ["--msp_reader", "host"])
    assert device == host and read == read_host and sorted(device) == sorted(from_mgf)
    assert {f.split(".", 1)[1] for f in device} >= {"csv", "library.csv", "annotations.csv", "network.graphml", "network.csv", "families.csv"}
    rows = _without_library_file(device["res.library.csv"])
    assert rows == _without_library_file(from_mgf["res.library.csv"]) and len(rows) > 20
    assert b"lib.msp" in device["res.library.csv"] and b"lib.mgf" in from_mgf["res.library.csv"]
    for name, text in device.items():                                              # every other file: equal but for the library's name
        assert text.replace(b"lib.msp", b"lib.mgf") == from_mgf[name], name


def test_an_mgf_and_an_msp_library_on_one_command_line(tmp_path, caplog, run_files):
    """in the command line's order, under the device readers and under the host readers"""
    mgf, entries, paths = run_files
    mixed = {}
    for tag, extra in (("dd", ["--mgf_reader", "device", "--msp_reader", "device"]), ("hh", ["--mgf_reader", "host", "--msp_reader", "host"])):
        mixed[tag], read = _run(tmp_path, caplog, tag, mgf, [paths["second.MSP"], paths["lib.mgf"]], extra)
        assert f"Read {2 * len(entries) + 1} library spectra from 2 file(s) (1 MGF, 1 MSP), skipped 1 " in read[0]
    assert mixed["dd"] == mixed["hh"]
    rows = _without_library_file(mixed["dd"]["res.library.csv"])
    files = [r[rows[0].index("name") + 1] for r in list(csv.reader(io.StringIO("".join(
        l + "\n" for l in mixed["dd"]["res.library.csv"].decode().split("\n") if l and not l.startswith("#")))))[1:]]
    assert set(files) == {"second.MSP", "lib.mgf"} and len(rows) > 20


def test_the_loader_keeps_the_order_of_the_command_line(tmp_path):
    from falcon_amd import falcon
    from falcon_amd.config import config
    from falcon_amd.device import Context
    entries = M.random_entries(30, 2)
    as_mgf, as_msp = M.both_formats(entries)
    a, b = str(tmp_path / "a.mgf"), str(tmp_path / "b.Msp")
    for path, text in ((a, as_mgf), (b, as_msp)):
        with open(path, "w") as f:
            f.write(text)
    ctx = Context(0)
    try:
        loaded = {}
        for readers in (("device", "device"), ("host", "host")):
            config.parse(["in.mgf", str(tmp_path / "unused"), "--library", b, a, "--mgf_reader", readers[0], "--msp_reader", readers[1], "--min_peaks", "1",
                          "--min_mz_range", "0"])
            loaded[readers] = falcon._load_annotation_library(ctx)
        d, h = loaded.values()
        assert list(d) == list(h) and all(d[k].tolist() == h[k].tolist() and d[k].dtype == h[k].dtype for k in h)
        n = len(d["library_id"]) // 2                                              # the same entries twice: first the MSP file's
        assert n >= 20 and d["library_file"].tolist() == ["b.Msp"] * n + ["a.mgf"] * n and d["library_id"][:n].tolist() == d["library_id"][n:].tolist()
        half = int(d["indptr"][n])
        assert d["mz"][:half].tobytes() == d["mz"][half:].tobytes() and d["precursor_mz"][:n].tobytes() == d["precursor_mz"][n:].tobytes()
    finally:
        ctx.close()
