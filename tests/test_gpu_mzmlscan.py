"""The device mzML reader (`Context.scan_mzml` = `fal_mzml_index` + `fal_mzml_parse`, and `mzml_io.read_chunks_device` on top of
it) against the host reader `mzml_io.read_chunks`: identifiers, precursor m/z, charge and retention time bit for bit, the arrays'
text, counts and flags equal and the decoded peak CSR bit-identical; exactly the expected spectra go back to the host reader (none
of the clean corpus); text outside the device grammar is read by the host reader with its warning; malformed text never writes
outside a slot; and the CLI gives byte-identical outputs with either reader.  The inputs are `tests/mzml_cases.py`'s, which
`test_mzmlscan_cpu.py` runs through the host build of the same functions."""
import ctypes as C
import logging

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io import mzml_io
from tests import mzml_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


class _Recording:
    """a context that keeps every status vector `scan_mzml` returned"""

    def __init__(self, ctx):
        self.ctx, self.status, self.calls = ctx, [], 0

    def scan_mzml(self, text):
        res = self.ctx.scan_mzml(text)
        self.calls += 1
        self.status += [int(s) for s in res.get("status", [])]
        return res


def _both(ctx, path, max_bytes=None):
    rec = _Recording(ctx)
    kw = {} if max_bytes is None else {"max_bytes": max_bytes}
    got = list(mzml_io.read_chunks_device(str(path), rec, **kw))
    want = list(mzml_io.read_chunks(str(path)))
    return got, want, rec


def _decoded(ctx, chunks):
    out = []
    for c in chunks:
        if len(c):
            indptr, mz, it, status = ctx.decode_peaks(*c.tables())
            out.append((np.diff(indptr.cpu().numpy()), mz.cpu().numpy(), it.cpu().numpy(), status.cpu().numpy()))
    return [np.concatenate([o[k] for o in out]) if out else np.zeros(0) for k in range(4)]


def _assert_equal(ctx, got, want, n=None):
    rows_g, rows_w = MC.chunk_rows(got), MC.chunk_rows(want)
    assert rows_g == rows_w
    if n is not None:
        assert len(rows_w[0]) == n
    for a, b in zip(_decoded(ctx, got), _decoded(ctx, want)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the clean corpus ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", MC.CORPUS_VARIANTS, ids=lambda v: "mz%d-int%d-%s-%s" % (v[0], v[1], "zlib" if v[2] else "none",
                                                                                             "indexed" if v[3] else "plain"))
def test_clean_corpus_equals_the_host_reader(ctx, tmp_path, variant):
    path = tmp_path / "corpus.mzML"
    MC.write_corpus(path, variant)
    got, want, rec = _both(ctx, path)
    _assert_equal(ctx, got, want, 300)
    assert rec.status.count(MC.OK) == 300 and rec.status.count(MC.SKIP) == 100 and MC.HOST not in rec.status
    assert sum(c.n_device for c in got if hasattr(c, "n_device")) == 400


def test_numpress_corpus_equals_the_host_reader(ctx, tmp_path):
    path = tmp_path / "np.mzML"
    MC.write_numpress_corpus(path)
    got, want, rec = _both(ctx, path)
    _assert_equal(ctx, got, want, 60)
    assert set(rec.status) == {MC.OK}


# ---- 2. param groups, odd cases -----------------------------------------------------------------------------------------------
def test_param_groups_go_to_the_host(ctx, tmp_path):
    path = tmp_path / "groups.mzML"
    MC.W.write_mzml(path, MC.corpus_spectra(40), param_groups=True, ms1_every=3)
    got, want, rec = _both(ctx, path)
    _assert_equal(ctx, got, want, 40)
    assert rec.status.count(MC.HOST) == 54 and MC.OK not in rec.status       # (the MS1 spectra's arrays carry group refs too)


def test_odd_cases(ctx, tmp_path):
    path = tmp_path / "odd.mzML"
    names, expected = MC.odd_file(path)
    got, want, rec = _both(ctx, path)
    rows_g, rows_w = MC.chunk_rows(got), MC.chunk_rows(want)
    assert rows_g == rows_w and sum(rows_w[1].values()) >= 4                 # rows in file order, skipped counters equal
    assert len(rec.status) == len(names) and list(zip(names, rec.status)) == list(zip(names, expected))


# ---- 3. outside the grammar ---------------------------------------------------------------------------------------------------
def test_text_outside_the_grammar_is_the_host_readers(ctx, tmp_path, caplog):
    path = tmp_path / "x.mzML"
    MC.write_corpus(path, MC.CORPUS_VARIANTS[1], n=30)
    data = path.read_bytes()
    header, pieces, footer = MC.split_file(data)
    cases = {"comment": header + b"".join(pieces[:10]) + b"<!-- c -->" + b"".join(pieces[10:]) + footer,
             "encoding": data.replace(b'encoding="utf-8"', b'encoding="ISO-8859-1"'),
             "cut mid-spectrum": header + b"".join(pieces[:20]) + pieces[20][:len(pieces[20]) // 2]}
    for name, text in cases.items():
        path.write_bytes(text)
        seen = []
        for reader in (lambda: mzml_io.read_chunks_device(str(path), ctx, 8192), lambda: mzml_io.read_chunks(str(path))):
            caplog.clear()
            with caplog.at_level(logging.WARNING, logger="falcon"):
                rows = MC.chunk_rows(reader())
            seen.append((rows, [r.getMessage() for r in caplog.records]))
        assert seen[0] == seen[1], name
        ms2_before_cut = sum(b'id="ms1_' not in p for p in pieces[:20])
        assert len(seen[1][0][0]) == (ms2_before_cut if name == "cut mid-spectrum" else 30)
        assert len(seen[1][1]) == (1 if name == "cut mid-spectrum" else 0), name


# ---- 4. sizes, chunking ---------------------------------------------------------------------------------------------------------
def test_empty_and_single(ctx, tmp_path):
    path = tmp_path / "s.mzML"
    for spectra in ([], MC.corpus_spectra(1)):
        MC.W.write_mzml(path, spectra)
        got, want, _ = _both(ctx, path)
        _assert_equal(ctx, got, want, len(spectra))
    assert ctx.scan_mzml(b"")["flags"] == 0 and len(ctx.scan_mzml(b"")["status"]) == 0


def test_one_spectrum_of_2_mb_of_base64(ctx, tmp_path):
    path = tmp_path / "big.mzML"
    rng = np.random.default_rng(2)
    k = 131072                                                                # 1 MB of float64 + 0.5 MB of float32 -> 2 MB of base64
    s = {"identifier": "big", "precursor_mz": 500.5, "precursor_charge": 2, "retention_time": 1.5,
         "mz": np.sort(rng.uniform(100.0, 1500.0, k)), "intensity": rng.uniform(1.0, 1e4, k).astype(np.float32)}
    MC.W.write_mzml(path, [s], zlib_arrays=False)
    assert MC.size(path) > 2_000_000
    got, want, rec = _both(ctx, path, 4096)
    _assert_equal(ctx, got, want, 1)
    assert rec.status == [MC.OK]


def test_a_10000_byte_id(ctx, tmp_path):
    path = tmp_path / "id.mzML"
    s = MC.corpus_spectra(3)
    s[1]["identifier"] = "i" * 10000
    MC.W.write_mzml(path, s)
    got, want, rec = _both(ctx, path)
    _assert_equal(ctx, got, want, 3)
    assert rec.status == [MC.OK] * 3


@pytest.mark.parametrize("max_bytes", [4096, 100])
def test_chunked_reading_equals_one_chunk(ctx, tmp_path, max_bytes):
    path = tmp_path / "chunks.mzML"
    MC.write_corpus(path, MC.CORPUS_VARIANTS[0], n=80)
    got, want, rec = _both(ctx, path, max_bytes)
    _assert_equal(ctx, got, want, 80)
    assert rec.calls > 10 and MC.HOST not in rec.status


# ---- 5. guarded outputs ---------------------------------------------------------------------------------------------------------
def _guarded_scan(ctx, text: bytes, guard=256):
    """fal_mzml_index + fal_mzml_parse with every output followed by 0xA5 bytes -> (spectra, flags, status, all guards intact?)"""
    import torch
    d_text = ctx.to_dev(np.frombuffer(bytearray(text), np.uint8)) if text else ctx.empty((0,), torch.uint8)
    n, _, flags, _ = ctx.mzml_index(d_text)
    sizes = dict(payload=len(text) + 16 * n, status=4 * n, id=16 * n, span=16 * n, pmz=8 * n, charge=4 * n, rt=8 * n, arrays=64 * n)
    bufs = {k: torch.full((v + guard,), 0xA5, dtype=torch.uint8, device=ctx.tdev) for k, v in sizes.items()}
    p = {k: C.c_void_p(b.data_ptr()) for k, b in bufs.items()}
    _lib.check(ctx.lib.fal_mzml_parse(ctx._h, C.c_void_p(d_text.data_ptr()) if text else None, len(text), n, p["payload"], sizes["payload"],
                                      p["status"], p["id"], p["span"], p["pmz"], p["charge"], p["rt"], p["arrays"]), "fal_mzml_parse")
    ctx.sync()
    intact = all(bool((b[sizes[k]:] == 0xA5).all().item()) for k, b in bufs.items())
    status = bufs["status"][:sizes["status"]].view(torch.int32).cpu().numpy()
    return n, flags, status, intact


def test_malformed_text_never_writes_outside_a_slot(ctx, tmp_path):
    muts, n = MC.mutations(tmp_path / "m.mzML")
    assert len(muts) > 40
    cuts = [m for m in muts if m[2] is None]
    for name, text, target in [m for m in muts if m[2] is not None] + cuts:
        k, flags, status, intact = _guarded_scan(ctx, text)
        assert intact, name
        if target is None:
            assert flags or k == n - 1, name
        else:
            assert flags or status[target] == MC.HOST, name


def test_parse_refuses_a_text_it_did_not_index(ctx, tmp_path):
    path = tmp_path / "one.mzML"
    MC.W.write_mzml(path, MC.corpus_spectra(2))
    _, pieces, _ = MC.split_file(path.read_bytes())
    a = ctx.to_dev(np.frombuffer(bytearray(b"".join(pieces)), np.uint8))
    b = ctx.to_dev(np.frombuffer(bytearray(b"".join(pieces[::-1])), np.uint8))
    n = ctx.mzml_index(a)[0]
    assert n == 2
    with pytest.raises(_lib.FalconHipError, match="fal_mzml_index"):
        ctx.mzml_parse(b, n)
    assert ctx.mzml_parse(a, n)[1].cpu().tolist() == [MC.OK, MC.OK]


# ---- 6. CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_outputs_do_not_depend_on_the_reader(tmp_path, caplog):
    from falcon_amd import synth
    from falcon_amd.falcon import main
    d = synth.generate(1500, seed=5)
    specs = []
    for i in range(1500):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        specs.append({"identifier": f"scan={i}", "precursor_mz": float(d["precursor_mz"][i]), "precursor_charge": int(d["precursor_charge"][i]),
                      "retention_time": float(d["retention_time"][i]), "mz": d["mz"][a:b].astype(np.float64), "intensity": d["intensity"][a:b]})
    mzml = str(tmp_path / "in.mzML")
    MC.W.write_mzml(mzml, specs, ms1_every=5)
    with open(mzml, "rb") as f:                       # one spectrum for the host reader, and one it counts as skipped
        header, pieces, footer = MC.split_file(f.read())
    pieces[7] = pieces[7].replace(b'name="ms level" value="2"', b"name=\"ms level\" value='2'")
    pieces[9] = pieces[9].replace(MC.ZLIB, MC.ZLIB + MC._cv("MS:1003089"), 1)
    with open(mzml, "wb") as f:
        f.write(header + b"".join(pieces) + footer)
    outs, counts = {}, {}
    for reader in ("device", "host"):
        out = str(tmp_path / f"res_{reader}")
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="falcon"):
            assert main([mzml, out, "--eps", "0.3", "--export_representatives", "--work_dir", str(tmp_path / f"work_{reader}")] +
                        ["--mzml_reader", reader]) == 0
        msgs = [r.getMessage() for r in caplog.records]
        counts[reader] = [m for m in msgs if m.startswith("Read ") and "spectra from" in m and "peak files" in m] + \
                         [m for m in msgs if m.startswith("Skipped ")]
        assert f"mzml_reader = {reader}" in msgs
        assert any("decided on the device, 2 handed to the host reader" in m for m in msgs) == (reader == "device")
        outs[reader] = (open(out + ".csv", "rb").read().replace(f"work_{reader}".encode(), b"work"), open(out + ".mgf", "rb").read())
    assert len(counts["device"]) >= 2 and counts["device"] == counts["host"]
    assert outs["device"][0] == outs["host"][0] and outs["device"][1] == outs["host"][1]
    assert b"mzml_reader" not in outs["device"][0]
    with pytest.raises(SystemExit):
        main([mzml, str(tmp_path / "x"), "--mzml_reader", "gpu"])
