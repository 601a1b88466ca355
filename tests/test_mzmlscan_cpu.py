"""The mzML device reader's pure functions (`csrc/mzmlscan.h`) on the host: the whole scan as a host loop
(`tests/hostbuild_mzml.py`) against `mzml_io.read_chunks` on the same bytes -- per-spectrum status, the columns bit for bit, the
arrays' base64 text, counts and flags -- and `mzml_io.read_chunks_device` over that scan against `read_chunks`."""
import logging

import pytest

from falcon_amd.ms_io import mzml_io
from tests import hostbuild_mzml as H
from tests import mzml_cases as MC

pytestmark = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("mzml_shim"))


def _both(lib, path, max_bytes=None):
    ctx = H.FakeContext(lib)
    kw = {} if max_bytes is None else {"max_bytes": max_bytes}
    got = MC.chunk_rows(mzml_io.read_chunks_device(str(path), ctx, **kw))
    want = MC.chunk_rows(mzml_io.read_chunks(str(path)))
    return got, want, ctx


def _statuses(lib, ctx):
    return [int(s) for text in ctx.texts for s in H.scan(lib, text).get("status", [])]


@pytest.mark.parametrize("variant", MC.CORPUS_VARIANTS, ids=lambda v: "mz%d-int%d-%s-%s" % (v[0], v[1], "zlib" if v[2] else "none",
                                                                                             "indexed" if v[3] else "plain"))
def test_clean_corpus_equals_the_host_reader(lib, tmp_path, variant):
    path = tmp_path / "corpus.mzML"
    MC.write_corpus(path, variant)
    got, want, ctx = _both(lib, path)
    assert len(want[0]) == 300 and got == want
    st = _statuses(lib, ctx)
    assert st.count(MC.OK) == 300 and st.count(MC.SKIP) == 100 and MC.HOST not in st


def test_numpress_corpus(lib, tmp_path):
    path = tmp_path / "np.mzML"
    MC.write_numpress_corpus(path)
    got, want, ctx = _both(lib, path)
    assert len(want[0]) == 60 and got == want
    assert set(_statuses(lib, ctx)) == {MC.OK}


def test_param_groups_go_to_the_host(lib, tmp_path):
    path = tmp_path / "groups.mzML"
    MC.W.write_mzml(path, MC.corpus_spectra(40), param_groups=True, ms1_every=3)
    got, want, ctx = _both(lib, path)
    assert len(want[0]) == 40 and got == want
    st = _statuses(lib, ctx)
    assert st.count(MC.HOST) == 54 and MC.OK not in st               # (the MS1 spectra's arrays carry group refs too)


def test_odd_cases(lib, tmp_path):
    path = tmp_path / "odd.mzML"
    names, expected = MC.odd_file(path)
    got, want, ctx = _both(lib, path)
    assert got == want
    assert sum(want[1].values()) >= 4                                    # the skipped counters are exercised
    st = _statuses(lib, ctx)
    assert len(st) == len(names) and list(zip(names, st)) == list(zip(names, expected))
    kept = [r[0] for r in want[0]]
    assert kept == sorted(kept, key=lambda i: int(i.split()[1].split("&")[0].rstrip("é")))      # file order


@pytest.mark.parametrize("max_bytes", [4096, 100])
def test_chunking(lib, tmp_path, max_bytes):
    path = tmp_path / "chunks.mzML"
    MC.write_corpus(path, MC.CORPUS_VARIANTS[0], n=80)
    got, want, ctx = _both(lib, path, max_bytes)
    assert got == want and len(ctx.texts) > 10


def test_outside_the_grammar(lib, tmp_path, caplog):
    path = tmp_path / "x.mzML"
    MC.write_corpus(path, MC.CORPUS_VARIANTS[1], n=30)
    data = path.read_bytes()
    header, pieces, footer = MC.split_file(data)
    cases = {"comment": header + b"".join(pieces[:10]) + b"<!-- c -->" + b"".join(pieces[10:]) + footer,
             "encoding": data.replace(b'encoding="utf-8"', b'encoding="ISO-8859-1"'),
             "spectrum inside a header comment": data.replace(b'<run id="r">', b"<!-- " + pieces[1] + b" -->" + b'<run id="r">'),
             "cut mid-spectrum": header + b"".join(pieces[:20]) + pieces[20][:len(pieces[20]) // 2],
             "cut behind a spectrum": header + b"".join(pieces[:20]),
             "cut in the footer": data[:-20]}
    for name, text in cases.items():
        path.write_bytes(text)
        warnings = []
        for reader in (lambda: mzml_io.read_chunks_device(str(path), H.FakeContext(lib), 8192), lambda: mzml_io.read_chunks(str(path))):
            caplog.clear()
            with caplog.at_level(logging.WARNING, logger="falcon"):
                rows = MC.chunk_rows(reader())
            warnings.append((rows, [r.getMessage() for r in caplog.records]))
        assert warnings[0] == warnings[1], name
        assert len(warnings[1][1]) == (1 if name.startswith("cut") else 0), name


def test_sizes(lib, tmp_path):
    path = tmp_path / "s.mzML"
    for spectra in ([], MC.corpus_spectra(1)):
        MC.W.write_mzml(path, spectra)
        got, want, _ = _both(lib, path)
        assert got == want and len(want[0]) == len(spectra)
    s = MC.corpus_spectra(1)
    s[0]["identifier"] = "i" * 10000
    MC.W.write_mzml(path, s)
    got, want, ctx = _both(lib, path)
    assert got == want and _statuses(lib, ctx) == [MC.OK]


def test_mutations_stay_decided_or_go_to_the_host(lib, tmp_path):
    muts, n = MC.mutations(tmp_path / "m.mzML")
    assert len(muts) > 40
    for name, text, target in muts:
        res = H.scan(lib, text)
        if target is None:
            assert res["flags"] or len(res["status"]) == n - 1, name
        else:
            assert res["flags"] or res["status"][target] == MC.HOST, name
