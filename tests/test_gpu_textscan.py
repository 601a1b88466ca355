"""The mark-table passes the MGF and the mzML reader share (`csrc/textscan.h`: a count walk of 16 bytes per lane and 4 KB per
block, a scan, the table walk) at their own edges, through `Context` only: marks on the first and last byte of a lane, of a tile
and of the text; the table's capacity of n / 4 + 2 entries from both sides; and line starts / tag positions whose spans end in a
later tile.  The references are `bytes.count` / `bytes.find`, the host reader `mgf_io.get_spectra` and the host build of
`mzmlscan.h` (`tests/hostbuild_mzml.py`)."""
import io
import itertools

import numpy as np
import pytest

from falcon_amd import _lib
from falcon_amd.ms_io import mgf_io
from tests import hostbuild_mzml as HM
from tests import mzml_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _dev(ctx, text: bytes):
    import torch
    return ctx.to_dev(np.frombuffer(bytearray(text), np.uint8)) if text else ctx.empty((0,), torch.uint8)


def _marked(n, positions, mark: bytes):
    text = bytearray(b"a" * n)
    for p in positions:
        text[p:p + 1] = mark
    return bytes(text)


# ---- 1. counts at lane and tile edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193])
def test_counts_with_marks_on_lane_and_tile_edges(ctx, n):
    edges = sorted({p for p in (0, 15, 16, 4095, 4096, n - 1) if 0 <= p < n})
    for k in range(len(edges) + 1):
        for positions in itertools.combinations(edges, k):
            text = _marked(n, positions, b"\n")
            assert ctx.mgf_index(_dev(ctx, text))[3] == text.count(b"\n") + 1, (n, positions)
            text = _marked(n, positions, b"<")
            assert ctx.mzml_index(_dev(ctx, text))[3] == text.count(b"<"), (n, positions)


# ---- 2. the capacity boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at_end", [False, True], ids=["front", "back"])
@pytest.mark.parametrize("n", [16, 4096])
def test_table_capacity_from_both_sides(ctx, n, at_end):
    cap = n // 4 + 2

    def text_of(marks, mark):
        return b"a" * (n - marks) + mark * marks if at_end else mark * marks + b"a" * (n - marks)

    spectra, _, flags, tags = ctx.mzml_index(_dev(ctx, text_of(cap, b"<")))
    assert tags == cap and not flags & _lib.MZML_FLAG_TAGS
    spectra, _, flags, tags = ctx.mzml_index(_dev(ctx, text_of(cap + 1, b"<")))
    assert tags == cap + 1 and flags & _lib.MZML_FLAG_TAGS and spectra == 0
    spectra, _, flags, lines = ctx.mgf_index(_dev(ctx, text_of(cap - 1, b"\n")))
    assert lines == cap and not flags & _lib.MGF_FLAG_LINES
    spectra, _, flags, lines = ctx.mgf_index(_dev(ctx, text_of(cap, b"\n")))
    assert lines == cap + 1 and flags & _lib.MGF_FLAG_LINES and spectra == 0


# ---- 3. positions ---------------------------------------------------------------------------------------------------------------
MGF_SPECTRA = b"BEGIN IONS\nTITLE=first\nPEPMASS=500.5\n200.5 3\n100.25 1\nEND IONS\n" \
              b"BEGIN IONS\nTITLE=second\nPEPMASS=612.25\nCHARGE=2+\n150.5 2\nEND IONS\n"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("filler", [15, 16, 4095, 4096])
def test_mgf_line_starts_behind_a_newline_on_a_lane_or_tile_edge(ctx, filler):
    from falcon_amd.falcon import _raw_csr
    text = b"#" + b"a" * (filler - 1) + b"\n" + MGF_SPECTRA
    assert text.index(b"\n") == filler
    spans, pos = [], 0
    for _ in range(2):
        a = text.find(b"BEGIN IONS", pos)
        pos = text.find(b"\n", text.find(b"END IONS", a)) + 1
        spans.append([a, pos])
    specs = list(mgf_io.get_spectra(io.StringIO(text.decode("ascii"))))
    mz, it, indptr = _raw_csr(specs)[:3]
    res = ctx.parse_mgf(text)
    assert res["flags"] == 0 and res["lines"] == text.count(b"\n") + 1
    assert res["span"].tolist() == spans
    assert len(specs) == 2 and res["status"].tolist() == [0, 0]
    assert np.array_equal(res["indptr"].cpu().numpy(), indptr)
    assert np.array_equal(_bits(res["mz"].cpu().numpy()), _bits(mz)) and np.array_equal(_bits(res["intensity"].cpu().numpy()), _bits(it))
    assert [text[a:b].decode() for a, b in res["title"]] == [s["identifier"] for s in specs]


@pytest.fixture(scope="module")
def mzml_reference(tmp_path_factory):
    """the host build of the scan, and two spectra of the test writer"""
    tmp = tmp_path_factory.mktemp("textscan")
    path = tmp / "two.mzML"
    MC.W.write_mzml(path, MC.corpus_spectra(2))
    return HM.build(tmp), b"".join(MC.split_file(path.read_bytes())[1])


@pytest.mark.parametrize("filler", [0, 15, 16, 4095, 4096, 4097])
def test_mzml_tag_positions_behind_filler_to_a_lane_or_tile_edge(ctx, mzml_reference, filler):
    lib, spectra = mzml_reference
    text = b" " * filler + spectra
    want, got = HM.scan(lib, text), ctx.scan_mzml(text)
    assert want["flags"] == 0 and len(want["status"]) == 2 and want["tags"] == text.count(b"<")
    assert sorted(got) == sorted(want)
    for key in ("flags", "tags", "inside"):
        assert got[key] == want[key], key
    for key in ("status", "id", "span", "precursor_mz", "charge", "retention_time", "arrays"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    # (the device payload has room for n_bytes + 16 n; the arrays' rows address what the host build laid out)
    assert got["payload"].cpu().numpy()[:len(want["payload"])].tobytes() == want["payload"].tobytes()
