"""The MGF writer on the GPU (`fal_mgf_write_sizes`, `fal_mgf_write`, `Context.format_mgf`, `mgf_io.write_representatives`,
`--mgf_writer`): the device-written text is byte for byte what `mgf_io.write_spectra` -- the writer of record -- writes for the
same entries."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mgfwrite_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


_WANT = {}


def expected(name) -> bytes:
    """`write_spectra`'s bytes of a case set, computed once"""
    if name not in _WANT:
        _WANT[name] = getattr(K, name)().expected()
    return _WANT[name]


def blob_of(e):
    from falcon_amd.ms_io import mgf_io
    blob = mgf_io.title_blob(e.title)
    assert blob is not None
    return blob


def device_text(ctx, e, **options) -> list:
    """the chunks `format_mgf` yields for the entries, as bytes"""
    title, ptr = blob_of(e)
    return [c.tobytes() for c in ctx.format_mgf(e.mz, e.intensity, e.indptr, e.rows, e.precursor_mz, e.retention_time, e.charge,
                                                e.cluster, title, ptr, **options)]


# ---- the checks (also run by tests/mgfwrite_poison_worker.py in a process under FALCON_DEBUG_POISON=1) ---------------------------
def check_case_set(ctx, name):
    e = getattr(K, name)()
    got = b"".join(device_text(ctx, e))
    want = expected(name)
    assert len(got) == len(want)
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{name}: first difference at byte {at}: {got[max(at - 60, 0):at + 40]!r} != {want[max(at - 60, 0):at + 40]!r}")


def check_chunking(ctx):
    e = K.entry_cases()
    want = expected("entry_cases")
    sizes = [len(c) for c in _entry_texts(e)]
    for max_bytes in (4096, 1):
        chunks = device_text(ctx, e, max_bytes=max_bytes)
        assert b"".join(chunks) == want
        lens = [len(c) for c in chunks]
        if max_bytes == 1:
            assert lens == sizes                                   # an entry a chunk
        else:
            assert len(chunks) > 3 and max(lens) > 4096            # many chunks, and the raw-sized entry grows its own
            assert all(n <= 4096 or n in sizes for n in lens)      # a chunk above the target is one entry
            assert sum(lens) == sum(sizes)


def _entry_texts(e):
    return [e.take([k]).expected() for k in range(len(e))]


def check_bounds(ctx):
    import torch
    from falcon_amd._lib import FAL_EINVAL, FalconHipError
    e = K.shuffled_rows()
    title, ptr = blob_of(e)
    cols = ctx._mgf_entries(e.mz, e.intensity, e.indptr, e.rows, e.precursor_mz, e.retention_time, e.charge, e.cluster, title, ptr)
    sizes, offsets, total = ctx.mgf_write_sizes(cols)
    texts = _entry_texts(e)
    assert sizes.cpu().tolist() == [len(t) for t in texts] and total == sum(len(t) for t in texts)
    assert offsets.cpu().tolist() == [0] + list(np.cumsum([len(t) for t in texts]))
    for first, last, front in ((0, len(e), 16), (5, 23, 7), (9, 10, 1), (4, 4, 3)):
        want = b"".join(texts[first:last])
        buf = torch.full((front + len(want) + 37,), SENTINEL, dtype=torch.uint8, device=ctx.tdev)
        ctx.mgf_write(cols, offsets, first, last, buf[front:front + len(want)])
        got = buf.cpu().numpy()
        assert got[front:front + len(want)].tobytes() == want
        assert (got[:front] == SENTINEL).all() and (got[front + len(want):] == SENTINEL).all()
        if len(want):
            buf.fill_(SENTINEL)                                    # one byte too few: FAL_EINVAL, nothing written
            with pytest.raises(FalconHipError, match=f"code {FAL_EINVAL}:"):
                ctx.mgf_write(cols, offsets, first, last, buf[front:front + len(want) - 1])
            assert (buf.cpu().numpy() == SENTINEL).all()
    want = b"".join(texts[5:23])                                   # every alignment of `out`
    for front in range(16):
        buf = torch.full((front + len(want) + 37,), SENTINEL, dtype=torch.uint8, device=ctx.tdev)
        ctx.mgf_write(cols, offsets, 5, 23, buf[front:front + len(want)])
        got = buf.cpu().numpy()
        assert got[front:front + len(want)].tobytes() == want, front
        assert (got[:front] == SENTINEL).all() and (got[front + len(want):] == SENTINEL).all(), front


def check_round_trip(ctx):
    e = K.entry_cases()
    keep = [k for k in range(len(e)) if len(str(e.title[k]).encode("utf-8")) < 4000 and str(e.title[k]).isascii()]
    assert len(keep) == len(e) - 2 and set(K.PEAK_COUNTS) <= {int(e.indptr[r + 1] - e.indptr[r]) for r in e.rows[keep]}
    e = e.take(keep)
    text = b"".join(device_text(ctx, e))
    res = ctx.parse_mgf(text)
    assert res["flags"] == 0 and len(res["status"]) == len(e) and not res["status"].any()
    indptr = res["indptr"].cpu().numpy()
    mz, it = res["mz"].cpu().numpy(), res["intensity"].cpu().numpy()
    for k, r in enumerate(e.rows):
        a, b = e.indptr[r], e.indptr[r + 1]
        order = np.argsort(e.mz[a:b].astype(np.float64), kind="stable")
        assert indptr[k + 1] - indptr[k] == b - a
        got_mz, got_it = mz[indptr[k]:indptr[k + 1]], it[indptr[k]:indptr[k + 1]]
        assert np.array_equal(got_mz.view(np.uint64), e.mz[a:b][order].astype(np.float64).view(np.uint64))
        assert np.array_equal(got_it.view(np.uint32), e.intensity[a:b][order].view(np.uint32))
    assert np.array_equal(res["precursor_mz"], e.precursor_mz.astype(np.float64))
    assert np.array_equal(res["retention_time"], e.retention_time.astype(np.float64))
    assert np.array_equal(res["has_charge"], e.charge != 0) and np.array_equal(res["charge"], e.charge)
    titles = [text[a:b].decode("ascii") for a, b in res["title"]]
    assert titles == [str(t).strip() for t in e.title]


CASE_SETS = ["entry_cases", "number_entries", "shuffled_rows"]


def run_all(ctx):
    for name in CASE_SETS:
        check_case_set(ctx, name)
    check_chunking(ctx)
    check_bounds(ctx)
    check_round_trip(ctx)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_SETS)
def test_device_text_equals_write_spectra(ctx, name):
    """entry_cases: 0 / 1 / 63 / 64 / 65 / 200 / 5,000 peaks, every charge form, cluster ids 0 and 2^40, titles of 0 / 1 / 255 /
    2,047 / 2,048 / 2,049 (around the title bytes the kernel appends per piece) / 5,000 bytes and a non-ASCII one, RT -1;
    number_entries: every exponent x the edge mantissas through the device compile of the formatter; shuffled_rows: `rows`
    shuffled with repeats (entry_cases has the identity of the consensus form)"""
    check_case_set(ctx, name)


def test_no_entries_give_an_empty_file(ctx, tmp_path):
    from falcon_amd.ms_io import ms_io
    e = K.entry_cases().take([])
    assert device_text(ctx, e) == []
    fn = str(tmp_path / "none.mgf")
    assert ms_io.write_representatives(fn, ctx, e.mz, e.intensity, e.indptr, e.rows, e.precursor_mz, e.retention_time, e.charge,
                                       e.cluster, e.title) == "device"
    assert os.path.getsize(fn) == 0


def test_chunks_of_4_kb_and_of_one_byte(ctx):
    check_chunking(ctx)


def test_write_stays_inside_its_buffer(ctx):
    """sentinels in front of and behind a tensor view stay; a view one byte too small: FAL_EINVAL and an untouched buffer"""
    check_bounds(ctx)


def test_reader_round_trip(ctx):
    check_round_trip(ctx)


def test_write_representatives_and_the_host_fallback(ctx, tmp_path):
    """the file front door: device tensors or arrays in, the writer of record's file out; a title with a newline sends the whole
    file to the host writer (which writes it as it always did)"""
    import torch
    from falcon_amd.ms_io import mgf_io, ms_io
    e = K.shuffled_rows()
    fn = str(tmp_path / "reps.mgf")
    dev = lambda a: torch.from_numpy(a).to(ctx.tdev)
    assert ms_io.write_representatives(fn, ctx, dev(e.mz), dev(e.intensity), dev(e.indptr), dev(e.rows), dev(e.precursor_mz),
                                       e.retention_time, e.charge, e.cluster, e.title, max_bytes=3000) == "device"
    assert open(fn, "rb").read() == expected("shuffled_rows")
    e.title = e.title.copy().astype(object)
    e.title[3] = "two\nlines"
    e.title = np.array(list(e.title), dtype=str)
    assert mgf_io.write_representatives(fn, ctx, e.mz, e.intensity, e.indptr, e.rows, e.precursor_mz, e.retention_time, e.charge,
                                        e.cluster, e.title) == "host"
    assert open(fn, "rb").read() == e.expected()
    with pytest.raises(ValueError):
        ms_io.write_representatives(str(tmp_path / "reps.mzML"), ctx)


def test_cluster_wrapper(ctx, tmp_path):
    from falcon_amd.cluster.cluster import ClusterPipeline, SpectrumDataset, write_representatives
    e = K.shuffled_rows()
    n_rows = len(e.indptr) - 1
    rng = np.random.default_rng(3)
    pmz, rt = rng.uniform(100, 900, n_rows).astype(np.float32), rng.uniform(0, 99, n_rows).astype(np.float32)
    ds = SpectrumDataset(pmz, rt, e.mz, e.intensity, e.indptr)
    fn = str(tmp_path / "w.mgf")
    assert write_representatives(fn, ds, e.rows, e.cluster, e.title, charge=3, pipeline=ClusterPipeline(ctx)) == "device"
    want = K.Entries(e.mz, e.intensity, e.indptr, e.rows, pmz[e.rows], rt[e.rows], np.full(len(e), 3), e.cluster, e.title)
    assert open(fn, "rb").read() == want.expected()


def test_every_check_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 is read once per process: a fresh child runs the case sets, chunking, bounds and round trip again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mgfwrite_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _input_mgf(path):
    from falcon_amd.ms_io import ms_io
    from tests import consensus_cases as cc
    d = cc.template_spectra(5, n_templates=6, n_spectra=120, n_peaks=30)
    specs = []
    for i in range(len(d["precursor_mz"])):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        specs.append({"identifier": f"scan={i}", "precursor_mz": float(d["precursor_mz"][i]), "precursor_charge": 2 + i % 2,
                      "retention_time": float(d["retention_time"][i]), "mz": d["mz"][a:b].astype(np.float64),
                      "intensity": d["intensity"][a:b]})
    ms_io.write_spectra(path, specs)
    return specs


def test_cli_writes_the_same_files_with_either_writer(tmp_path):
    """`--export_representatives` with `--mgf_writer host` and `device`, medoid and consensus representatives: the .mgf and the
    .csv are identical per pair; `--assign_to` over the device-written file gives the CSV it gives over the host-written one;
    the option is in no CSV header line; a bad value in a config file is a parse error"""
    from falcon_amd.falcon import main
    mgf = str(tmp_path / "in.mgf")
    specs = _input_mgf(mgf)
    out = {}
    for reps in ("medoid", "consensus"):
        for writer in ("host", "device"):
            o = out[reps, writer] = str(tmp_path / f"{reps}_{writer}")
            # (one work directory for the pair: the CSV header names it)
            assert main([mgf, o, "--work_dir", str(tmp_path / f"work_{reps}"), "--overwrite", "--eps", "0.35",
                         "--export_representatives", "--representatives", reps, "--mgf_writer", writer]) == 0
        host, dev = (open(out[reps, w] + ".mgf", "rb").read() for w in ("host", "device"))
        assert len(host) > 10000 and host.count(b"BEGIN IONS") >= 6 and dev == host
        csv_h, csv_d = (open(out[reps, w] + ".csv").read() for w in ("host", "device"))
        assert csv_h == csv_d and "mgf_writer" not in csv_h
    assert open(out["medoid", "host"] + ".mgf", "rb").read() != open(out["consensus", "host"] + ".mgf", "rb").read()
    from falcon_amd.ms_io import ms_io
    more = str(tmp_path / "more.mgf")
    ms_io.write_spectra(more, [dict(s, identifier=f"again={k}") for k, s in enumerate(specs[::3])])
    csvs = []
    for writer in ("host", "device"):
        o = str(tmp_path / f"assign_{writer}")
        os.replace(out["medoid", writer] + ".mgf", str(tmp_path / "library.mgf"))      # (one name: the header line names the file)
        assert main([more, o, "--work_dir", str(tmp_path / "work_assign"), "--overwrite", "--eps", "0.35", "--assign_to",
                     str(tmp_path / "library.mgf")]) == 0
        csvs.append(open(o + ".csv").read())
    assert csvs[0] == csvs[1] and "again=0" in csvs[0]
    from falcon_amd.config import Config
    ini = tmp_path / "falcon.ini"
    ini.write_text("export_representatives = true\nmgf_writer = gpu\n")
    with pytest.raises(SystemExit):
        Config().parse(f"in.mgf out -c {ini}")
