"""The cluster CSV writer on the GPU (`fal_csv_order`, `fal_csv_write_sizes`, `fal_csv_write`, `Context.format_csv`, `--csv_writer`):
the device's row order is the host's stable sort by `_natural_key`, and the device-written text is byte for byte what
`falcon._write_cluster_info` -- the writer of record -- writes for the same rows."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import csvwrite_cases as K

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


def expected(name, tmp_dir) -> list:
    """`_write_cluster_info`'s bytes of a case set, row by row, computed once"""
    if name not in _WANT:
        body = K.body_of(getattr(K, name)().tuples(through_numpy=True), tmp_dir)
        rows = getattr(K, name)()
        # (cut behind every row: a quoted field may hold a '\r' but never a '\n')
        texts = body.split(b"\n")
        assert texts[-1] == b"" and len(texts) == len(rows) + 1
        _WANT[name] = [t + b"\n" for t in texts[:-1]]
    return _WANT[name]


def columns_of(rows, order=None):
    """the arguments of `format_csv` / `_csv_columns` for a case set (one file name per row: the distinct names in first-seen order)"""
    from falcon_amd.ms_io import mgf_io
    fn = np.array(rows.filename, dtype=str).tolist()
    names = list(dict.fromkeys(fn))
    where = {name: i for i, name in enumerate(names)}
    file_id = np.array([where[f] for f in fn], np.int32)
    fn_blob, id_blob = mgf_io.title_blob(np.array(names, dtype=str)), mgf_io.title_blob(np.array(rows.identifier, dtype=str))
    assert fn_blob is not None and id_blob is not None
    return dict(file_id=file_id, file_names=fn_blob[0], file_name_ptr=fn_blob[1], ident=id_blob[0], id_ptr=id_blob[1], charge=rows.charge,
                precursor_mz=rows.precursor_mz, retention_time=rows.retention_time, cluster=rows.cluster, order=order)


# ---- the checks (also run by tests/csvwrite_poison_worker.py in a process under FALCON_DEBUG_POISON=1) ---------------------------
ORDER_SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 20000]      # the sort's block of 1,024 and its merge-path cut +- 1


def check_order(ctx, n):
    from falcon_amd.ms_io import mgf_io
    file_rank, ids = K.order_pool(n)
    blob, ptr = mgf_io.title_blob(np.array(ids, dtype=str)) if n else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
    order, longest = ctx.csv_order(file_rank, blob, ptr)
    assert order.cpu().tolist() == K.host_order(file_rank, ids)
    assert longest == (max(K_digit_run(s) for s in ids) if n else 0)


def K_digit_run(s: str) -> int:
    import re
    return max((len(m) for m in re.findall(r"\d+", s)), default=0)


def check_bad_id_ptr(ctx):
    from falcon_amd._lib import FAL_EINVAL, FalconHipError
    from falcon_amd.ms_io import mgf_io
    file_rank, ids = K.order_pool(200)
    blob, ptr = mgf_io.title_blob(np.array(ids, dtype=str))
    for at, value in ((0, -1), (200, len(blob) + 1), (100, int(ptr[99]) - 1), (7, 2 ** 40)):
        bad = ptr.copy()
        bad[at] = value
        with pytest.raises(FalconHipError, match=f"code {FAL_EINVAL}:"):
            ctx.csv_order(file_rank, blob, bad)
    assert ctx.csv_order(file_rank, blob, ptr)[0].cpu().tolist() == K.host_order(file_rank, ids)


def check_case_set(ctx, name, tmp_dir, **options):
    rows = getattr(K, name)()
    want = b"".join(expected(name, tmp_dir))
    got = b"".join(c.tobytes() for c in ctx.format_csv(**columns_of(rows), **options))
    assert len(got) == len(want)
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{name}: first difference at byte {at}: {got[max(at - 60, 0):at + 40]!r} != {want[max(at - 60, 0):at + 40]!r}")


def check_permuted(ctx, tmp_dir):
    """rows read through `order`: a shuffle with repeats"""
    rows = K.ascii_rows()
    texts = expected("ascii_rows", tmp_dir)
    order = np.random.default_rng(9).integers(0, len(rows), 2 * len(rows)).astype(np.int32)
    got = b"".join(c.tobytes() for c in ctx.format_csv(**columns_of(rows, order)))
    assert got == b"".join(texts[i] for i in order)


def check_chunking(ctx, tmp_dir):
    rows = K.long_rows()
    texts = expected("long_rows", tmp_dir)
    sizes = [len(t) for t in texts]
    for max_bytes in (4096, 1):
        chunks = [c.tobytes() for c in ctx.format_csv(**columns_of(rows), max_bytes=max_bytes)]
        assert b"".join(chunks) == b"".join(texts)
        lens = [len(c) for c in chunks]
        if max_bytes == 1:
            assert lens == sizes                                   # a row a chunk
        else:
            assert len(chunks) > 3 and max(lens) > 4096            # many chunks, and a long row grows its own
            assert all(n <= 4096 or n in sizes for n in lens)      # a chunk above the target is one row
    assert all(c.endswith(b"\n") for c in chunks)


def check_bounds(ctx, tmp_dir):
    import torch
    from falcon_amd._lib import FAL_EINVAL, FalconHipError
    rows = K.long_rows()
    texts = expected("long_rows", tmp_dir)
    cols = ctx._csv_columns(**columns_of(rows))
    sizes, offsets, total = ctx.csv_write_sizes(cols)
    assert sizes.cpu().tolist() == [len(t) for t in texts] and total == sum(len(t) for t in texts)
    assert offsets.cpu().tolist() == [0] + list(np.cumsum([len(t) for t in texts]))
    n = len(rows)
    for first, last, front in ((0, n, 16), (5, 23, 7), (7, 8, 1), (9, 10, 3), (4, 4, 3), (60, n, 5), (13, 13 + 64, 9)):
        want = b"".join(texts[first:last])
        buf = torch.full((front + len(want) + 37,), SENTINEL, dtype=torch.uint8, device=ctx.tdev)
        ctx.csv_write(cols, offsets, first, last, buf[front:front + len(want)])
        got = buf.cpu().numpy()
        assert got[front:front + len(want)].tobytes() == want
        assert (got[:front] == SENTINEL).all() and (got[front + len(want):] == SENTINEL).all()
        if len(want):
            buf.fill_(SENTINEL)                                    # one byte too few: FAL_EINVAL, nothing written
            with pytest.raises(FalconHipError, match=f"code {FAL_EINVAL}:"):
                ctx.csv_write(cols, offsets, first, last, buf[front:front + len(want) - 1])
            assert (buf.cpu().numpy() == SENTINEL).all()
    # every alignment of `out`: rows [5, 5 + 70) are two tiles of 64 rows, with rows longer than a tile among them
    want = b"".join(texts[5:75])
    assert max(len(t) for t in texts[5:75]) == max(len(t) for t in texts) > 8192
    for front in range(16):
        buf = torch.full((front + len(want) + 37,), SENTINEL, dtype=torch.uint8, device=ctx.tdev)
        ctx.csv_write(cols, offsets, 5, 75, buf[front:front + len(want)])
        got = buf.cpu().numpy()
        assert got[front:front + len(want)].tobytes() == want, front
        assert (got[:front] == SENTINEL).all() and (got[front + len(want):] == SENTINEL).all(), front
    # offsets that are not the columns': FAL_EINVAL, and every store stays inside the buffer
    wrong = offsets.clone()
    wrong[3:] += 1
    buf = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device=ctx.tdev)
    with pytest.raises(FalconHipError, match=f"code {FAL_EINVAL}:"):
        ctx.csv_write(cols, wrong, 0, n, buf[16:16 + total + 1])
    got = buf.cpu().numpy()
    assert (got[:16] == SENTINEL).all() and (got[16 + total + 1:] == SENTINEL).all()


def run_all(ctx, tmp_dir):
    for n in ORDER_SIZES:
        check_order(ctx, n)
    check_bad_id_ptr(ctx)
    for name in K.ROW_SETS:
        check_case_set(ctx, name, tmp_dir)
    check_permuted(ctx, tmp_dir)
    check_chunking(ctx, tmp_dir)
    check_bounds(ctx, tmp_dir)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ORDER_SIZES)
def test_order_equals_the_host_sort(ctx, n):
    """3 file ranks, ids with long shared prefixes, exact duplicates and leading-zero ties, shuffled: `order` is
    `sorted(range(n), key=(rank, _natural_key))` exactly, ties in input order"""
    check_order(ctx, n)


def test_bad_id_ptr_is_einval(ctx):
    check_bad_id_ptr(ctx)


@pytest.mark.parametrize("name", K.ROW_SETS)
def test_device_text_equals_write_cluster_info(ctx, name, tmp_path_factory):
    check_case_set(ctx, name, tmp_path_factory.mktemp("want"))


def test_rows_through_an_order_with_repeats(ctx, tmp_path_factory):
    check_permuted(ctx, tmp_path_factory.mktemp("want"))


def test_no_rows_give_no_chunks(ctx):
    assert list(ctx.format_csv(**columns_of(K.ascii_rows().take([])))) == []


def test_chunks_of_4_kb_and_of_one_byte(ctx, tmp_path_factory):
    check_chunking(ctx, tmp_path_factory.mktemp("want"))


def test_write_stays_inside_its_buffer(ctx, tmp_path_factory):
    """sentinels in front of and behind a tensor view stay, for ranges that begin and end inside tiles and at rows longer than a
    tile; a view one byte too small: FAL_EINVAL and an untouched buffer"""
    check_bounds(ctx, tmp_path_factory.mktemp("want"))


def test_write_outputs_sorts_and_writes_blocks_on_the_device(ctx, tmp_path, caplog):
    """`falcon._write_outputs` with column blocks: the file of the tuple path, header included"""
    from falcon_amd import falcon
    from falcon_amd.config import config
    file_rank, ids = K.order_pool(3000)
    names = np.array(["b10.mgf", "b9.mgf", 'a "1",2.mgf'])[file_rank]
    rng = np.random.default_rng(2)
    blocks, tuples = [], []
    for z, (a, b) in zip((2, 0, -1), ((0, 1000), (1000, 1900), (1900, 3000))):
        rows = K.Rows(names[a:b], ids[a:b], np.full(b - a, z), rng.uniform(100, 2000, b - a), rng.uniform(0, 9000, b - a),
                      rng.integers(0, 700, b - a))
        blocks.append(rows.block())
        tuples += rows.tuples(through_numpy=True)
    tuples.sort(key=lambda r: (falcon._natural_key(r[0]), falcon._natural_key(r[1])))
    config.parse(["in.mgf", str(tmp_path / "host"), "--work_dir", "w"])
    falcon._write_cluster_info(tuples)
    config.parse(["in.mgf", str(tmp_path / "device"), "--work_dir", "w"])
    with caplog.at_level(logging.DEBUG, logger="falcon"):
        falcon._write_outputs([], [], ctx, csv_blocks=blocks)
    assert open(tmp_path / "device.csv", "rb").read() == open(tmp_path / "host.csv", "rb").read()
    assert not [r for r in caplog.records if "the host writer writes" in r.getMessage()]
    unique = len({t[5] for t in tuples})
    assert [r for r in caplog.records if f"3000 spectra to {unique} unique clusters" in r.getMessage()]


def test_every_check_again_under_debug_poison(tmp_path):
    """FALCON_DEBUG_POISON=1 is read once per process: a fresh child runs the order, text, chunking and bounds checks again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "csvwrite_poison_worker.py"), str(tmp_path)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _input_mgf(path, title=lambda i: f'run "A", fraction {i % 7}.{i}.{i}.2 File:"run A.raw", NativeID:"scan={i}"'):
    from falcon_amd.ms_io import ms_io
    from tests import consensus_cases as cc
    d = cc.template_spectra(5, n_templates=6, n_spectra=120, n_peaks=30)
    specs = []
    for i in range(len(d["precursor_mz"])):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        specs.append({"identifier": title(i), "precursor_mz": float(d["precursor_mz"][i]), "precursor_charge": 2 + i % 2,
                      "retention_time": float(d["retention_time"][i]), "mz": d["mz"][a:b].astype(np.float64),
                      "intensity": d["intensity"][a:b]})
    ms_io.write_spectra(path, specs)
    return specs


def _cli(args):
    from falcon_amd.falcon import main
    assert main(args) == 0


def test_cli_writes_the_same_csv_with_either_writer(tmp_path, caplog):
    """titles with quotes, commas and spaces: `--csv_writer device` and `host` give one file (one work directory: the header names
    it); the same with `--assign_to` over the first run's representatives; a non-ASCII title goes through the logged host fallback"""
    mgf = str(tmp_path / "in.mgf")
    specs = _input_mgf(mgf)
    common = ["--work_dir", str(tmp_path / "work"), "--overwrite", "--eps", "0.35", "--export_representatives"]
    out = {}
    with caplog.at_level(logging.DEBUG, logger="falcon"):
        for writer in ("host", "device"):
            out[writer] = str(tmp_path / f"first_{writer}")
            _cli([mgf, out[writer], *common, "--csv_writer", writer])
    assert not [r for r in caplog.records if "the host writer writes" in r.getMessage()]
    host, dev = (open(out[w] + ".csv", "rb").read() for w in ("host", "device"))
    assert dev == host and host.count(b"\n") > 120 and b'"run ""A"", fraction' in host and b"csv_writer" not in host
    from falcon_amd.ms_io import ms_io
    more = str(tmp_path / "more.mgf")
    ms_io.write_spectra(more, [dict(s, identifier=f'again "{k}", 0{k}') for k, s in enumerate(specs[::3])])
    csvs = []
    for writer in ("host", "device"):
        o = str(tmp_path / f"assign_{writer}")
        _cli([more, o, "--work_dir", str(tmp_path / "work_assign"), "--overwrite", "--eps", "0.35", "--assign_to", out["host"] + ".mgf",
              "--csv_writer", writer])
        csvs.append(open(o + ".csv", "rb").read())
    assert csvs[0] == csvs[1] and b'"again ""0"", 00"' in csvs[0]
    # one non-ASCII title: the host writer writes the file, and says so once
    odd = str(tmp_path / "odd.mgf")
    _input_mgf(odd, title=lambda i: f"münchen scan={i}" if i == 17 else f"scan={i}")
    caplog.clear()
    csvs = []
    with caplog.at_level(logging.DEBUG, logger="falcon"):
        for writer in ("host", "device"):
            o = str(tmp_path / f"odd_{writer}")
            _cli([odd, o, "--work_dir", str(tmp_path / "work_odd"), "--overwrite", "--eps", "0.35", "--csv_writer", writer])
            csvs.append(open(o + ".csv", "rb").read())
    assert csvs[0] == csvs[1] and "münchen scan=17".encode() in csvs[0]
    assert len([r for r in caplog.records if "the host writer writes" in r.getMessage()]) == 1
