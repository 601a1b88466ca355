"""The cluster CSV's rows through the device writer (DESIGN.md "Cluster CSV out of the device"): column blocks in, the rows that
`falcon._write_outputs` sorts and `falcon._write_cluster_info` writes out, byte for byte.  The host writer stays the writer of
record: it writes the header, and the whole file wherever the device path does not mirror it (`device_columns` says why)."""
import csv
import io
import logging
import sys

import numpy as np

from . import mgf_io

logger = logging.getLogger("falcon")

COLUMNS = ["filename", "spectrum_id", "precursor_charge", "precursor_mz", "retention_time", "cluster"]
_QUOTES_CR = None


def host_quotes_cr() -> bool:
    """does this interpreter's csv module quote a field for a bare carriage return, with the line terminator the host writer
    uses?  (CPython 3.13 on does; before, only the terminator's own characters count)"""
    global _QUOTES_CR
    if _QUOTES_CR is None:
        out = io.StringIO()
        csv.writer(out, quoting=csv.QUOTE_MINIMAL, lineterminator="\n").writerow(["\r", ""])
        _QUOTES_CR = out.getvalue().startswith('"')
    return _QUOTES_CR


def column_block(filename, identifier, charge, precursor_mz, retention_time, cluster):
    """one block of rows as columns: `charge` is the partition's key ("None", or the integer's text) or an int"""
    z = 0 if charge in (None, "None") else int(charge)
    return dict(filename=filename, identifier=identifier, charge=z, precursor_mz=precursor_mz, retention_time=retention_time,
                cluster=cluster)


def block_tuples(blocks):
    """the blocks -> the tuples the host writer takes, in the blocks' order"""
    for b in blocks:
        charge = "None" if b["charge"] == 0 else str(b["charge"])
        for i in range(len(b["cluster"])):
            yield (str(b["filename"][i]), str(b["identifier"][i]), charge, np.float32(b["precursor_mz"][i]),
                   np.float32(b["retention_time"][i]), int(b["cluster"][i]))


def file_ranks(filename, key):
    """the filename column -> (file_id i32[n] into `names`, names: the distinct names, rank i32 per name): the runs of equal names
    from one vectorised compare, `key` (the natural key) of the distinct names only; names with equal keys share a rank"""
    filename = np.asarray(filename, dtype=str)
    n = len(filename)
    if n == 0:
        return np.zeros(0, np.int32), [], np.zeros(0, np.int32)
    starts = np.concatenate([[0], np.flatnonzero(filename[1:] != filename[:-1]) + 1])
    names, run_id = [], np.zeros(len(starts), np.int32)
    seen = {}
    for k, name in enumerate(filename[starts].tolist()):          # (a loop over the runs, not over the rows)
        if name not in seen:
            seen[name] = len(names)
            names.append(name)
        run_id[k] = seen[name]
    keys = [key(name) for name in names]
    distinct = sorted({_freeze(k) for k in keys})
    rank = np.array([distinct.index(_freeze(k)) for k in keys], np.int32)
    return np.repeat(run_id, np.diff(np.concatenate([starts, [n]]))), names, rank


def _freeze(key):
    return tuple(key)


def device_columns(blocks, key):
    """column blocks -> (columns for `Context.csv_order` / `Context.format_csv`, None), or (None, why the host writer has to
    write the file)"""
    for b in blocks:
        for name, dtype in (("precursor_mz", np.float32), ("retention_time", np.float32)):
            if np.asarray(b[name]).dtype != dtype:
                return None, f"a {name} column is {np.asarray(b[name]).dtype}, not the partitions' {np.dtype(dtype)}"
        if np.asarray(b["cluster"]).dtype.kind not in "iu" or not isinstance(b["charge"], int) or abs(b["charge"]) >= 2 ** 31:
            return None, "a cluster or charge column is not an integer column"
        for name in ("filename", "identifier"):
            if np.asarray(b[name]).dtype.kind != "U":
                return None, f"a {name} column holds no str"
    cat = lambda name, dtype: (np.concatenate([np.asarray(b[name], dtype) for b in blocks]) if blocks else np.zeros(0, dtype))
    ident = mgf_io.title_blob(cat("identifier", str))
    if ident is None:
        return None, "an identifier holds a newline or cannot be written as plain bytes"
    if (ident[0] >= 0x80).any():
        return None, "an identifier holds a non-ASCII byte"
    file_id, names, rank = file_ranks(cat("filename", str), key)
    fn = mgf_io.title_blob(np.array(names, dtype=str))
    if fn is None:
        return None, "a file name holds a newline or cannot be written as plain bytes"
    if (ident[0] == 0).any() or (fn[0] == 0).any():
        return None, "a field holds a NUL byte (csv.writer decides whether it can be written)"
    charge = (np.concatenate([np.full(len(b["cluster"]), b["charge"], np.int32) for b in blocks]) if blocks else np.zeros(0, np.int32))
    cols = dict(file_id=file_id, file_names=fn[0], file_name_ptr=fn[1], ident=ident[0], id_ptr=ident[1], charge=charge,
                precursor_mz=cat("precursor_mz", np.float32), retention_time=cat("retention_time", np.float32),
                cluster=cat("cluster", np.int64), file_rank=rank[file_id] if len(file_id) else np.zeros(0, np.int32))
    return cols, None


def digit_run_limit() -> int:
    """the longest digit run `int()` of the host key takes (0: any)"""
    get = getattr(sys, "get_int_max_str_digits", None)
    return int(get()) if get else 0


def sort_rows(ctx, cols):
    """the columns of `device_columns` -> their rows' order on the device (`Context.csv_order`), or None when a digit run of an id
    is longer than `int()` of the host key takes (the host writer then decides what happens)"""
    if len(cols["ident"]):
        cols["ident"], cols["id_ptr"] = ctx._text_to_dev(cols["ident"]), ctx.to_dev(cols["id_ptr"])      # (one upload for both calls)
    order, longest = ctx.csv_order(cols["file_rank"], cols["ident"], cols["id_ptr"])
    limit = digit_run_limit()
    return None if limit and longest > limit else order


def write_rows(out, ctx, cols, order, max_bytes=None) -> None:
    """append the rows' text, in `order`, to the binary file `out`"""
    columns = {k: v for k, v in cols.items() if k != "file_rank"}
    for chunk in ctx.format_csv(**columns, order=order, max_bytes=max_bytes, copy=False):
        out.write(memoryview(chunk))
