"""Host build of `csrc/recwrite.h` (the record writer's field values, XML character data and unit layout) for the CPU tests: the
header the kernels include, compiled by the host C++ compiler behind `extern "C"` entry points (`tests/hostbuild.py`'s compiler
choice and flags)."""
import ctypes as C

import numpy as np

from falcon_amd._lib import REC_KINDS, RecField
from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include "recwrite.h"

extern "C" {

int t_field_bytes() { return (int)sizeof(fal::RecField); }
int t_limits(int which) { return which == 0 ? fal::kRecMaxFields : which == 1 ? fal::kRecLitMax : which == 2 ? fal::kRecNumMax : fal::kRecEntityMax; }

static fal::RecTable table_of(const fal::RecField* fields, int n_fields, const int32_t* head_tail) {
    fal::RecTable t = fal::RecTable();
    for (int j = 0; j < n_fields; ++j) t.f[j] = fields[j];
    t.n_fields = n_fields;
    t.head[0] = head_tail[0], t.head[1] = head_tail[1], t.tail[0] = head_tail[2], t.tail[1] = head_tail[3];
    return t;
}

// units [0, n): the sizing function's length and its bad flag
void t_unit_lens(const fal::RecField* fields, int n_fields, const int32_t* head_tail, int64_t n, int64_t* len, int32_t* bad) {
    const fal::RecTable t = table_of(fields, n_fields, head_tail);
    for (int64_t u = 0; u < n; ++u) {
        bool b = false;
        len[u] = fal::rec_unit_len(t, u, &b);
        bad[u] = b;
    }
}

// units [0, n) back to back at dst + at[u] -> written[u]
void t_units(const fal::RecField* fields, int n_fields, const int32_t* head_tail, const uint8_t* lit, int64_t n, const int64_t* at, uint8_t* dst,
             int64_t* written) {
    const fal::RecTable t = table_of(fields, n_fields, head_tail);
    for (int64_t u = 0; u < n; ++u) written[u] = fal::rec_write_unit(dst + at[u], t, lit, u);
}

int64_t t_xml(const uint8_t* p, int64_t n, uint8_t* dst, int64_t* len_only, int32_t* bad) {
    bool b = false;
    *len_only = fal::rec_xml_len(p, n, &b);
    *bad = b;
    return fal::rec_xml_write(dst, p, n);
}

}  // extern "C"
"""

GUARD = 0xA5


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "records_shim", SHIM)
    p = C.c_void_p
    lib.t_field_bytes.restype = C.c_int
    lib.t_limits.argtypes, lib.t_limits.restype = [C.c_int], C.c_int
    lib.t_unit_lens.argtypes, lib.t_unit_lens.restype = [p, C.c_int, p, C.c_int64, p, p], None
    lib.t_units.argtypes, lib.t_units.restype = [p, C.c_int, p, p, C.c_int64, p, p, p], None
    lib.t_xml.argtypes, lib.t_xml.restype = [p, C.c_int64, p, p, p], C.c_int64
    return lib


def host_table(table):
    """a record table of `Context.format_records` over host arrays -> (RecField array, head / tail ranges i32[4], literal blob,
    the arrays kept alive)"""
    dtypes = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "text": np.uint8}
    blob, keep = bytearray(), []

    def literal(b):
        at = len(blob)
        blob.extend(bytes(b))
        return at, len(blob)

    head_tail = np.array([*literal(table["head"]), *literal(table["tail"])], np.int32)
    recs = (RecField * max(len(table["fields"]), 1))()
    for rec, f in zip(recs, table["fields"]):
        col = np.ascontiguousarray(np.asarray(f["column"]), dtypes[f["kind"]])
        col = np.concatenate([col, np.zeros(1, col.dtype)])          # (never NULL)
        ptr = None if f["kind"] != "text" else np.ascontiguousarray(f["ptr"], np.int64)
        index = None if f.get("index") is None else np.ascontiguousarray(f["index"], np.int32)
        keep += [col, ptr, index]
        rec.column = col.ctypes.data
        rec.ptr = None if ptr is None else ptr.ctypes.data
        rec.index = None if index is None else (index.ctypes.data if len(index) else np.zeros(1, np.int32).ctypes.data)
        rec.rows = len(ptr) - 1 if ptr is not None else len(col) - 1
        rec.blob_bytes = len(col) - 1 if ptr is not None else 0
        rec.kind = REC_KINDS[f["kind"]]
        rec.prefix[:], rec.suffix[:] = literal(f["prefix"]), literal(f["suffix"])
    lit = np.frombuffer(bytes(blob) + b"\x00", np.uint8).copy()
    return recs, head_tail, lit, keep


def units(lib, table):
    """-> (every unit's bytes, the sizing function's lengths, its bad flags, guard bytes behind the text intact)"""
    recs, head_tail, lit, keep = host_table(table)
    n, nf = int(table["n"]), len(table["fields"])
    lens, bad = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
    lib.t_unit_lens(C.cast(recs, C.c_void_p), nf, _p(head_tail), n, _p(lens), _p(bad))
    lens, bad = lens[:n], bad[:n]
    at = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dst = np.full(int(at[-1]) + 64, GUARD, np.uint8)
    written = np.zeros(max(n, 1), np.int64)
    lib.t_units(C.cast(recs, C.c_void_p), nf, _p(head_tail), _p(lit), n, _p(at), _p(dst), _p(written))
    raw = dst.tobytes()
    return [raw[at[u]:at[u] + written[u]] for u in range(n)], lens, bad, bool((dst[at[-1]:] == GUARD).all())


def xml(lib, s: bytes):
    """-> (character data, the length function's count, outside the grammar?)"""
    src = np.frombuffer(s + b"\x00", np.uint8).copy()
    dst = np.full(5 * len(s) + 16, GUARD, np.uint8)
    only, bad = C.c_int64(0), C.c_int32(0)
    got = lib.t_xml(_p(src), len(s), _p(dst), C.byref(only), C.byref(bad))
    return dst[:got].tobytes(), int(only.value), bool(bad.value)
