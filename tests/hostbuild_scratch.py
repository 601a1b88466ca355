"""Host build of `csrc/scratch.h` for the CPU tests: the layout type every host entry point cuts its scratch slots with, compiled
with the host C++ compiler (the header includes no HIP).  Two builds.  The SHIM is a shared object behind `extern "C"` entry
points, loaded with ctypes: its fake context records (slot, bytes) of every reserve and hands out a malloc of exactly `bytes`.
The PROGRAM is a stand-alone executable in the manner of tests/hostbuild_unionfind.py, run as a child process, nothing loaded
into Python: it declares the same layouts, reserves from a malloc of exactly bytes() and writes every array end to end -- built
with `-fsanitize=address,undefined` a clean exit shows that no array reaches past the block or sits misaligned."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.hostbuild import CSRC, compile_shim
from tests.hostbuild_unionfind import plain_compiler

ASAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
PLAIN = ("-O2",)

# element kinds of the generic entry point
U8, I32, I64, F64, PAD = 0, 1, 2, 3, 4

# the three library layouts both builds declare, copied from families.hip (fal_network_families), nettile.h (net_sort_records)
# and tail.hip (fal_cluster_graph_tiled): `ptrs` receives every handle's pointer in declaration order
LAYOUTS = r"""
#include <stdint.h>
#include <stdlib.h>
#include "scratch.h"

namespace {

struct FakeCtx {
    int calls = 0, slot = -1, fail = 0;
    size_t bytes = 0;
    void* block = nullptr;
    int reserve(int s, size_t b, void** out) {
        ++calls;
        slot = s;
        bytes = b;
        if (fail) return fail;
        *out = block = malloc(b);
        return FAL_OK;
    }
    ~FakeCtx() { free(block); }
};

template <class Ctx>
int families_layout(Ctx* ctx, fal::ScratchLayout& L, int64_t n, int64_t m, void** ptrs) {
    const auto misc = L.array<int32_t>(16);
    const auto rank = L.array<int64_t>(n + 1);
    const auto parent = L.array<int32_t>(n), root = L.array<int32_t>(n), size = L.array<int32_t>(n), flag = L.array<int32_t>(n);
    const auto lo = L.array<uint32_t>(n);
    const auto round = L.array<int32_t>(m);
    const int rc = L.reserve(ctx, 7);
    void* p[] = {misc.get(), rank.get(), parent.get(), root.get(), size.get(), flag.get(), lo.get(), round.get()};
    for (int i = 0; i < 8; ++i) ptrs[i] = p[i];
    return rc;
}

template <class Ctx>
int net_sort_layout(Ctx* ctx, fal::ScratchLayout& L, int64_t m, void** ptrs) {
    const auto keys = L.array<uint64_t>(m), vals = L.array<uint64_t>(m);
    const auto place = L.array<int64_t>(m + 1);
    const auto flag = L.array<int32_t>(m);
    L.pad(56);
    const int rc = L.reserve(ctx, 7);
    void* p[] = {keys.get(), vals.get(), place.get(), flag.get()};
    for (int i = 0; i < 4; ++i) ptrs[i] = p[i];
    return rc;
}

template <class Ctx>
int tiles_layout(Ctx* ctx, fal::ScratchLayout& LT, int nt, void** ptrs) {
    const auto d_tile_row = LT.array<int32_t>(nt + 1);
    const auto cnt = LT.array<int32_t>(4 * (int64_t)nt), base = LT.array<int32_t>(4 * (int64_t)(nt + 1));
    const auto kept = LT.array<int32_t>(nt), fbase = LT.array<int32_t>(nt + 1);
    const auto totals = LT.array<int64_t>(5);
    LT.pad(8);
    const int rc = LT.reserve(ctx, 7);
    void* p[] = {d_tile_row.get(), cnt.get(), base.get(), kept.get(), fbase.get(), totals.get()};
    for (int i = 0; i < 6; ++i) ptrs[i] = p[i];
    return rc;
}

}  // namespace
"""

SHIM = LAYOUTS + r"""
namespace {
// ptrs -> offsets from the block the fake context handed out (-1: the handle gave nullptr)
void report(const FakeCtx& ctx, const fal::ScratchLayout& L, void* const* ptrs, int n, int64_t* off, int64_t* seen) {
    for (int i = 0; i < n; ++i) off[i] = ptrs[i] ? (char*)ptrs[i] - (char*)ctx.block : -1;
    seen[0] = ctx.calls;
    seen[1] = ctx.slot;
    seen[2] = (int64_t)ctx.bytes;
    seen[3] = (int64_t)L.bytes();
}
}  // namespace

extern "C" {

// n statements of (kind, count) in order, reserved in `slot` from a context that fails with `fail` (0: succeeds).
// -> reserve's code; off[i] (a pad's: -2), seen = {calls, slot, bytes asked, bytes()}; before[i] = 1 when handle i gave nullptr
//    BEFORE the reserve
int t_layout(const int32_t* kind, const int64_t* count, int n, int slot, int fail, int64_t* off, int64_t* seen, int32_t* before) {
    FakeCtx ctx;
    ctx.fail = fail;
    fal::ScratchLayout L;
    fal::ScratchLayout::Array<uint8_t> a8[16] = {};
    fal::ScratchLayout::Array<int32_t> a32[16] = {};
    fal::ScratchLayout::Array<int64_t> a64[16] = {};
    fal::ScratchLayout::Array<double> af[16] = {};
    if (n > 16) return -100;
    for (int i = 0; i < n; ++i) {
        if (kind[i] == 0) a8[i] = L.array<uint8_t>(count[i]);
        else if (kind[i] == 1) a32[i] = L.array<int32_t>(count[i]);
        else if (kind[i] == 2) a64[i] = L.array<int64_t>(count[i]);
        else if (kind[i] == 3) af[i] = L.array<double>(count[i]);
        else L.pad(count[i]);
    }
    const auto ptr_of = [&](int i) -> void* {
        return kind[i] == 0 ? (void*)a8[i].get() : kind[i] == 1 ? (void*)a32[i].get() : kind[i] == 2 ? (void*)a64[i].get()
                                                                                                     : (void*)af[i].get();
    };
    for (int i = 0; i < n; ++i) before[i] = kind[i] == 4 || ptr_of(i) == nullptr;
    const int rc = L.reserve(&ctx, slot);
    for (int i = 0; i < n; ++i) {
        void* p = kind[i] == 4 ? nullptr : ptr_of(i);
        off[i] = kind[i] == 4 ? -2 : p ? (char*)p - (char*)ctx.block : -1;
    }
    seen[0] = ctx.calls;
    seen[1] = ctx.slot;
    seen[2] = (int64_t)ctx.bytes;
    seen[3] = (int64_t)L.bytes();
    return rc;
}

int t_families(int64_t n, int64_t m, int64_t* off, int64_t* seen) {
    FakeCtx ctx;
    fal::ScratchLayout L;
    void* p[8];
    const int rc = families_layout(&ctx, L, n, m, p);
    report(ctx, L, p, 8, off, seen);
    return rc;
}

int t_net_sort(int64_t m, int64_t* off, int64_t* seen) {
    FakeCtx ctx;
    fal::ScratchLayout L;
    void* p[4];
    const int rc = net_sort_layout(&ctx, L, m, p);
    report(ctx, L, p, 4, off, seen);
    return rc;
}

int t_tiles(int nt, int64_t* off, int64_t* seen) {
    FakeCtx ctx;
    fal::ScratchLayout L;
    void* p[6];
    const int rc = tiles_layout(&ctx, L, nt, p);
    report(ctx, L, p, 6, off, seen);
    return rc;
}

int t_einternal() { return FAL_EINTERNAL; }
int t_enomem() { return FAL_ENOMEM; }

}  // extern "C"
"""

PROGRAM = LAYOUTS + r"""
#include <stdio.h>

namespace {

// every element of [p, p + count) stored through its own type: past the block is the address sanitizer's, a misaligned
// store the undefined-behaviour sanitizer's
template <class T>
void fill(T* p, int64_t count) {
    for (int64_t i = 0; i < count; ++i) p[i] = (T)i;
}

int small_cases() {
    FakeCtx ctx;
    fal::ScratchLayout L;
    const auto a = L.array<uint8_t>(1);
    const auto b = L.array<int64_t>(1);
    const auto c = L.array<int32_t>(3);
    const auto d = L.array<int64_t>(2);
    const auto e = L.array<double>(2);
    const auto f = L.array<int32_t>(3);
    const auto g = L.array<uint8_t>(5);
    const auto z = L.array<int64_t>(0);
    L.pad(64);
    const auto h = L.array<int32_t>(1);
    if (L.reserve(&ctx, 3) != FAL_OK || ctx.bytes != L.bytes()) return 1;
    fill(a.get(), 1), fill(b.get(), 1), fill(c.get(), 3), fill(d.get(), 2), fill(e.get(), 2), fill(f.get(), 3), fill(g.get(), 5);
    fill(z.get(), 0), fill(h.get(), 1);
    return 0;
}

int families(int64_t n, int64_t m) {
    FakeCtx ctx;
    fal::ScratchLayout L;
    void* p[8];
    if (families_layout(&ctx, L, n, m, p) != FAL_OK || ctx.bytes != L.bytes()) return 1;
    fill((int32_t*)p[0], 16), fill((int64_t*)p[1], n + 1);
    for (int i = 2; i < 6; ++i) fill((int32_t*)p[i], n);
    fill((uint32_t*)p[6], n), fill((int32_t*)p[7], m);
    return 0;
}

int net_sort(int64_t m) {
    FakeCtx ctx;
    fal::ScratchLayout L;
    void* p[4];
    if (net_sort_layout(&ctx, L, m, p) != FAL_OK || ctx.bytes != L.bytes()) return 1;
    fill((uint64_t*)p[0], m), fill((uint64_t*)p[1], m), fill((int64_t*)p[2], m + 1), fill((int32_t*)p[3], m);
    return 0;
}

int tiles(int nt) {
    FakeCtx ctx;
    fal::ScratchLayout L;
    void* p[6];
    if (tiles_layout(&ctx, L, nt, p) != FAL_OK || ctx.bytes != L.bytes()) return 1;
    fill((int32_t*)p[0], nt + 1), fill((int32_t*)p[1], 4 * (int64_t)nt), fill((int32_t*)p[2], 4 * (int64_t)(nt + 1));
    fill((int32_t*)p[3], nt), fill((int32_t*)p[4], nt + 1), fill((int64_t*)p[5], 5);
    return 0;
}

}  // namespace

int main() {
    int failed = small_cases();
    failed += families(3, 5) + families(0, 0) + families(4, 2);
    failed += net_sort(1) + net_sort(2);
    failed += tiles(1) + tiles(2) + tiles(3);
    if (failed == 0) printf("ok: every array written end to end\n");
    return failed != 0;
}
"""


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "scratch_shim", SHIM)
    p = C.c_void_p
    lib.t_layout.argtypes = [p, p, C.c_int, C.c_int, C.c_int, p, p, p]
    lib.t_families.argtypes = [C.c_int64, C.c_int64, p, p]
    lib.t_net_sort.argtypes = [C.c_int64, p, p]
    lib.t_tiles.argtypes = [C.c_int, p, p]
    for f in (lib.t_layout, lib.t_families, lib.t_net_sort, lib.t_tiles, lib.t_einternal, lib.t_enomem):
        f.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def layout(lib, statements, slot=5, fail=0):
    """statements = [(kind, count)] -> (code, offsets (-1 null, -2 pad), {calls, slot, asked, bytes}, null before reserve?)"""
    kind = np.array([k for k, _ in statements], np.int32)
    count = np.array([c for _, c in statements], np.int64)
    off, seen, before = np.zeros(len(kind), np.int64), np.zeros(4, np.int64), np.zeros(len(kind), np.int32)
    rc = lib.t_layout(_p(kind), _p(count), len(kind), slot, fail, _p(off), _p(seen), _p(before))
    return rc, off.tolist(), dict(zip(("calls", "slot", "asked", "bytes"), seen.tolist())), bool(before.all())


def real(fn, n_arrays, *args):
    """one of t_families / t_net_sort / t_tiles -> (code, offsets, {calls, slot, asked, bytes})"""
    off, seen = np.zeros(n_arrays, np.int64), np.zeros(4, np.int64)
    rc = fn(*args, _p(off), _p(seen))
    return rc, off.tolist(), dict(zip(("calls", "slot", "asked", "bytes"), seen.tolist()))


def _compile(tmp_dir, name, source, flags):
    src, exe = os.path.join(str(tmp_dir), name + ".cpp"), os.path.join(str(tmp_dir), name)
    with open(src, "w") as f:
        f.write(source)
    cmd = plain_compiler() + [*flags, "-std=c++17", "-I", CSRC, src, "-o", exe]
    return exe, cmd, subprocess.run(cmd, capture_output=True, text=True)


def sanitizer_missing(tmp_dir):
    """-> why an AddressSanitizer + UBSan build cannot be used here (its runtime does not link, or does not start), or None"""
    exe, cmd, r = _compile(tmp_dir, "asan_probe", "int main() { return 0; }\n", ASAN)
    if r.returncode != 0:
        return "the sanitizer runtime does not link: " + r.stderr.strip()[-200:]
    r = subprocess.run([exe], capture_output=True, text=True)
    if r.returncode != 0:
        return "a sanitizer program does not start: " + r.stderr.strip()[-200:]
    return None


def build_program(tmp_dir, name, flags):
    """compile the stand-alone program into `tmp_dir`/`name` -> path of the executable"""
    exe, cmd, r = _compile(tmp_dir, name, PROGRAM, flags)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-4000:]}"
    return exe
