// What the text writers on the device (mgfwrite.hip, csvwrite.hip) share, the counterpart of textscan.h: the flag bits of a
// sizing call (every unit's bytes -- an MGF entry, a CSV row -- scanned into offsets) and of a write call (a range of units into a
// bounded output), the flush of a wave's LDS tile into the output, and the ends of the two host drivers.
//
// The tile.  A wave formats its text into an LDS tile that stands for the 16-byte aligned stretch of the output around its write
// position: tile[i] is the byte at gbase + i, gbase 16-byte aligned whatever the caller's buffer is.  A flush stores every
// complete 16-byte unit of the text with one 16-byte store per lane; only the bytes in front of the text's first aligned unit and
// behind its last one -- under 16 each, in units shared with the neighbouring text, which other waves write -- go out as single
// bytes.  flush_plan is that arithmetic, pure, for the kernels and the CPU test (tests/test_textwrite_cpu.py).
#pragma once
#include <stdint.h>
#include "numtext.h"         // (the qualifiers for a plain host compiler: flush_plan in the CPU tests' shim)

namespace fal {

enum { TW_BAD_INPUT = 1, TW_TOO_SMALL = 2, TW_OVERFLOW = 4 };      // meta[META_FLAGS] bits of a writer's call

// the flush of tile bytes [lo, hi): [lo, head_end) singly, the 16-byte units [u0, u1) whole, then [rest, hi) singly or carried over
struct FlushPlan {
    int u0, u1, head_end, rest;
};

__host__ __device__ __forceinline__ FlushPlan flush_plan(int lo, int hi) {
    FlushPlan p;
    p.u0 = (lo + 15) >> 4;                                       // the complete 16-byte units [u0, u1)
    p.u1 = hi >> 4;
    p.head_end = (p.u0 << 4) < hi ? (p.u0 << 4) : hi;            // in front of the first aligned unit: < 16 bytes
    p.rest = (p.u1 << 4) > p.head_end ? (p.u1 << 4) : p.head_end;   // behind the last complete unit: < 16 bytes
    return p;
}

}  // namespace fal

#ifdef __HIPCC__
#include <algorithm>
#include "common.h"
#include "ivf.h"
#include "util.h"

namespace fal {

// a wave's tile; [lo, hi) is text not stored yet; `end`: the end of the range the wave may store to (an entry's, a round's)
struct Tile {
    uint8_t* tile;
    uint8_t* gbase;
    uint8_t* end;
    int lo, hi;
    bool overflow;
};

// final: all of [lo, hi) is stored.  Otherwise the complete units go, if there is one, and the rest moves to the tile's front
__device__ __forceinline__ void tile_flush(Tile& t, bool final, int lane) {
    wave_lds_sync();
    const int64_t room = t.end - t.gbase;                                        // bytes of the tile inside the range
    if (t.hi > room) {                                                           // (more text than the sizes said: never stored)
        t.hi = (int)std::max<int64_t>(room, t.lo);
        t.overflow = true;
    }
    const FlushPlan p = flush_plan(t.lo, t.hi);
    if (!final && p.u1 <= p.u0) return;
    if (t.lo + lane < p.head_end) t.gbase[t.lo + lane] = t.tile[t.lo + lane];
    for (int u = p.u0 + lane; u < p.u1; u += 64) *reinterpret_cast<uint4*>(t.gbase + 16 * u) = *reinterpret_cast<const uint4*>(t.tile + 16 * u);
    if (final) {
        if (p.rest + lane < t.hi) t.gbase[p.rest + lane] = t.tile[p.rest + lane];
        t.lo = t.hi;
        return;
    }
    const int rem = t.hi - p.rest;
    const uint8_t v = lane < rem ? t.tile[p.rest + lane] : (uint8_t)0;
    wave_lds_sync();
    if (lane < rem) t.tile[lane] = v;
    t.gbase += p.rest;
    t.lo = 0;
    t.hi = rem;
    wave_lds_sync();
}

// ---- host side: the drivers -----------------------------------------------------------------------------------------------------------
// the meta block of a writer's call, cleared, at the front of its scratch slot
inline int writer_meta(fal_ctx* ctx, int slot, unsigned long long** meta) {
    FAL_TRY(ctx->reserve(slot, 64, (void**)meta));
    FAL_CHECK_HIP(hipMemsetAsync(*meta, 0, 64, ctx->stream));
    return FAL_OK;
}

// the end of a sizing call, behind the launch of its kernel: the scan of the n sizes into n + 1 offsets, the call's one
// synchronisation, the kernel's bad-input flag (`bad_input`: the whole message) and the total
inline int finish_sizes(fal_ctx* ctx, const unsigned long long* meta, const int64_t* sizes, int64_t n, int64_t* offsets, int64_t* total_out,
                        const char* bad_input) {
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i64(ctx, sizes, n, offsets, SLOT_SORT));
    const unsigned long long* h = nullptr;
    FAL_TRY(read_meta(ctx, meta, &h, offsets + n));
    FAL_REQUIRE(!(h[META_FLAGS] & TW_BAD_INPUT), FAL_EINVAL, "%s", bad_input);
    *total_out = (int64_t)h[META_WORDS];
    return FAL_OK;
}

// the end of a write call `who` ("fal_x_write", its sizing call "fal_x_write_sizes"), behind the launch of its kernel: the copy to
// host_out if there is one, the call's one synchronisation and the kernel's three flags; `units` / `a_unit`: "entries" / "an entry"
inline int finish_write(fal_ctx* ctx, const unsigned long long* meta, const char* who, const char* units, const char* a_unit, int64_t first,
                        int64_t last, const uint8_t* out, int64_t out_bytes, uint8_t* host_out) {
    FAL_CHECK_HIP(hipGetLastError());
    if (host_out && out_bytes > 0) FAL_CHECK_HIP(hipMemcpyAsync(host_out, out, (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    const unsigned long long* h = nullptr;
    FAL_TRY(read_meta(ctx, meta, &h));
    FAL_REQUIRE(!(h[META_FLAGS] & TW_TOO_SMALL), FAL_EINVAL, "%s: %lld bytes are too few for %s [%lld, %lld)", who, (long long)out_bytes,
                units, (long long)first, (long long)last);
    FAL_REQUIRE(!(h[META_FLAGS] & TW_BAD_INPUT), FAL_EINVAL,
                "%s: offsets that are no scan of the %s' sizes, or columns that are not those of %s_sizes", who, units, who);
    FAL_REQUIRE(!(h[META_FLAGS] & TW_OVERFLOW), FAL_EINTERNAL, "%s: %s's text is not the size %s_sizes gave", who, a_unit, who);
    return FAL_OK;
}

}  // namespace fal
#endif
