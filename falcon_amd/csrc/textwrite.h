// What the text writers on the device (mgfwrite.hip, csvwrite.hip, recwrite.hip) share, the counterpart of textscan.h: the flag
// bits of a sizing call (every unit's bytes -- an MGF entry, a CSV row, a record -- scanned into offsets) and of a write call (a
// range of units into a bounded output), a wave's LDS tile with its flush into the output and the pieces a wave appends to it, the
// two kernel bodies of a writer with a lane per unit (sizes_by_lane, write_units_by_lane), and the ends of the two host drivers.
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

// ---- a wave per unit: the wave appends piece after piece to its tile, the complete 16-byte units flushed behind every piece -------
// what such a flush may leave in the tile (under 16 bytes behind the last complete unit; or under 16 in front of the first one and
// an incomplete one): a tile takes any piece of up to its size - kTileCarry bytes
constexpr int kTileCarry = 31;

// an empty tile for the range [begin, end) of the output
__device__ __forceinline__ Tile tile_open(uint8_t* tile, uint8_t* begin, uint8_t* end) {
    const int mis = (int)(reinterpret_cast<uintptr_t>(begin) & 15);
    return Tile{tile, begin - mis, end, mis, mis, false};
}

// a piece of m bytes that lane 0 writes: write(dst)
template <class F>
__device__ __forceinline__ void tile_append_by_lane0(Tile& t, int m, int lane, F write) {
    if (lane == 0) write(t.tile + t.hi);
    t.hi += m;
    tile_flush(t, false, lane);
}

// m bytes of src, copied lane-strided in pieces of at most kPiece bytes (m: the same in every lane).  N, the caller's own length
// type, is there for the register allocation alone: a 32-bit length is not widened across the flushes (profiles/NOTES.md)
template <int kPiece, class N>
__device__ __forceinline__ void tile_append_bytes(Tile& t, const uint8_t* src, N m, int lane) {
    for (N c = 0; c < m; c += kPiece) {
        const int n = (int)std::min<N>(kPiece, m - c);
        for (int i = lane; i < n; i += 64) t.tile[t.hi + i] = src[c + i];
        t.hi += n;
        tile_flush(t, false, lane);
    }
}

// a piece per lane, placed at a wave prefix sum of their lengths: a lane with len > 0 bytes writes them, write(dst)
template <class F>
__device__ __forceinline__ void tile_append_by_lanes(Tile& t, int len, int lane, F write) {
    const int incl = wave_prefix_sum(len);
    if (len > 0) write(t.tile + t.hi + incl - len);
    t.hi += __shfl(incl, 63, 64);
    tile_flush(t, false, lane);
}

// the last flush; TW_OVERFLOW unless the text ends where the range does; the tile is free for the wave's next unit
__device__ __forceinline__ void tile_close(Tile& t, int lane, unsigned long long* meta) {
    tile_flush(t, true, lane);
    const bool shortfall = t.gbase + t.hi != t.end;                              // (less text than the sizes said)
    if (lane == 0 && (t.overflow || shortfall)) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_OVERFLOW);
    wave_lds_sync();
}

// ---- a lane per unit ----------------------------------------------------------------------------------------------------------------
// W is the writer's view of its units: W::Unit, what a lane keeps of a unit between measuring and formatting it;
// load(k, &bad) -> Unit (*bad: unit k or one of its ranges lies outside its arrays); len(unit); write(dst, unit, k) -> the bytes
// written.  A unit that no tile takes is written by lane 0 alone, straight into its own range, unless W::kLongByWave: then the
// whole wave calls long_unit(tile, dst, len, k, meta), which flags TW_OVERFLOW itself.

// sizes[k] = the bytes of unit k (0 and TW_BAD_INPUT for a bad one): the body of a sizes kernel
template <class W>
__device__ __forceinline__ void sizes_by_lane(const W& w, int64_t n, int64_t* __restrict__ sizes, unsigned long long* __restrict__ meta) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    bool any_bad = false;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += step) {
        bool bad = false;
        const typename W::Unit u = w.load(k, &bad);
        sizes[k] = bad ? 0 : w.len(u);
        any_bad |= bad;
    }
    if (any_bad) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
}

// The body of a write kernel: units [first, last) into out, a wave per 64 consecutive units, `tile`: the wave's kTile bytes of LDS.
// A round measures the next 64 units, places as many leading ones as the tile takes at a wave prefix sum of their lengths, the
// lanes format them there and the tile -- a Tile around the round's first byte -- is flushed whole.  Every unit's length is checked
// against offsets[k + 1] - offsets[k] and every round's range against [0, offsets[last] - offsets[first]] <= out_bytes before
// anything of it is stored.
template <int kTile, class W>
__device__ __forceinline__ void write_units_by_lane(const W& w, uint8_t* tile, const int64_t* __restrict__ offsets, int64_t first, int64_t last,
                                                    uint8_t* __restrict__ out, int64_t out_bytes, unsigned long long* __restrict__ meta) {
    static_assert(kTile % 16 == 0, "a tile is whole 16-byte units");
    const int lane = threadIdx.x & 63;
    const int64_t base = offsets[first], need = offsets[last] - base;
    if (need < 0 || need > out_bytes) {                                          // uniform over the grid: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_TOO_SMALL);
        return;
    }
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6), n_tiles = (last - first + 63) / 64;
    for (int64_t t = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); t < n_tiles; t += waves) {
        const int64_t k1 = std::min<int64_t>(first + 64 * (t + 1), last);
        int64_t r = first + 64 * t;
        while (r < k1) {                                                         // (r, k1: the same in every lane)
            const int64_t k = r + lane;
            const bool on = k < k1;
            bool bad = false;
            typename W::Unit unit = {};
            int64_t len = 0;
            if (on) {
                unit = w.load(k, &bad);
                len = w.len(unit);
                bad |= len != offsets[k + 1] - offsets[k];
            }
            const int64_t g0 = offsets[r] - base;
            const int mis = (int)((reinterpret_cast<uintptr_t>(out) + (uintptr_t)g0) & 15);   // (no pointer is formed before g0 is checked)
            const int cap = kTile - mis;
            const int clen = (int)std::min<int64_t>(len, kTile + 1);            // (64 of them stay far below 2^31)
            const int incl = wave_prefix_sum(clen);
            const int cnt = __popcll(__ballot(on && incl <= cap));              // the leading units the tile takes (incl ascends)
            const int64_t total = cnt ? __shfl(incl, cnt - 1, 64) : __shfl((long long)len, 0, 64);   // (no unit fits: unit r alone)
            if (__ballot(bad) != 0ull || g0 < 0 || g0 > need || total > need - g0) {   // columns or offsets that are not the sizing pass's
                if (lane == 0) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_BAD_INPUT);
                break;
            }
            if (cnt == 0) {
                if constexpr (W::kLongByWave) w.long_unit(tile, out + g0, total, r, meta);
                else if (lane == 0 && w.write(out + g0, unit, r) != total) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_OVERFLOW);
                r += 1;
                continue;
            }
            if (lane < cnt && w.write(tile + mis + incl - clen, unit, k) != len) atomicOr(&meta[META_FLAGS], (unsigned long long)TW_OVERFLOW);
            Tile text{tile, out + g0 - mis, out + g0 + total, mis, mis + (int)total, false};   // [mis, mis + total): this round's text
            tile_flush(text, true, lane);
            wave_lds_sync();                                                     // (the next round writes the tile again)
            r += cnt;
        }
    }
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
