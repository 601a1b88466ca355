// Header values by a caller's key table, for the line readers on the device: what fal_mgf_headers (mgfparse.hip) and
// fal_msp_headers (mspparse.hip) share -- the table's validation on the host and the kernel body, one wave per entry.  The two
// differ in the separator between key and value ('=' / ':'), in the lines of an entry that are scanned and in the keys that are
// reserved; the per-line functions are mgfkeys.h's.
#pragma once
#include <algorithm>
#include "common.h"
#include "mgfkeys.h"
#include "textscan.h"

namespace fal {

constexpr int kKeyWaveStage = 4096;              // LDS tile of a wave's 64 lines

static_assert(kMgfMaxKeys == FAL_MGF_MAX_KEYS && kMgfMaxKeyBytes == FAL_MGF_MAX_KEY_BYTES && MGF_VAL_SPAN == FAL_MGF_KEY_SPAN &&
                  MGF_VAL_INT == FAL_MGF_KEY_INT && MGF_STATE_ABSENT == FAL_MGF_KEY_ABSENT && MGF_STATE_PRESENT == FAL_MGF_KEY_PRESENT &&
                  MGF_STATE_HOST == FAL_MGF_KEY_HOST && kMgfMaxKeys <= 64,
              "mgfkeys.h and include/falcon_hip.h name the same table limits, kinds and states");

// The kernel body.  A line per lane gives the index of its key in the table (-1: none, or no header line); one ballot of "any
// table key" gates the ballots per key, whose highest lane -- the entry's last such line so far -- wins.  Lane k carries key
// k's result across the turns, so no per-key array is indexed by a loop counter.
//   range(s, &first, &last) : the lines [first, last) of entry s that are scanned
//   is_header(c)            : is a line of class c (the reader's cls byte) a header line?  Its bit 8 is the reader's LONG bit.
template <char Sep, class Range, class IsHeader>
__device__ __forceinline__ void headers_pass(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ start,
                                             const uint8_t* __restrict__ cls, int64_t n_spec, const MgfKeyTable& table,
                                             int64_t* __restrict__ span_out, int64_t* __restrict__ value_out,
                                             int32_t* __restrict__ state_out, const Range& range, const IsHeader& is_header) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4][kKeyWaveStage + 16];
    __shared__ MgfKeyTable keys;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&table);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&keys);
        for (int i = threadIdx.x; i < (int)(sizeof(MgfKeyTable) / 4); i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const int n_keys = keys.n;
    const int lane = threadIdx.x & 63;
    uint8_t* tile = tiles[threadIdx.x >> 6];
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_spec; s += waves) {
        int64_t first, last;
        range(s, &first, &last);
        int my_state = MGF_STATE_ABSENT;                                       // lane k: key k
        int64_t my_lo = 0, my_hi = 0, my_val = 0;
        for (int64_t g = first; g < last; g += 64) {
            const int64_t g1 = std::min<int64_t>(g + 64, last);
            const int64_t b0 = start[g], b1 = std::min<int64_t>(start[g1], n), a0 = b0 & ~(int64_t)15;
            const bool staged = b1 - a0 <= kKeyWaveStage;                      // wave-uniform
            if (staged) stage_bytes(text, n, b0, b1, tile, lane, 64);
            wave_lds_sync();
            const int64_t line = g + lane;
            int idx = -1, st = MGF_STATE_PRESENT;
            int64_t v_lo = 0, v_hi = 0, ival = 0;
            if (line < g1) {
                const int c = cls[line];
                if (is_header(c)) {
                    const int64_t ls = start[line];
                    const int len = (int)(start[line + 1] - 1 - ls);
                    const uint8_t* p = staged ? tile + (ls - a0) : text + ls;
                    int lo = 0, hi = len, klo, khi, a, z;
                    mgf_strip(p, &lo, &hi);
                    mgf_split_at<Sep>(p, lo, hi, &klo, &khi, &a, &z);
                    idx = mgf_table_key(p + klo, khi - klo, keys.bytes, keys.len, n_keys);
                    if (idx >= 0) {
                        v_lo = ls + a;
                        v_hi = ls + z;
                        if (c & MGF_LONG) st = MGF_STATE_HOST;
                        else if (keys.kind[idx] == MGF_VAL_INT && z > a && !mgf_parse_int(p + a, z - a, &ival)) st = MGF_STATE_HOST;
                    }
                }
            }
            if (__ballot(idx >= 0) == 0) continue;                             // no table key among these lines
            for (int k = 0; k < n_keys; ++k) {
                const uint64_t m = __ballot(idx == k);
                if (m == 0) continue;
                const int src = 63 - __builtin_clzll(m);
                const int st_k = __shfl(st, src, 64);
                const int64_t lo_k = __shfl(v_lo, src, 64), hi_k = __shfl(v_hi, src, 64), val_k = __shfl(ival, src, 64);
                if (lane == k) {
                    my_state = st_k;
                    my_lo = lo_k;
                    my_hi = hi_k;
                    my_val = st_k == MGF_STATE_PRESENT ? val_k : 0;
                }
            }
        }
        if (lane < n_keys) {
            const int64_t at = s * n_keys + lane;                              // < n_spec * n_keys
            span_out[2 * at] = my_lo;
            span_out[2 * at + 1] = my_hi;
            value_out[at] = my_val;
            state_out[at] = my_state;
        }
    }
}

// The caller's table (keys back to back, key_ptr, key_kind) -> the kernel's form, checked: 1 to kMgfMaxKeys keys of 1 to
// kMgfMaxKeyBytes bytes of stripped lower-case printable ASCII without `sep`, every key once; `mgf_own`: none of fal_mgf_parse's
// own keys.  `who` is the entry point's name in the messages.
inline int key_table_from(const char* who, char sep, bool mgf_own, const uint8_t* keys, const int64_t* key_ptr, const int32_t* key_kind,
                          int n_keys, MgfKeyTable* out) {
    FAL_REQUIRE(n_keys >= 1 && n_keys <= kMgfMaxKeys, FAL_EINVAL, "%s: %d keys, 1 to %d are taken", who, n_keys, kMgfMaxKeys);
    MgfKeyTable& table = *out;
    table = MgfKeyTable{};
    table.n = n_keys;
    for (int k = 0; k < n_keys; ++k) {
        const int64_t a = key_ptr[k], len = key_ptr[k + 1] - a;
        FAL_REQUIRE(a >= 0 && len >= 1 && len <= kMgfMaxKeyBytes, FAL_EINVAL, "%s: key %d has %lld bytes, 1 to %d are taken", who, k,
                    (long long)len, kMgfMaxKeyBytes);
        FAL_REQUIRE(key_kind[k] == FAL_MGF_KEY_SPAN || key_kind[k] == FAL_MGF_KEY_INT, FAL_EINVAL, "%s: key %d: unknown kind %d", who, k,
                    key_kind[k]);
        const uint8_t* w = keys + a;
        bool plain = !mgf_space(w[0]) && !mgf_space(w[len - 1]);
        for (int64_t i = 0; i < len; ++i) plain = plain && w[i] >= 0x20 && w[i] <= 0x7E && w[i] != (uint8_t)sep && !(w[i] - 'A' < 26u);
        FAL_REQUIRE(plain, FAL_EINVAL, "%s: key %d is no stripped lower-case ASCII key", who, k);
        int vlo, vhi;
        FAL_REQUIRE(!mgf_own || mgf_header(w, 0, (int)len, &vlo, &vhi) == MGF_KEY_OTHER, FAL_EINVAL,
                    "%s: key %d is one of fal_mgf_parse's own (title, pepmass, charge, rtinseconds)", who, k);
        FAL_REQUIRE(mgf_table_key(w, (int)len, table.bytes, table.len, k) < 0, FAL_EINVAL, "%s: key %d repeats an earlier key", who, k);
        for (int64_t i = 0; i < len; ++i) table.bytes[k][i] = w[i];
        table.len[k] = (int32_t)len;
        table.kind[k] = key_kind[k];
    }
    return FAL_OK;
}

}  // namespace fal
