// Byte-streaming helpers shared by the text readers on the device (mgfparse.hip, mzmlscan.hip): 16-byte loads that stop at the
// end of the text, a block-wide prefix sum and the copy of a byte range into an LDS tile.
#pragma once
#include "common.h"

namespace fal {

// 16 text bytes at pos (a multiple of 16) as four words; bytes at or behind n read as 0
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ text, int64_t n, int64_t pos) {
    if (pos + 16 <= n) return *reinterpret_cast<const uint4*>(text + pos);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (pos + j < n) w[j >> 2] |= (uint32_t)text[pos + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t byte_of(const uint4& v, int j) {
    const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 0xFF;
}

// exclusive prefix of v over the 256 threads of a block, *total: the block's sum
__device__ __forceinline__ int block_prefix(int v, int* total) {
    __shared__ int ws[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_prefix_sum(v);
    __syncthreads();                             // (the previous use of ws is over)
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
    for (int w = 0; w < 4; ++w) {
        before += w < wave ? ws[w] : 0;
        sum += ws[w];
    }
    *total = sum;
    return before + incl - v;
}

// bytes [b0, b1) of the text into an LDS tile whose byte 0 is text byte (b0 & ~15); `step` lanes x 16 bytes per round
__device__ __forceinline__ void stage_bytes(const uint8_t* __restrict__ text, int64_t n, int64_t b0, int64_t b1, uint8_t* tile, int lane,
                                            int step) {
    const int64_t a0 = b0 & ~(int64_t)15;
    for (int64_t off = lane * 16; a0 + off < b1; off += step * 16) *reinterpret_cast<uint4*>(tile + off) = load16(text, n, a0 + off);
}

}  // namespace fal
