// Peak-file payload decode on the device: the binary arrays of mzML / mzXML spectra (base64 text, optionally zlib) -> the raw
// peak CSR that fal_process_spectra takes (indptr i64, m/z f64, intensity f32, peaks sorted by m/z inside every spectrum).
//
// The host reader keeps the XML structure; every binary array arrives as a range of one contiguous payload buffer plus a
// descriptor row (offset, base64 length, declared value count, flags).  Six launches, no host round trip:
//   arrays  : one thread per array: validate the row, its slot of the inflate buffer (inflated capacity -- declared count x
//             element size, or the longest numpress stream of that count -- plus the float64 values of a numpress array, each
//             8-byte rounded);
//   counts  : one thread per spectrum: its peak count (the declared count of its m/z array); two device scans give the output
//             indptr and the per-array offsets of the inflate buffer;
//   base64  : one wave per array, 4 characters -> 3 bytes per lane; the decoded bytes land at the array's own payload offset in
//             a buffer the size of the payload (decoded <= encoded), so arrays never overlap and stay 8-byte aligned;
//   inflate : one thread per zlib array (RFC 1950/1951: stored, fixed- and dynamic-Huffman blocks, overlapping copies, header and
//             Adler-32 checks).  Canonical-code tables of the thread in LDS (puff-style count / symbol form, 896 B per thread:
//             64 threads = 56 KB per block); output bytes go straight to the array's slot, bounded by its declared capacity;
//   numpress: MS-Numpress arrays (numpress.h) -> float64 in the array's slot, behind its inflated bytes.  Every wave takes 64
//             arrays: linear and pic are sequential per stream, one lane each; slof values are independent, so the wave
//             then walks its slof arrays together, one value per lane;
//   convert : one wave per spectrum: byte swap (mzXML is big-endian), widen / narrow to f64 m/z and f32 intensity (a numpress
//             array is little-endian f64 in the scratch by now), de-interleave
//             the mzXML pairs, stable sort by m/z (what np.lexsort does in falcon._raw_csr: NaN last, ties in input order) --
//             already-sorted spectra (nearly all) are copied, the rest ranked within the wave (peaksort.h, shared with the
//             MGF reader).
// A bad array sets bits of its spectrum's status word (FAL_PEAK_ST_*) and the spectrum's output range is zero-filled; nothing is
// ever written outside an array's slot or a spectrum's range, and every loop is bounded by the input or the declared output.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "inflate.h"
#include "ivf.h"
#include "numpress.h"
#include "peaksort.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kInflateBlock = 64;

__host__ __device__ __forceinline__ int elem_bytes(int64_t flags) { return (flags & FAL_PEAK_F64) ? 8 : 4; }

__host__ __device__ __forceinline__ int64_t array_bytes(const int64_t* d) {      // declared decoded size of an array
    return d[2] * elem_bytes(d[3]) * ((d[3] & FAL_PEAK_PAIRS) ? 2 : 1);
}

__host__ __device__ __forceinline__ int64_t codec_of(int64_t flags) { return flags & FAL_PEAK_NUMPRESS_MASK; }

// bytes a zlib array may inflate to: the declared size, or (its size is not declared) the longest numpress stream of the count
__host__ __device__ __forceinline__ int64_t inflate_cap(const int64_t* d) {
    return codec_of(d[3]) ? numpress_max_bytes(codec_of(d[3]), d[2]) : array_bytes(d);
}

__host__ __device__ __forceinline__ int64_t round8(int64_t v) { return (v + 7) & ~(int64_t)7; }

// a numpress array's float64 values sit behind its inflated bytes
__host__ __device__ __forceinline__ int64_t values_offset(const int64_t* d) { return (d[3] & FAL_PEAK_ZLIB) ? round8(inflate_cap(d)) : 0; }

// ---- launch 1: descriptors ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pd_arrays_kernel(const int64_t* __restrict__ desc, int64_t n_arrays, int64_t payload_bytes,
                                                        int32_t* __restrict__ arr_status, int64_t* __restrict__ cap) {
    for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < n_arrays; a += (int64_t)gridDim.x * blockDim.x) {
        const int64_t* d = desc + 4 * a;
        const int64_t off = d[0], len = d[1], cnt = d[2], flags = d[3];
        const bool ok = off >= 0 && len >= 0 && (off & 7) == 0 && (len & 3) == 0 && off <= payload_bytes &&
                        len <= payload_bytes - off && cnt >= 0 && cnt < (int64_t(1) << 40) &&
                        (flags & ~(int64_t)(FAL_PEAK_F64 | FAL_PEAK_ZLIB | FAL_PEAK_BIG_ENDIAN | FAL_PEAK_PAIRS | FAL_PEAK_NUMPRESS_MASK)) == 0 &&
                        !(codec_of(flags) && (flags & (FAL_PEAK_F64 | FAL_PEAK_BIG_ENDIAN | FAL_PEAK_PAIRS)));
        arr_status[a] = ok ? 0 : FAL_PEAK_ST_DESC;
        cap[a] = ok ? values_offset(d) + (codec_of(flags) ? cnt * 8 : 0) : 0;
    }
}

// ---- launch 2: peaks per spectrum -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pd_counts_kernel(const int64_t* __restrict__ desc, int64_t n_arrays,
                                                        const int64_t* __restrict__ spec, int64_t n_spec, int64_t* __restrict__ count) {
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n_spec; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ma = spec[2 * s];
        const int64_t c = ma >= 0 && ma < n_arrays ? desc[4 * ma + 2] : 0;
        count[s] = c >= 0 && c < (int64_t(1) << 40) ? c : 0;
    }
}

// ---- launch 3: base64 -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int b64_value(uint32_t c) {          // -1: not a base64 character ('=' handled by the caller)
    if (c - 'A' < 26u) return (int)(c - 'A');
    if (c - 'a' < 26u) return (int)(c - 'a') + 26;
    if (c - '0' < 10u) return (int)(c - '0') + 52;
    if (c == '+') return 62;
    if (c == '/') return 63;
    return -1;
}

__global__ __launch_bounds__(256) void pd_base64_kernel(const uint8_t* __restrict__ payload, const int64_t* __restrict__ desc,
                                                        int64_t n_arrays, int32_t* __restrict__ arr_status, uint8_t* __restrict__ dec,
                                                        int64_t* __restrict__ dec_len) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t a = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); a < n_arrays; a += waves) {
        if (arr_status[a]) continue;                                    // wave-uniform
        const int64_t* d = desc + 4 * a;
        const int64_t off = d[0], groups = d[1] >> 2;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(payload + off);
        uint8_t* out = dec + off;
        int pad = 0;
        bool bad = false;
        for (int64_t g = lane; g < groups; g += 64) {
            const uint32_t w = src[g];
            const uint32_t c0 = w & 0xFF, c1 = (w >> 8) & 0xFF, c2 = (w >> 16) & 0xFF, c3 = w >> 24;
            const bool last = g == groups - 1;
            const int p3 = last && c3 == '=', p2 = p3 && c2 == '=';
            const int v0 = b64_value(c0), v1 = b64_value(c1), v2 = p2 ? 0 : b64_value(c2), v3 = p3 ? 0 : b64_value(c3);
            if ((v0 | v1 | v2 | v3) < 0) {
                bad = true;
                continue;
            }
            const uint32_t v = ((uint32_t)v0 << 18) | ((uint32_t)v1 << 12) | ((uint32_t)v2 << 6) | (uint32_t)v3;
            out[3 * g] = (uint8_t)(v >> 16);
            if (!p2) out[3 * g + 1] = (uint8_t)(v >> 8);
            if (!p3) out[3 * g + 2] = (uint8_t)v;
            if (last) pad = p3 + p2;
        }
        const bool any_bad = __ballot(bad) != 0;
        const int total_pad = __shfl(pad, (int)((groups - 1) & 63), 64);
        if (lane == 0) {
            const int64_t n = groups * 3 - (groups ? total_pad : 0);
            dec_len[a] = n;
            int st = any_bad ? FAL_PEAK_ST_BASE64 : 0;
            if (!any_bad && !(d[3] & (FAL_PEAK_ZLIB | FAL_PEAK_NUMPRESS_MASK))) {      // else the stream's decoder counts
                const int64_t want = array_bytes(d);
                st = n > want ? FAL_PEAK_ST_OVERFLOW : n < want ? FAL_PEAK_ST_SHORT : 0;
            }
            arr_status[a] = st;
        }
    }
}

// ---- launch 4: inflate (the inflater itself: inflate.h) -------------------------------------------------------------------
__global__ __launch_bounds__(kInflateBlock) void pd_inflate_kernel(const int64_t* __restrict__ desc, int64_t n_arrays,
                                                                   const uint8_t* __restrict__ dec, int64_t* __restrict__ dec_len,
                                                                   const int64_t* __restrict__ raw_off, int64_t inflate_bytes,
                                                                   uint8_t* __restrict__ raw, int32_t* __restrict__ arr_status) {
    __shared__ HuffLds tables[kInflateBlock];
    HuffLds& h = tables[threadIdx.x];
    for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < n_arrays; a += (int64_t)gridDim.x * blockDim.x) {
        const int64_t* d = desc + 4 * a;
        if (!(d[3] & FAL_PEAK_ZLIB) || arr_status[a]) continue;
        const int64_t cap = inflate_cap(d);
        if (raw_off[a] + cap > inflate_bytes) {
            arr_status[a] = FAL_PEAK_ST_CAPACITY;
            continue;
        }
        int64_t got;                                                    // a numpress stream may be shorter than its bound
        arr_status[a] = inflate_stream_upto(dec + d[0], dec_len[a], raw + raw_off[a], cap, !codec_of(d[3]), &got, h);
        dec_len[a] = got;                                               // the stream the numpress stage reads
    }
}

// ---- launch 5: MS-Numpress (the codecs themselves: numpress.h) ----------------------------------------------------------------
struct NumpressJob {
    const uint8_t* in;               // the stream: the array's inflated bytes, or its base64-decoded ones
    int64_t len, count;
    double* out;                     // count float64 values of the array's slot
};

// the array's stream and output; false (with *st set) when the slot ends behind the scratch
__device__ __forceinline__ bool numpress_job(const int64_t* d, int64_t a, const uint8_t* dec, const int64_t* dec_len,
                                             const int64_t* raw_off, int64_t inflate_bytes, uint8_t* raw, NumpressJob* j, int* st) {
    const int64_t voff = raw_off[a] + values_offset(d);
    if (voff + d[2] * 8 > inflate_bytes) {
        *st = FAL_PEAK_ST_CAPACITY;
        return false;
    }
    j->in = (d[3] & FAL_PEAK_ZLIB) ? raw + raw_off[a] : dec + d[0];
    j->len = dec_len[a];
    j->count = d[2];
    j->out = reinterpret_cast<double*>(raw + voff);
    return true;
}

__global__ __launch_bounds__(256) void numpress_decode_kernel(const int64_t* __restrict__ desc, int64_t n_arrays,
                                                              const uint8_t* __restrict__ dec, const int64_t* __restrict__ dec_len,
                                                              const int64_t* __restrict__ raw_off, int64_t inflate_bytes,
                                                              uint8_t* raw, int32_t* __restrict__ arr_status) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t g = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); g * 64 < n_arrays; g += waves) {
        const int64_t a = g * 64 + lane;
        const int64_t codec = a < n_arrays && !arr_status[a] ? codec_of(desc[4 * a + 3]) : 0;
        if (codec == FAL_PEAK_NUMPRESS_LINEAR || codec == FAL_PEAK_NUMPRESS_PIC) {      // sequential streams: a lane each
            NumpressJob j;
            int st = 0;
            if (numpress_job(desc + 4 * a, a, dec, dec_len, raw_off, inflate_bytes, raw, &j, &st)) {
                int64_t n;
                st = codec == FAL_PEAK_NUMPRESS_PIC ? numpress_pic(j.in, j.len, j.out, j.count, &n)
                                                    : numpress_linear(j.in, j.len, j.out, j.count, &n);
                if (!st && n < j.count) st = FAL_PEAK_ST_SHORT;
            }
            arr_status[a] = st;
        }
        unsigned long long todo = __ballot(codec == FAL_PEAK_NUMPRESS_SLOF);            // independent values: the wave per array
        while (todo) {
            const int64_t b = g * 64 + (__ffsll(todo) - 1);
            todo &= todo - 1;
            NumpressJob j;
            int st = 0;
            if (numpress_job(desc + 4 * b, b, dec, dec_len, raw_off, inflate_bytes, raw, &j, &st)) {
                double fp;
                int64_t n;
                st = numpress_slof_header(j.in, j.len, &fp, &n);
                if (!st) {
                    for (int64_t i = lane; i < std::min(n, j.count); i += 64) j.out[i] = numpress_slof_value(j.in, fp, i);
                    st = n > j.count ? FAL_PEAK_ST_OVERFLOW : n < j.count ? FAL_PEAK_ST_SHORT : 0;
                }
            }
            if (lane == 0) arr_status[b] = st;
        }
    }
}

// ---- launch 6: convert + sort ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double load_value(const uint8_t* base, int64_t i, bool f64, bool be) {
    if (f64) {
        uint64_t u = reinterpret_cast<const uint64_t*>(base)[i];
        if (be) u = __builtin_bswap64(u);
        return __builtin_bit_cast(double, u);
    }
    uint32_t u = reinterpret_cast<const uint32_t*>(base)[i];
    if (be) u = __builtin_bswap32(u);
    return (double)__builtin_bit_cast(float, u);
}

struct ArrayView {
    const uint8_t* base;
    bool f64, be;
    int stride, shift;               // element index = stride * peak + shift (mzXML pairs: 2p, 2p + 1)
    __device__ __forceinline__ double at(int64_t p) const { return load_value(base, stride * p + shift, f64, be); }
    // intensity: float32 data as stored, float64 data rounded to nearest (numpy's astype(float32))
    __device__ __forceinline__ float at_f32(int64_t p) const {
        if (f64) return (float)load_value(base, stride * p + shift, true, be);
        uint32_t u = reinterpret_cast<const uint32_t*>(base)[stride * p + shift];
        if (be) u = __builtin_bswap32(u);
        return __builtin_bit_cast(float, u);
    }
};

__global__ __launch_bounds__(256) void pd_convert_kernel(const int64_t* __restrict__ desc, int64_t n_arrays,
                                                         const int64_t* __restrict__ spec, int64_t n_spec,
                                                         const int32_t* __restrict__ arr_status, const uint8_t* __restrict__ dec,
                                                         const uint8_t* __restrict__ raw, const int64_t* __restrict__ raw_off,
                                                         const int64_t* __restrict__ indptr, int64_t nnz_cap,
                                                         double* __restrict__ out_mz, float* __restrict__ out_it,
                                                         int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < n_spec; s += waves) {
        const int64_t ma = spec[2 * s], ia = spec[2 * s + 1];
        const int64_t b = indptr[s], e = indptr[s + 1], n = e - b;
        int st = 0;
        if (ma < 0 || ma >= n_arrays || ia < 0 || ia >= n_arrays) {
            st = FAL_PEAK_ST_DESC;
        } else {
            const int64_t fm = desc[4 * ma + 3], fi = desc[4 * ia + 3];
            const bool pairs = (fm & FAL_PEAK_PAIRS) != 0;
            if (pairs != ((fi & FAL_PEAK_PAIRS) != 0) || (pairs && ma != ia) || desc[4 * ia + 2] != n) st = FAL_PEAK_ST_DESC;
            st |= arr_status[ma] | arr_status[ia];
        }
        if (e > nnz_cap) st |= FAL_PEAK_ST_CAPACITY;
        if (st) {
            for (int64_t j = b + lane; j < std::min(e, nnz_cap); j += 64) {
                out_mz[j] = 0.0;
                out_it[j] = 0.0f;
            }
            if (lane == 0) status[s] = st;
            continue;
        }
        auto view = [&](int64_t a, int shift) {
            const int64_t* d = desc + 4 * a;
            ArrayView v;
            v.base = codec_of(d[3]) ? raw + raw_off[a] + values_offset(d) : (d[3] & FAL_PEAK_ZLIB) ? raw + raw_off[a] : dec + d[0];
            v.f64 = (d[3] & FAL_PEAK_F64) != 0 || codec_of(d[3]);
            v.be = (d[3] & FAL_PEAK_BIG_ENDIAN) != 0;
            v.stride = (d[3] & FAL_PEAK_PAIRS) ? 2 : 1;
            v.shift = (d[3] & FAL_PEAK_PAIRS) ? shift : 0;
            return v;
        };
        const ArrayView vm = view(ma, 0), vi = view(ia, 1);
        wave_sort_peaks(n, lane, [&](int64_t j) { return vm.at(j); }, [&](int64_t j) { return vi.at_f32(j); }, out_mz + b, out_it + b);
        if (lane == 0) status[s] = 0;
    }
}

FAL_WARM_KERNEL(pd_convert_kernel);

}  // namespace
}  // namespace fal

using namespace fal;

extern "C" int fal_decode_peaks(fal_ctx* ctx, const uint8_t* payload, int64_t payload_bytes, const int64_t* arrays, int64_t n_arrays,
                                const int64_t* spectra, int64_t n_spectra, int64_t inflate_bytes, int64_t nnz_cap,
                                int64_t* out_indptr, double* out_mz, float* out_intensity, int32_t* status_out) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && payload_bytes >= 0 && n_arrays >= 0 && n_spectra >= 0 && inflate_bytes >= 0 && nnz_cap >= 0, FAL_EINVAL,
                "fal_decode_peaks: bad argument");
    FAL_REQUIRE(out_indptr, FAL_EINVAL, "fal_decode_peaks: NULL out_indptr");
    if (n_spectra == 0) {
        FAL_CHECK_HIP(hipMemsetAsync(out_indptr, 0, sizeof(int64_t), ctx->stream));
        return FAL_OK;
    }
    FAL_REQUIRE(spectra && status_out && (n_arrays == 0 || arrays), FAL_EINVAL, "fal_decode_peaks: NULL table");
    FAL_REQUIRE(payload_bytes == 0 || payload, FAL_EINVAL, "fal_decode_peaks: NULL payload");
    FAL_REQUIRE(nnz_cap == 0 || (out_mz && out_intensity), FAL_EINVAL, "fal_decode_peaks: NULL peaks");
    const int64_t na = std::max<int64_t>(n_arrays, 1);
    int32_t* arr_status = nullptr;
    int64_t *cap = nullptr, *raw_off = nullptr, *count = nullptr, *dec_len = nullptr;
    uint8_t *dec = nullptr, *raw = nullptr;
    FAL_TRY(ctx->reserve(SLOT_MISC, sizeof(int32_t) * (size_t)na, (void**)&arr_status));
    FAL_TRY(ctx->reserve(SLOT_MISC2, sizeof(int64_t) * (size_t)na, (void**)&cap));
    FAL_TRY(ctx->reserve(SLOT_SORT2, sizeof(int64_t) * (size_t)(na + 1), (void**)&raw_off));
    FAL_TRY(ctx->reserve(SLOT_TAIL, sizeof(int64_t) * (size_t)n_spectra, (void**)&count));
    FAL_TRY(ctx->reserve(SLOT_TAIL2, sizeof(int64_t) * (size_t)na, (void**)&dec_len));
    FAL_TRY(ctx->reserve(SLOT_TAIL3, (size_t)payload_bytes + 64, (void**)&dec));
    FAL_TRY(ctx->reserve(SLOT_TAIL4, (size_t)inflate_bytes + 64, (void**)&raw));
    const auto grid_for = [&](int64_t items, int per_block) {
        return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, per_block), (int64_t)ctx->num_cus * 16));
    };
    if (n_arrays > 0) {
        hipLaunchKernelGGL(pd_arrays_kernel, dim3(grid_for(n_arrays, 256)), dim3(256), 0, ctx->stream, arrays, n_arrays, payload_bytes,
                           arr_status, cap);
        FAL_CHECK_HIP(hipGetLastError());
    }
    FAL_TRY(device_scan_i64(ctx, cap, n_arrays, raw_off, SLOT_SORT));
    hipLaunchKernelGGL(pd_counts_kernel, dim3(grid_for(n_spectra, 256)), dim3(256), 0, ctx->stream, arrays, n_arrays, spectra,
                       n_spectra, count);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i64(ctx, count, n_spectra, out_indptr, SLOT_DB));
    if (n_arrays > 0) {
        hipLaunchKernelGGL(pd_base64_kernel, dim3(grid_for(n_arrays, 4)), dim3(256), 0, ctx->stream, payload, arrays, n_arrays,
                           arr_status, dec, dec_len);
        FAL_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(pd_inflate_kernel, dim3(grid_for(n_arrays, kInflateBlock)), dim3(kInflateBlock), 0, ctx->stream, arrays,
                           n_arrays, dec, dec_len, raw_off, inflate_bytes, raw, arr_status);
        FAL_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(numpress_decode_kernel, dim3(grid_for(n_arrays, 256)), dim3(256), 0, ctx->stream, arrays, n_arrays, dec,
                           dec_len, raw_off, inflate_bytes, raw, arr_status);
        FAL_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(pd_convert_kernel, dim3(grid_for(n_spectra, 4)), dim3(256), 0, ctx->stream, arrays, n_arrays, spectra, n_spectra,
                       arr_status, dec, raw, raw_off, out_indptr, nnz_cap, out_mz, out_intensity, status_out);
    FAL_CHECK_HIP(hipGetLastError());
    return FAL_OK;
}
