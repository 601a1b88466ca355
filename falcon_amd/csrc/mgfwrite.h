// MGF text out of the device: the entry layout of the writer, on numtext.h's digits and number text.  Shared by mgfwrite.hip's
// kernels and the host build of the CPU tests (tests/hostbuild_mgfwrite.py); they mirror falcon_amd/ms_io/mgf_io.write_spectra,
// which stays the writer of record: for the same entries the bytes are the same.
//
// Numbers.  A float32 x becomes the bytes of Python's repr(float(x)): num_shortest_widened's digits in repr's layout.
//   layout : decpt = position of the decimal point in front of the digits' first; -4 < decpt <= 16 positional ("0.000ddd", "dd.dd",
//            "dd00.0"), otherwise d[.ddd]e[+-]XX with at least two exponent digits; "-0.0", "nan" (any NaN), "inf", "-inf".
//   length : at most 17 digits; sign + "0.000" + 17 digits = sign + 17 digits + '.' + "e-XX" = 23 bytes = kMgfNumMax.
//
// Entries.  BEGIN IONS / TITLE= / PEPMASS= / CHARGE= (charge != 0) / RTINSECONDS= / CLUSTER= / "<mz> <intensity>" per peak /
// END IONS and an empty line, every line closed by '\n'.  The pieces below are what one lane of the writer formats: the four
// fields behind the title (mgf_field_*) and a peak line (mgf_peak_*); mgf_entry_len / mgf_write_entry put them together serially.
#pragma once
#include <stdint.h>
#include "numtext.h"

namespace fal {

constexpr int kMgfNumMax = 23;                       // bytes of one number, at most
constexpr int kMgfPeakMax = 2 * kMgfNumMax + 2;      // "<mz> <intensity>\n"
constexpr int kMgfHeadLen = 17;                      // "BEGIN IONS\nTITLE="
constexpr int kMgfTailLen = 10;                      // "END IONS\n\n"
constexpr int kMgfFields = 4;                        // "\nPEPMASS=..\n", "CHARGE=..\n" or nothing, "RTINSECONDS=..\n", "CLUSTER=..\n"
constexpr int kMgfFieldMax = 12 + kMgfNumMax + 1;    // the longest of them (RTINSECONDS)
// numtext.h's tables under the names this writer's CPU tests (tests/hostbuild_mgfwrite.py) read them by
constexpr int kMgfPow5InvCount = kNumPow5InvCount, kMgfPow5Count = kNumPow5Count;
constexpr const uint64_t (&kMgfPow5Inv)[22][2] = kNumPow5Inv, (&kMgfPow5)[64][2] = kNumPow5;

__host__ __device__ __forceinline__ bool mgf_positional(int decpt) { return decpt > -4 && decpt <= 16; }

// bytes of repr(float(x))
__host__ __device__ __forceinline__ int mgf_num_len(float x) {
    const uint32_t bits = num_float_bits(x);
    const int neg = (int)(bits >> 31);
    if ((bits & 0x7F800000u) == 0x7F800000u) return (bits & 0x7FFFFFu) ? 3 : 3 + neg;
    if ((bits & 0x7FFFFFFFu) == 0) return 3 + neg;
    const NumDecimal d = num_shortest_widened(bits);
    return neg + num_decimal_len(d, mgf_positional(d.decpt));
}

// repr(float(x)) at dst (room for kMgfNumMax bytes) -> its length
__host__ __device__ __forceinline__ int mgf_write_num(uint8_t* dst, float x) {
    const uint32_t bits = num_float_bits(x);
    int at = 0;
    if ((bits & 0x7F800000u) == 0x7F800000u && (bits & 0x7FFFFFu)) {
        dst[0] = 'n';
        dst[1] = 'a';
        dst[2] = 'n';
        return 3;
    }
    if (bits >> 31) dst[at++] = '-';
    if ((bits & 0x7F800000u) == 0x7F800000u) {
        dst[at] = 'i';
        dst[at + 1] = 'n';
        dst[at + 2] = 'f';
        return at + 3;
    }
    if ((bits & 0x7FFFFFFFu) == 0) {
        dst[at] = '0';
        dst[at + 1] = '.';
        dst[at + 2] = '0';
        return at + 3;
    }
    const NumDecimal d = num_shortest_widened(bits);
    return at + num_write_decimal(dst + at, d, mgf_positional(d.decpt));
}

// the four fields behind the title's bytes; `which` 0: "\nPEPMASS=<pm>\n" (it closes the title line), 1: "CHARGE=<|z|><+ or ->\n"
// when charge != 0, 2: "RTINSECONDS=<rt>\n", 3: "CLUSTER=<id>\n"
__host__ __device__ __forceinline__ int mgf_field_len(int which, float pm, int32_t charge, float rt, int64_t cluster) {
    switch (which) {
        case 0: return 9 + mgf_num_len(pm) + 1;
        case 1: return charge == 0 ? 0 : 7 + num_int_len((int64_t)num_abs64(charge)) + 2;
        case 2: return 12 + mgf_num_len(rt) + 1;
        default: return 8 + num_int_len(cluster) + 1;
    }
}

// (room for kMgfFieldMax bytes)
__host__ __device__ __forceinline__ int mgf_write_field(uint8_t* dst, int which, float pm, int32_t charge, float rt, int64_t cluster) {
    int at;
    if (which == 0) {
        at = num_put(dst, "\nPEPMASS=", 9);
        at += mgf_write_num(dst + at, pm);
    } else if (which == 1) {
        if (charge == 0) return 0;
        at = num_put(dst, "CHARGE=", 7);
        at += num_write_int(dst + at, (int64_t)num_abs64(charge));
        dst[at++] = charge < 0 ? '-' : '+';
    } else if (which == 2) {
        at = num_put(dst, "RTINSECONDS=", 12);
        at += mgf_write_num(dst + at, rt);
    } else {
        at = num_put(dst, "CLUSTER=", 8);
        at += num_write_int(dst + at, cluster);
    }
    dst[at++] = '\n';
    return at;
}

__host__ __device__ __forceinline__ int mgf_peak_len(float mz, float intensity) { return mgf_num_len(mz) + mgf_num_len(intensity) + 2; }

// "<mz> <intensity>\n" (room for kMgfPeakMax bytes)
__host__ __device__ __forceinline__ int mgf_write_peak(uint8_t* dst, float mz, float intensity) {
    int at = mgf_write_num(dst, mz);
    dst[at++] = ' ';
    at += mgf_write_num(dst + at, intensity);
    dst[at++] = '\n';
    return at;
}

__host__ __device__ __forceinline__ int mgf_write_head(uint8_t* dst) { return num_put(dst, "BEGIN IONS\nTITLE=", kMgfHeadLen); }
__host__ __device__ __forceinline__ int mgf_write_tail(uint8_t* dst) { return num_put(dst, "END IONS\n\n", kMgfTailLen); }

// one entry, serially: what the kernels compute a lane per field and per peak
__host__ __device__ inline int64_t mgf_entry_len(int64_t title_len, float pm, int32_t charge, float rt, int64_t cluster, const float* mz,
                                                 const float* intensity, int64_t n_peaks) {
    int64_t len = kMgfHeadLen + title_len + kMgfTailLen;
    for (int f = 0; f < kMgfFields; ++f) len += mgf_field_len(f, pm, charge, rt, cluster);
    for (int64_t j = 0; j < n_peaks; ++j) len += mgf_peak_len(mz[j], intensity[j]);
    return len;
}

__host__ __device__ inline int64_t mgf_write_entry(uint8_t* dst, const uint8_t* title, int64_t title_len, float pm, int32_t charge, float rt,
                                                   int64_t cluster, const float* mz, const float* intensity, int64_t n_peaks) {
    int64_t at = mgf_write_head(dst);
    for (int64_t i = 0; i < title_len; ++i) dst[at + i] = title[i];
    at += title_len;
    for (int f = 0; f < kMgfFields; ++f) at += mgf_write_field(dst + at, f, pm, charge, rt, cluster);
    for (int64_t j = 0; j < n_peaks; ++j) at += mgf_write_peak(dst + at, mz[j], intensity[j]);
    at += mgf_write_tail(dst + at);
    return at;
}

}  // namespace fal
