// mzML structure on the device: the pure functions of the reader -- tag classifier with its attribute reader, and the walker
// over one spectrum's tag records.  Shared by mzmlscan.hip's kernels and the host build of the CPU tests
// (tests/hostbuild_mzml.py); they mirror falcon_amd/ms_io/mzml_io._spectrum / _array, which stay the reader of record: whatever
// these functions do not decide ("not decided": they never guess and never report an error) is decided by that reader on the host.
//
// Tags.  A tag runs from its '<' to the first '>' outside a "..." or '...' value, which must come before the next '<'.  The only
// attribute grammar taken is name="value" pairs, each behind at least one space, tab, CR or LF; a '-quoted value, anything but
// '=' and '"' directly behind the name, '&', a byte >= 0x80 anywhere in the tag and a byte < 0x20 inside a value leave the tag
// not decided.  "<!", "<?" and a tag or attribute name with ':' are markup: the whole text is the host reader's.
//
// Values.  ms level and array lengths: 1 to 9 decimal digits.  m/z and scan start time: mgf_parse_double.  Charge: a decided
// double with |v| < 2^31 truncated toward zero (int(float(v))), and not 0 (0 is "no charge" in the output column).
#pragma once
#include <stdint.h>
#include "mgfparse.h"

namespace fal {

enum { MZ_OTHER = 0, MZ_SPECTRUM, MZ_CVPARAM, MZ_GROUPREF, MZ_SCANLIST, MZ_SCAN, MZ_PRECLIST, MZ_PREC, MZ_SILIST, MZ_SI, MZ_BDALIST,
       MZ_BDA, MZ_BINARY, MZ_KIND = 15 };
enum { MZ_OPEN = 0, MZ_CLOSE = 1, MZ_SELF = 2, MZ_FORM_SHIFT = 4, MZ_FORM = 3 };
enum { MZ_UNDECIDED = 1 << 6, MZ_MARKUP = 1 << 7, MZ_HAS_VALUE = 1 << 8 };
enum { MZ_ST_OK = 0, MZ_ST_SKIP = 1, MZ_ST_HOST = 2 };
// array flags of fal_decode_peaks (falcon_hip.h FAL_PEAK_*; mzmlscan.hip asserts that they agree)
enum { MZ_PEAK_F64 = 1, MZ_PEAK_ZLIB = 2, MZ_PEAK_NP_LINEAR = 16, MZ_PEAK_NP_PIC = 32, MZ_PEAK_NP_SLOF = 48 };

// one tag: kind | form << 4 | MZ_* bits; cvParam: accession code (MS:ddddddd -> the 7 digits, else 0) and the value's byte
// range; spectrum: the id's byte range and defaultArrayLength; binaryDataArray: arrayLength (-1: absent); end: the tag's '>'
struct MzTag {
    int32_t info, code, v_lo, v_hi, ival, end;
};

__host__ __device__ __forceinline__ int mz_kind(const MzTag& t) { return t.info & MZ_KIND; }
__host__ __device__ __forceinline__ int mz_form(const MzTag& t) { return (t.info >> MZ_FORM_SHIFT) & MZ_FORM; }

// 1 to 9 decimal digits -> value
__host__ __device__ __forceinline__ bool mzml_parse_uint(const uint8_t* p, int len, int32_t* out) {
    if (len < 1 || len > 9) return false;
    int32_t v = 0;
    for (int i = 0; i < len; ++i) {
        if (!mgf_digit(p[i])) return false;
        v = v * 10 + (int32_t)(p[i] - '0');
    }
    *out = v;
    return true;
}

__host__ __device__ __forceinline__ int mzml_tag_kind(const uint8_t* p, int n) {
    switch (n) {
        case 4: return mgf_equals(p, n, "scan", 4, false) ? MZ_SCAN : MZ_OTHER;
        case 6: return mgf_equals(p, n, "binary", 6, false) ? MZ_BINARY : MZ_OTHER;
        case 7: return mgf_equals(p, n, "cvParam", 7, false) ? MZ_CVPARAM : MZ_OTHER;
        case 8: return mgf_equals(p, n, "spectrum", 8, false) ? MZ_SPECTRUM : mgf_equals(p, n, "scanList", 8, false) ? MZ_SCANLIST : MZ_OTHER;
        case 9: return mgf_equals(p, n, "precursor", 9, false) ? MZ_PREC : MZ_OTHER;
        case 11: return mgf_equals(p, n, "selectedIon", 11, false) ? MZ_SI : MZ_OTHER;
        case 13: return mgf_equals(p, n, "precursorList", 13, false) ? MZ_PRECLIST : MZ_OTHER;
        case 15: return mgf_equals(p, n, "selectedIonList", 15, false) ? MZ_SILIST
                        : mgf_equals(p, n, "binaryDataArray", 15, false) ? MZ_BDA : MZ_OTHER;
        case 19: return mgf_equals(p, n, "binaryDataArrayList", 19, false) ? MZ_BDALIST : MZ_OTHER;
        case 26: return mgf_equals(p, n, "referenceableParamGroupRef", 26, false) ? MZ_GROUPREF : MZ_OTHER;
        default: return MZ_OTHER;
    }
}

// "MS:" and 7 digits -> their value; anything else 0
__host__ __device__ __forceinline__ int32_t mzml_accession(const uint8_t* p, int len) {
    int32_t v = 0;
    if (len != 10 || p[0] != 'M' || p[1] != 'S' || p[2] != ':' || !mzml_parse_uint(p + 3, 7, &v)) return 0;
    return v;
}

// the tag whose '<' is p[0]; p[0, limit): the bytes up to the next '<' (or the end of the text); base: the text position of p[0]
__host__ __device__ __forceinline__ void mzml_classify_tag(const uint8_t* p, int limit, int32_t base, MzTag* out) {
    MzTag t = {MZ_OTHER, 0, 0, 0, -1, base + limit - 1};
    const uint32_t c1 = limit > 1 ? p[1] : 0;
    if (c1 == '!' || c1 == '?') {
        t.info = MZ_MARKUP | MZ_UNDECIDED;
        *out = t;
        return;
    }
    // the closing '>': a quote-aware walk
    int end = -1;
    bool bad = false;
    uint32_t quote = 0;
    for (int i = 1; i < limit; ++i) {
        const uint32_t c = p[i];
        bad |= c >= 0x80;
        if (quote) {
            if (c == quote) quote = 0;
            else bad |= c == '&' || c < 0x20;
        } else if (c == '"') {
            quote = c;
        } else if (c == '\'') {
            quote = c;
            bad = true;
        } else if (c == '>') {
            end = i;
            break;
        }
    }
    if (end < 0) {                                                     // no '>' before the next '<': nothing of it is known
        t.info = MZ_UNDECIDED;
        *out = t;
        return;
    }
    t.end = base + end;
    int form = MZ_OPEN, i = 1;
    if (c1 == '/') {
        form = MZ_CLOSE;
        i = 2;
    }
    const int n0 = i;
    bool markup = false;
    while (i < end && !mgf_space(p[i]) && p[i] != '/') {
        markup |= p[i] == ':';
        ++i;
    }
    const int kind = mzml_tag_kind(p + n0, i - n0);
    bad |= i == n0;
    int aend = end;
    if (form == MZ_OPEN && p[end - 1] == '/' && end - 1 >= i) {
        form = MZ_SELF;
        aend = end - 1;
    }
    bool has_value = false;
    int j = i;
    while (!bad) {                                                     // name="value" pairs, each behind whitespace
        const int j0 = j;
        while (j < aend && mgf_space(p[j])) ++j;
        if (j >= aend) break;
        if (j == j0 || form == MZ_CLOSE) {
            bad = true;
            break;
        }
        const int a0 = j;
        while (j < aend && p[j] != '=' && p[j] != '"' && p[j] != '\'' && !mgf_space(p[j])) {
            markup |= p[j] == ':';
            ++j;
        }
        const int a1 = j;
        if (a1 == a0 || j + 1 >= aend || p[j] != '=' || p[j + 1] != '"') {
            bad = true;
            break;
        }
        const int v0 = j + 2;
        j = v0;
        while (j < aend && p[j] != '"') ++j;
        if (j >= aend) {
            bad = true;
            break;
        }
        const int v1 = j++;
        const uint8_t* a = p + a0;
        const int an = a1 - a0;
        if (kind == MZ_CVPARAM) {
            if (mgf_equals(a, an, "accession", 9, false)) t.code = mzml_accession(p + v0, v1 - v0);
            else if (mgf_equals(a, an, "value", 5, false)) {
                has_value = true;
                t.v_lo = base + v0;
                t.v_hi = base + v1;
            }
        } else if (kind == MZ_SPECTRUM) {
            if (mgf_equals(a, an, "id", 2, false)) {
                has_value = true;
                t.v_lo = base + v0;
                t.v_hi = base + v1;
            } else if (mgf_equals(a, an, "defaultArrayLength", 18, false)) {
                bad |= !mzml_parse_uint(p + v0, v1 - v0, &t.ival);
            }
        } else if (kind == MZ_BDA) {
            if (mgf_equals(a, an, "arrayLength", 11, false)) bad |= !mzml_parse_uint(p + v0, v1 - v0, &t.ival);
        }
    }
    t.info = kind | (form << MZ_FORM_SHIFT) | (bad ? MZ_UNDECIDED : 0) | (markup ? MZ_MARKUP | MZ_UNDECIDED : 0) | (has_value ? MZ_HAS_VALUE : 0);
    *out = t;
}

// a byte of a binary element's text the device copies as it is: base64 and every other printable byte but '&' (whitespace is
// stripped by the host reader, an entity is expanded, anything else fails there in its own way: not decided)
__host__ __device__ __forceinline__ bool mzml_binary_byte(uint32_t c) { return c > 0x20 && c < 0x7F && c != '&'; }

// what the walker found in one spectrum; row 0: the m/z array, row 1: the intensity array
struct MzSpectrum {
    int32_t status, id_lo, id_hi, charge;
    double pmz, rt;
    int32_t text_lo[2], text_hi[2], count[2], flags[2];
};

__host__ __device__ __forceinline__ bool mzml_value_double(const uint8_t* text, const MzTag& t, double* v) {
    return (t.info & MZ_HAS_VALUE) && mgf_parse_double(text + t.v_lo, t.v_hi - t.v_lo, v);
}

__host__ __device__ __forceinline__ bool mzml_value_charge(const uint8_t* text, const MzTag& t, int32_t* out) {
    double v;
    if (!mzml_value_double(text, t, &v) || !(v > -2147483648.0 && v < 2147483648.0)) return false;
    *out = (int32_t)v;
    return *out != 0;
}

// the nodes whose direct children count: the spectrum and the first chain below it
enum { MZN_SPEC = 0, MZN_SCANLIST, MZN_SCAN, MZN_PRECLIST, MZN_PREC, MZN_SILIST, MZN_SI, MZN_BDALIST, MZN_BDA };
enum { MZB_MZ = 1, MZB_INT = 2, MZB_F32 = 4, MZB_F64 = 8, MZB_ZLIB = 16, MZB_NONE = 32, MZB_NP = 64 /* six bits from here */,
       MZB_NP_ALL = 63 * 64, MZB_TRUNC = 4096 };

__host__ __device__ __forceinline__ uint32_t mzml_array_bit(int32_t code) {
    switch (code) {
        case 1000514: return MZB_MZ;
        case 1000515: return MZB_INT;
        case 1000521: return MZB_F32;
        case 1000523: return MZB_F64;
        case 1000574: return MZB_ZLIB;
        case 1000576: return MZB_NONE;
        case 1002312: case 1002313: case 1002314: return (uint32_t)MZB_NP << (code - 1002312);
        case 1002746: case 1002747: case 1002748: return (uint32_t)MZB_NP << (3 + code - 1002746);
        case 1003089: case 1003090: case 1003091: return MZB_TRUNC;
        default: return 0;
    }
}

// one spectrum: tags[k0] its <spectrum ...>, tags[k1] its </spectrum>; pos[k]: the '<' of tag k
__host__ __device__ __forceinline__ void mzml_walk(const uint8_t* text, const MzTag* tags, const int32_t* pos, int64_t k0, int64_t k1,
                                                   MzSpectrum* o) {
    const MzTag sp = tags[k0];
    MzSpectrum r = {MZ_ST_HOST, 0, 0, 0, 0.0, -1.0, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
    bool hard = ((sp.info | tags[k1].info) & MZ_UNDECIDED) != 0;      // an undecided tag, a group ref, a depth that does not close: always HOST
    bool soft = false;                              // outside the fast forms, but only if the spectrum is read at all
    int depth = 0, node = MZN_SPEC, node_depth = 0;
    uint32_t seen = 0;                              // bit n: a first child that opens node n was met
    bool have_level = false, level_ok = false, have_rt = false, have_mz = false, have_ch = false, have_pch = false;
    bool ch_ok = false, pch_ok = false;
    int32_t level = 0, ch = 0, pch = 0;
    uint32_t bits = 0;                              // of the binaryDataArray being read
    int32_t alen = -1, b_lo = 0, b_hi = 0;
    bool have_bin = false;
    int n_arr[2] = {0, 0};
    const int32_t default_count = sp.ival >= 0 ? sp.ival : 0;

    const auto finish_array = [&]() {
        const int which = (bits & MZB_MZ) ? 0 : (bits & MZB_INT) ? 1 : -1;
        if (which < 0) return;                      // neither kind: the host reader ignores it before looking at anything else
        const uint32_t np = bits & MZB_NP_ALL, others = bits & (MZB_ZLIB | MZB_NONE | MZB_TRUNC);
        int32_t flags = 0;
        if (np) {
            if ((np & (np - 1)) || others) soft = true;
            const int c = __builtin_ctz(np >> 6);   // 0-2 plain, 3-5 followed by zlib
            flags = ((c % 3) + 1) * MZ_PEAK_NP_LINEAR | (c >= 3 ? MZ_PEAK_ZLIB : 0);
        } else {
            if ((bits & MZB_TRUNC) || (others == (MZB_ZLIB | MZB_NONE))) soft = true;
            flags = (bits & MZB_ZLIB) ? MZ_PEAK_ZLIB : 0;
            if (bits & MZB_F64) flags |= MZ_PEAK_F64;
            else if (!(bits & MZB_F32)) soft = true;
        }
        if (!have_bin) soft = true;
        if (n_arr[which]++) {
            soft = true;                            // a second array of the kind
            return;
        }
        r.text_lo[which] = b_lo;
        r.text_hi[which] = b_hi;
        r.count[which] = alen >= 0 ? alen : default_count;
        r.flags[which] = flags;
    };

    for (int64_t k = k0 + 1; k < k1 && !hard; ++k) {
        const MzTag t = tags[k];
        const int kind = mz_kind(t), form = mz_form(t);
        if ((t.info & MZ_UNDECIDED) || (kind == MZ_GROUPREF && form != MZ_CLOSE)) {
            hard = true;
            break;
        }
        if (form == MZ_CLOSE) {
            if (--depth < 0) hard = true;
            else if (depth < node_depth) {
                if (node == MZN_BDA) finish_array();
                node = (node == MZN_SCANLIST || node == MZN_PRECLIST || node == MZN_BDALIST) ? MZN_SPEC : node - 1;
                --node_depth;
            }
            continue;
        }
        if (depth == node_depth) {                  // a direct child of the node
            if (kind == MZ_CVPARAM) {
                if (node == MZN_SPEC && t.code == 1000511 && !have_level) {
                    have_level = true;
                    level_ok = (t.info & MZ_HAS_VALUE) && mzml_parse_uint(text + t.v_lo, t.v_hi - t.v_lo, &level);
                } else if (node == MZN_SCAN && t.code == 1000016 && !have_rt) {
                    have_rt = true;
                    if (!mzml_value_double(text, t, &r.rt)) soft = true;
                } else if (node == MZN_SI && t.code == 1000744 && !have_mz) {
                    have_mz = true;
                    if (!mzml_value_double(text, t, &r.pmz)) soft = true;
                } else if (node == MZN_SI && t.code == 1000041 && !have_ch) {
                    have_ch = true;
                    ch_ok = mzml_value_charge(text, t, &ch);
                } else if (node == MZN_SI && t.code == 1000633 && !have_pch) {
                    have_pch = true;
                    pch_ok = mzml_value_charge(text, t, &pch);
                } else if (node == MZN_BDA) {
                    bits |= mzml_array_bit(t.code);
                }
            } else {
                int child = -1;
                if (node == MZN_SPEC) child = kind == MZ_SCANLIST ? MZN_SCANLIST : kind == MZ_PRECLIST ? MZN_PRECLIST : kind == MZ_BDALIST ? MZN_BDALIST : -1;
                else if (node == MZN_SCANLIST) child = kind == MZ_SCAN ? MZN_SCAN : -1;
                else if (node == MZN_PRECLIST) child = kind == MZ_PREC ? MZN_PREC : -1;
                else if (node == MZN_PREC) child = kind == MZ_SILIST ? MZN_SILIST : -1;
                else if (node == MZN_SILIST) child = kind == MZ_SI ? MZN_SI : -1;
                else if (node == MZN_BDALIST) child = kind == MZ_BDA ? MZN_BDA : -1;
                if (child >= 0 && child != MZN_BDA && (seen >> child & 1)) child = -1;        // only the first of its kind
                if (child >= 0) {
                    seen |= 1u << child;
                    if (child == MZN_BDA) {
                        bits = 0;
                        alen = t.ival;
                        have_bin = false;
                        b_lo = b_hi = 0;
                    }
                    if (form == MZ_OPEN) {
                        node = child;
                        node_depth = depth + 1;
                    } else if (child == MZN_BDA) {
                        finish_array();
                    }
                } else if (node == MZN_BDA && kind == MZ_BINARY && !have_bin) {
                    have_bin = true;
                    if (form == MZ_OPEN) {          // its text: up to the next tag, which has to be its close
                        const MzTag nx = tags[k + 1];
                        b_lo = t.end + 1;
                        b_hi = pos[k + 1];
                        if (k + 1 >= k1 || (nx.info & MZ_UNDECIDED) || mz_kind(nx) != MZ_BINARY || mz_form(nx) != MZ_CLOSE) soft = true;
                    }
                }
            }
        }
        if (form == MZ_OPEN) ++depth;
    }
    const MzSpectrum none = {MZ_ST_HOST, 0, 0, 0, 0.0, 0.0, {0, 0}, {0, 0}, {0, 0}, {0, 0}};      // not OK: every column and row zero
    if (hard || depth != 0) {
        *o = none;
        return;
    }
    if (!have_level || (level_ok && level <= 1)) {
        r = none;
        r.status = MZ_ST_SKIP;
        *o = r;
        return;
    }
    const bool charge_ok = have_ch ? ch_ok : have_pch ? pch_ok : true;
    const bool ok = level_ok && !soft && (sp.info & MZ_HAS_VALUE) && (seen >> MZN_SCAN & 1) && (seen >> MZN_SI & 1) && have_mz && charge_ok &&
                    (seen >> MZN_BDALIST & 1) && n_arr[0] == 1 && n_arr[1] == 1;
    if (ok) {
        r.status = MZ_ST_OK;
        r.id_lo = sp.v_lo;
        r.id_hi = sp.v_hi;
        r.charge = have_ch ? ch : have_pch ? pch : 0;
        if (!have_rt) r.rt = -1.0;
    } else {
        r = none;
    }
    *o = r;
}

}  // namespace fal
