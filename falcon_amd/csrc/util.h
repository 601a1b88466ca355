// Small shared launch helpers (implemented in sortutil.hip, the inline ones here).
#pragma once
#include <algorithm>
#include "common.h"
#include "peakmatch.h"

namespace fal {
// blocks of a grid-stride kernel over `items`, `per_block` to a block: at least one, at most 16 a compute unit
inline unsigned capped_grid(const fal_ctx* ctx, int64_t items, int per_block) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, per_block), (int64_t)ctx->num_cus * 16));
}

// The meta block of the text readers and writers: META_WORDS device words a call clears, its kernels set and its one
// synchronisation reads back.  meta[META_FLAGS]: the call's flag bits; meta[META_COUNT]: the mark table's entries (textscan.h).
enum { META_COUNT = 0, META_FLAGS = 1, META_WORDS = 4 };

// the meta words on the host, through the pinned buffer; `extra`: one more device word, read into host[META_WORDS].  Synchronises
inline int read_meta(fal_ctx* ctx, const unsigned long long* meta, const unsigned long long** host, const int64_t* extra = nullptr) {
    unsigned long long* h = nullptr;
    FAL_TRY(ctx->pinned_reserve(sizeof(unsigned long long) * (META_WORDS + 1), (void**)&h));
    FAL_CHECK_HIP(hipMemcpyAsync(h, meta, sizeof(unsigned long long) * META_WORDS, hipMemcpyDeviceToHost, ctx->stream));
    if (extra) FAL_CHECK_HIP(hipMemcpyAsync(h + META_WORDS, extra, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FAL_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *host = h;
    return FAL_OK;
}

// out[0..n) = exclusive prefix of in (int32 flags/counts), out[n] = total (all on device).  Sums are int64 throughout.
// Three forms (sortutil.hip device_scan_t), by nb = ceil(n / 1024) blocks:
//   nb <= 1,025 (n <= 1,049,600)   block sums + fused apply: every block adds up the sums in front of it in ONE round of
//                                  its front-sum loop (1,024 threads, block index <= 1,024); the last block writes the total
//   nb <= 4,096 (n <= 4,194,304)   the same two launches, the front-sum loop goes round up to four times
//   nb >  4,096 (n >= 4,194,305)   block sums -> exclusive_scan_kernel over them (ivf.hip, one workgroup) -> scan_apply_kernel
//                                  -> a device-to-device copy of the total
// tests/test_gpu_plumbing.py has a case on each side of both switches, for both input types.
int device_scan_i32(fal_ctx* ctx, const int32_t* in, int64_t n, int64_t* out, int scratch_slot);
int device_scan_i64(fal_ctx* ctx, const int64_t* in, int64_t n, int64_t* out, int scratch_slot);   // same, int64 input
// stable LSD radix sort of (uint32 key, int32 value) pairs on bits [0, end_bit)
int sort_pairs_u32_i32(fal_ctx* ctx, const uint32_t* kin, uint32_t* kout, const int32_t* vin, int32_t* vout,
                       int64_t n, int end_bit, int scratch_slot);
// stable LSD radix sort of (uint64 key, 8-byte value) pairs on all 64 key bits (exact.hip).  The values are only moved: any
// 8-byte payload may travel as the bit pattern of a double
int sort_pairs_u64_f64(fal_ctx* ctx, uint64_t* kin, uint64_t* kout, double* vin, double* vout, int64_t n, int scratch_slot);
// a9 / a10 / a11+a12 with every count left on the device (graph.hip, tail.hip)
// (*extent_out: per row, one past its last stored neighbour -- valid until SLOT_DB is reserved again)
int dbscan_dev(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k, float eps, int32_t* labels,
               int64_t** d_count_out, const int32_t** extent_out = nullptr, const int32_t* nb_count = nullptr);
// f4: hierarchical clustering of the neighbour graph cut at t (linkage.hip): method 0 single, 1 complete, 2 average
int linkage_dev(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k, float t, int method, int32_t* labels,
                int64_t** d_count_out);
// the edge source of linkage_dev_src: the ANN's ELL lists (float32), or exact mode's symmetric CSR (float64, sorted-row ids);
// exact_fill: every member pair of a component is scored again from `peaks` (average linkage), *err set on a component of
// more than kMaxComp peaks (peaks.err)
struct LinkageSource {
    const int32_t* nb_idx = nullptr;
    const float* nb_dist = nullptr;
    int k = 0;
    const int64_t* csr_ptr = nullptr;
    const int32_t* csr_idx = nullptr;
    const double* csr_dist = nullptr;
    bool exact_fill = false;
    ExactPeaks peaks{};
};
int linkage_dev_src(fal_ctx* ctx, const LinkageSource& src, int64_t n, double t, int method, int32_t* labels,
                    int64_t** d_count_out);
int refine_dev(fal_ctx* ctx, int32_t* labels, int64_t n, const float* mz, const float* rt, double tol, int is_da,
               double rt_tol, const int64_t* d_count_in, int64_t** d_count_out);
int finalize_dev(fal_ctx* ctx, const int32_t* labels_sorted, int64_t n, const int64_t* d_count,
                 const int64_t* row_order, const int32_t* nb_idx, const float* nb_dist, int k, int32_t* labels_out,
                 int32_t* medoids_out, int64_t** d_noise_out, const int32_t* extent = nullptr,
                 const ExactPeaks* exact = nullptr);
// exact mode's medoid scores (exact.hip): per member, the float32 sum in ascending member order of float32(d) to every other
// member of its cluster, all pairs scored again; argmin per cluster into best (score bits, row), ties to the lowest row
int exact_medoids_dev(fal_ctx* ctx, const ExactPeaks& pk, const int32_t* labels_sorted, int64_t n, const int32_t* size,
                      unsigned long long* best);
}  // namespace fal
