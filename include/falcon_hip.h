/*
 * falcon_hip.h -- C ABI of libfalcon_hip.so: falcon's vectorise -> ANN -> DBSCAN hot
 * path as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (bittremieux/falcon @ 2024-12-23) is pure Python and has no FFI; the seam
 * this library sits behind is the one call `cluster.generate_clusters(...)`
 * (reference falcon/cluster/cluster.py:24-156, call site falcon/falcon.py:178-188).
 * Each entry point below names the reference code (file:line) whose work it does.
 * INTEGRATION.md shows the ctypes binding a falcon maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative FAL_E* code and never throws or
 *     aborts across the boundary; fal_last_error() returns a thread-local message;
 *   - plain C types only; pointers marked [dev] are device (HBM) pointers valid on the
 *     context's device (e.g. torch tensor .data_ptr()), [host] are host pointers;
 *   - the CALLER allocates every input/output array; the library owns only the opaque
 *     handles (fal_ctx, fal_ivf) and grow-only scratch inside the context;
 *   - all device work is enqueued on the context's stream; outputs are valid after
 *     fal_ctx_sync() (or any later call on the same context that reads them);
 *   - one fal_ctx per device, not shared between threads;
 *   - there is NO CPU fallback: a context can only be created on a HIP device.
 */
#ifndef FALCON_HIP_H
#define FALCON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAL_OK            0
#define FAL_EINVAL       -1   /* bad argument */
#define FAL_EHIP         -2   /* a HIP runtime call failed */
#define FAL_ENOMEM       -3   /* device allocation failed */
#define FAL_ENODEV       -4   /* no usable gfx950 device */
#define FAL_EUNSUPPORTED -5   /* parameter outside the compiled limits */
#define FAL_EINTERNAL    -6   /* a library invariant failed (only raised under FALCON_DEBUG_POISON=1) */

#define FAL_DTYPE_F32 0
#define FAL_DTYPE_F16 1
#define FAL_DTYPE_SPLIT16 2   /* per row: low_dim f16 'hi' = f16(x), then low_dim f16 'lo' = f16((x - hi) * 2048) */
#define FAL_OUT_F32_F16   3   /* fal_vectorize_rows: float32 rows to `out` + their float16 rounding to `out2` (= fal_vectorize_pair) */
#define FAL_OUT_F16_IMAGE 4   /* fal_vectorize_rows: float16 VECTORS to `out2` + their float32 image to `out` (= fal_vectorize_f16_image) */

#define FAL_MAX_LOW_DIM   1024     /* multiple of 8 */
#define FAL_MAX_K_ANN      256
#define FAL_MAX_N_PROBE    128
#define FAL_MAX_N_LIST  131072

typedef struct fal_ctx fal_ctx;
typedef struct fal_ivf fal_ivf;

/* ---- library / context ------------------------------------------------------------- */
int         fal_version(void);
const char* fal_last_error(void);
int fal_device_count(int* count);
/* own_stream != 0: the library creates (and later destroys) a private stream and `stream`
 * is ignored.  own_stream == 0: the context enqueues on the caller's hipStream_t `stream`
 * (e.g. torch.cuda.current_stream().cuda_stream; NULL is the legacy default stream). */
int fal_ctx_create(int device, void* stream, int own_stream, fal_ctx** out);
int fal_ctx_destroy(fal_ctx* ctx);
int fal_ctx_sync(fal_ctx* ctx);
/* The one-shot call pattern of the reference (falcon.py:153-193: generate_clusters ONCE per precursor charge, in a fresh
 * process) makes the FIRST pass the only one.  fal_ctx_plan: before it, load the code objects of every kernel on the context's
 * device (otherwise loaded one translation unit at a time between the first pass's kernels) and size the scratch slots that follow
 * from the shape alone (n spectra, k_ann, n_probe, batch_size); a host-side call, safe at any time, never shrinks anything.
 * fal_ctx_trim: return the context's cached device memory (scratch slots, free pool blocks) to the driver -- between jobs of very
 * different sizes; drains the stream. */
int fal_ctx_plan(fal_ctx* ctx, int64_t n, int low_dim, int k_ann, int n_probe, int64_t batch_size);
int fal_ctx_trim(fal_ctx* ctx);
/* Elapsed milliseconds (HIP events on the context's stream) of the kernels the LAST
 * call of the named stage enqueued; used by bench.py for the roofline figure.
 * stage: 0 vectorize, 1 kmeans/ivf build, 2 coarse probe, 3 fine scan (cosine kernel),
 * 4 top-k select, 5 filter, 6 dbscan, 7 tail, 8 the launches of the cosine kernel alone (dense4_kernel / dense_kernel /
 * scan16_kernel / list16_kernel / ivf_list4_kernel; a subset of stage 3: the exact pair chains and the one-block
 * buckets' dense_tiny4_kernel are not in it). */
int fal_ctx_stage_ms(fal_ctx* ctx, int stage, float* ms, int64_t* launches);
int fal_ctx_enable_timing(fal_ctx* ctx, int on);
/* Work counters of the LAST fal_ivf_search_topk on this context (for roofline accounting):
 * which = 0: (query, candidate) inner products the fine scan produced results for
 *            (= sum over queries of candidates in their probed lists; n_b^2 per flat bucket);
 * which = 1: (query, centroid) inner products of the coarse quantiser;
 * which = 2: number of scan kernel launches (batches);  3: bytes of the sims scratch buffer;
 * which = 4: inner products the matrix cores actually computed for the flat buckets (tile padding
 *            included; the fp32 kernel computes only the blocks on/above each bucket's diagonal);
 * which = 5: queries of the last prefiltered search that took the exact fallback (after a sync);
 * which = 6: precondition check of the float16 prefilters for the LAST index built on this context: bit 0 = rows of
 *            an indexed bucket, bit 1 = rows handed to the flat prefilter hold negative / non-finite components, so
 *            that index is built / searched with the exact kernels (see fal_ivf_build_x16);
 * which = 7, 8: the part of counters 0 and 4 that belongs to flat buckets of up to 32 rows, whose kernel is not
 *            timed under stage 8 (subtract them to price stage 8's launches);
 * which = 9: the pairs the Hungarian solver finished in the LAST fal_assign_nearest or fal_member_scores on this context;
 * which = 10: 1 when the last fal_cluster_graph_tiled ran per bucket tile, 0 when it took the per-row path;
 * which = 11: the tiles of that call whose eps-edges took the edge list's second pass;
 * which = 12: the pairs the greedy kernel finished in the LAST fal_network_edges on this context;
 * which = 13: the edges the LAST fal_network_families on this context cut;
 * which = 14: the pairs the greedy kernels finished in the LAST fal_library_search on this context;
 * which = 15: the nodes the LAST fal_network_propagate on this context reached (hops >= 1). */
int fal_ctx_counter(fal_ctx* ctx, int which, int64_t* value);

/* ---- a1  bin geometry: reference spectrum.py:172-199 `get_dim` (float32) --- [host] */
int fal_get_dim(float min_mz, float max_mz, float bin_size,
                uint32_t* dim, float* start_dim, float* end_dim);

/* ---- a3  feature-hash lookup table: MurmurHash3_x86_32(int32 bin, seed) % low_dim;
 *          spec reference README.md:124-131 ------------------------------------ [host] */
int fal_hash_lookup(uint32_t n_bins, uint32_t low_dim, uint32_t seed, uint32_t* out_table);

/* ---- a2  m/z -> bin index (the CSR `indices` of reference spectrum.py:250-296
 *          `_to_vector`): floor(((double)mz - min_mz) / bin_size) as int32 ------ [dev] */
int fal_to_vector_indices(fal_ctx* ctx, const float* mz, int64_t nnz,
                          double min_mz, double bin_size, int32_t* out_indices);

/* ---- a2+a3  CSR peaks -> dense low_dim vectors, L2-normalised: reference
 *          spectrum.py:202-247 `to_vector` with the projection realised as feature
 *          hashing.  Row r of `out` is spectrum row_order[r] (row_order may be NULL).
 *          out: [n, low_dim] float32 or float16, or [n, 2, low_dim] float16 hi/lo planes of the
 *          float32 result (out_dtype, FAL_DTYPE_*).  Peaks whose bin lies outside [0, n_bins)
 *          are ignored; an all-zero row stays zero. ------------------------------- [dev] */
int fal_vectorize(fal_ctx* ctx, const float* mz, const float* intensity,
                  const int64_t* indptr, const int64_t* row_order, int64_t n,
                  double min_mz, double bin_size, uint32_t n_bins,
                  uint32_t low_dim, uint32_t seed, int normalize, int out_dtype, void* out);
/* The same with TWO outputs from one pass over the peaks: the float32 rows and their float16 rounding (the copy the
 * float16 prefilters of the index build and of the search read; same values as fal_vectorize with FAL_DTYPE_F16). [dev] */
int fal_vectorize_pair(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr,
                       const int64_t* row_order, int64_t n, double min_mz, double bin_size, uint32_t n_bins,
                       uint32_t low_dim, uint32_t seed, int normalize, float* out_f32, void* out_f16);
/* float16 VECTORS (BASELINE configs[4]: low_dim 800 fp16): out_f16 = the rows rounded to float16 (= fal_vectorize with
 * FAL_DTYPE_F16), out_f32_image = the float32 image of those rounded values.  The similarity of two float16 vectors is
 * defined as the k-ordered float32 fmaf chain over their images (products of float16 values are exact in float32), so an
 * index built on the image with out_f16 as its prefilter copy (fal_ivf_build_x16 / fal_ivf_attach_prefilter_ex) searches
 * float16 vectors exactly and reproducibly; the oracle restates it as "round to float16, then the float32 path". [dev] */
int fal_vectorize_f16_image(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr,
                            const int64_t* row_order, int64_t n, double min_mz, double bin_size, uint32_t n_bins,
                            uint32_t low_dim, uint32_t seed, int normalize, float* out_f32_image, void* out_f16);

/* `--low_dim` is a free integer in the reference (README.md:114-117, config.py: "low_dim" of the nearest-neighbour options);
 * the cosine kernels are instantiated for rows of 64, 128, 256, 400 and 800 columns.  fal_row_width: the row width the path
 * stores `low_dim`-dimensional vectors in = the smallest of those widths >= low_dim (FAL_EUNSUPPORTED beyond 800) -- [host].
 * fal_vectorize_rows: fal_vectorize / _pair / _f16_image (out_mode = FAL_DTYPE_* / FAL_OUT_*) with the hash taken modulo
 * `low_dim` (any integer in [1, row_width]) and rows of `row_width` columns (a multiple of 8) whose columns >= low_dim are
 * zero.  A zero column adds fma(0 * 0, acc) = acc to every k-ordered inner-product chain, so every kernel downstream runs at
 * d = row_width unchanged and the similarities are those of the low_dim-dimensional vectors summed in the order of the
 * row_width-wide chain (the oracle pads the same way). ---------------------------------------- [dev] */
int fal_row_width(uint32_t low_dim, uint32_t* row_width);
int fal_vectorize_rows(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr,
                       const int64_t* row_order, int64_t n, double min_mz, double bin_size, uint32_t n_bins,
                       uint32_t low_dim, uint32_t row_width, uint32_t seed, int normalize, int out_mode,
                       void* out, void* out2 /*second output of FAL_OUT_*, else NULL*/);

/* ---- a5  precursor-m/z bucket boundaries: reference cluster.py:159-209
 *          `_get_precursor_mz_splits` over the m/z-SORTED float32 precursor array,
 *          plus (flags) the build's two extra rules: chunk the last block
 *          too, and cut at fixed windows floor(mz / mz_interval).
 *          splits_out [host] receives at most max_splits int64 boundaries
 *          (first 0, last n); *n_splits = how many. -------------------------------- */
int fal_precursor_splits(fal_ctx* ctx, const float* precursor_mz_sorted /*[dev]*/, int64_t n,
                         double tol, int tol_is_da, int64_t batch_size,
                         double mz_interval, int chunk_last,
                         int64_t* splits_out /*[host]*/, int64_t max_splits, int64_t* n_splits);

/* ---- e   the multi-GPU front end: whole precursor windows floor(mz / mz_interval) are the unit dealt to GPUs (buckets never
 *          cross a window and a window's buckets depend on its own spectra only; reference analogue: blocks are
 *          clustered independently, cluster.py:107-141).  fal_window_counts: all n_parts partitions (precursor charges) of a
 *          job in one call -- precursor_mz[p] [host array of device pointers], n[p] [host] spectra of partition p,
 *          counts[p * n_windows + w] [dev] = spectra of partition p in window w (windows >= n_windows - 1 share the last
 *          counter; the call zeroes counts first); counts_host (optional, pinned host memory, n_parts * (n_windows + 2)
 *          int32): the same table, then (first, last) occupied window of every partition (INT32_MAX, 0 for an empty
 *          one), copied stream-ordered (valid after fal_ctx_sync).  fal_window_select: the spectra whose
 *          window belongs to `rank` (owner[w], int32 per window) -- rows_out i64 ascending dataset rows, mz_out their
 *          precursor m/z; *count [host] how many (synchronises).  Buffers need room for n entries. ------------- [dev] */
int fal_window_counts(fal_ctx* ctx, const float* const* precursor_mz /*[host]*/, const int64_t* n /*[host]*/, int n_parts,
                      double mz_interval, int64_t n_windows, int32_t* counts, int32_t* counts_host /*[pinned host] or NULL*/);
int fal_window_select(fal_ctx* ctx, const float* precursor_mz, int64_t n, double mz_interval, int64_t n_windows,
                      const int32_t* owner, int rank, int64_t* rows_out, float* mz_out, int64_t* count /*[host]*/);

/* ---- a6  IVF build per bucket (k-means + inverted lists); the reference's only
 *          statement is README.md:134-136 (Faiss IndexIVFFlat, un-vendored dep
 *          setup.cfg:25).  X [dev] is [n, low_dim] float32 in precursor-sorted row order;
 *          bucket_off [host] has n_buckets+1 row offsets; n_list [host] lists per bucket
 *          (1 = flat).  Deterministic: init rows floor(i*n_b/n_list), `kmeans_iters`
 *          x (argmax-IP assign, spherical mean in row order), final assign. ---------- */
int fal_ivf_build(fal_ctx* ctx, const float* X, int64_t n, int low_dim,
                  const int64_t* bucket_off, int64_t n_buckets, const int32_t* n_list,
                  int kmeans_iters, fal_ivf** out);
/* The same build with float16 copies [n, low_dim] of X (fal_vectorize FAL_DTYPE_F16 on the same peaks) as a PREFILTER of
 * the k-means / final assignment of buckets with <= 512 lists: the arg-max runs on the f16 matrix cores and only the
 * rows whose two best centroids are closer than the float16 error bound are re-evaluated exactly in float32 -- every
 * assignment, centroid and list is identical to fal_ivf_build's (low_dim in {64, 128, 256, 400}; X16 NULL = fal_ivf_build).
 * PRECONDITION of every float16 prefilter of this library (here and fal_ivf_attach_prefilter[_ex]): X16 is the float16
 * rounding of X, and no component of X is negative, infinite or NaN -- the error bound that makes the prefiltered results
 * exact, |f16-MFMA(x.y) - fp32 chain(x.y)| <= 1.3e-3 (x.y) + 2e-6, is relative to the similarity and holds for
 * non-negative rows only (hashed spectra are: intensities >= 0).  The precondition is CHECKED, not assumed: the build's
 * pass over the rows of the indexed buckets looks at every component (one stream synchronisation when X16 is given), and
 * an index whose rows fail it is built and searched with the exact float32 kernels -- same results, no error. */
int fal_ivf_build_x16(fal_ctx* ctx, const float* X, const void* X16, int64_t n, int low_dim,
                      const int64_t* bucket_off, int64_t n_buckets, const int32_t* n_list,
                      int kmeans_iters, fal_ivf** out);
/* Optional: float16 copies of the vectors, [n, planes, low_dim] in the same (sorted) row order, that
 * the FLAT buckets are then scanned with on the f16 matrix cores: planes = 1 plain float16 rows
 * (fal_vectorize FAL_DTYPE_F16; BASELINE config 5), planes = 2 the hi/lo split of the float32
 * rows (FAL_DTYPE_SPLIT16; float32-accurate to ~3e-7).  With planes = 1 fal_ivf_build may be given
 * X = NULL as long as every bucket is flat.  The buffer is borrowed. ------------------- [dev] */
int fal_ivf_attach_f16(fal_ivf* ivf, const void* X16, int planes);
/* Optional: float16 copies [n, low_dim] of the float32 vectors (fal_vectorize FAL_DTYPE_F16 on the same
 * peaks) used ONLY as a PREFILTER by fal_ivf_search_neighbors on flat buckets: the bucket is scanned on the
 * f16 matrix cores to bracket every query's n_neighbors_ann-th best similarity, the candidates inside the
 * precursor window are then evaluated exactly in float32 and the bracket is resolved exactly where it
 * matters -- the neighbour lists are BIT-IDENTICAL to the ones computed without the prefilter, the
 * [n, candidates] similarity matrix never exists in HBM.  low_dim in {64, 128, 256, 400}; other sizes
 * ignore the prefilter.  fal_ivf_search_topk never uses it.  The buffer is borrowed.  Precondition as stated at
 * fal_ivf_build_x16 (non-negative finite components); the call checks it with one pass over X16 and one stream
 * synchronisation, and rows that fail it make the searches ignore the prefilter (exact staged scan). ---- [dev] */
int fal_ivf_attach_prefilter(fal_ivf* ivf, const void* X16);
/* The same with a choice of where the prefilter is used: which & 1 = flat buckets (as above), which & 2 = buckets
 * with an index: their fine scan runs on the f16 matrix cores over X16 itself (gathered through the index's row
 * permutation; the buffer is borrowed and must outlive the index for this part too), the k-th best key
 * of every query is bracketed from 16-bit keys, and the exact float32 work is limited to the precursor window
 * and to the candidates that can decide the k-th key.  BIT-IDENTICAL neighbour lists under the same precondition
 * (the build has already looked at the rows of the indexed buckets: if any has a negative / non-finite component
 * no float16 copy is made and the searches run the exact fine scan).  Reference: the n_probe query of README.md:107-113
 * (faiss IndexIVFFlat.search, an un-vendored dependency: setup.cfg:25). ------------------------------------ [dev] */
int fal_ivf_attach_prefilter_ex(fal_ivf* ivf, const void* X16, int which);
int fal_ivf_destroy(fal_ivf* ivf);
int fal_ivf_total_lists(const fal_ivf* ivf, int64_t* total_lists);
/* Copy the index out for inspection (any pointer may be NULL): centroids
 * [total_lists, low_dim] f32, list id of every row (bucket-local) i32[n], perm i32[n]
 * (row ids in (bucket, list, row) order), list_off i64[total_lists+1]. --------- [dev] */
int fal_ivf_export(fal_ctx* ctx, const fal_ivf* ivf, float* centroids, int32_t* assign,
                   int32_t* perm, int64_t* list_off);

/* ---- a7  n_probe query of every row against its bucket's index + top-k_ann by
 *          (inner product desc, row id asc); reference spec README.md:107-113,137-142.
 *          sim f32[n,k_ann] (pad -inf), idx i32[n,k_ann] (pad -1, ids = sorted rows). */
int fal_ivf_search_topk(fal_ctx* ctx, const fal_ivf* ivf, int n_probe, int k_ann,
                        float* sim, int32_t* idx);

/* ---- a8  neighbour filter + distance: drop self / pads / neighbours outside the
 *          precursor (and RT) tolerance, keep the first n_neighbors,
 *          dist = clip(1 - sim, 0, 1): reference cluster.py:190-195 (mass_diff usage),
 *          cluster.py:626, similarity.py:78.  rt may be NULL / rt_tol < 0 = no RT filter.
 *          nb_idx i32[n,k] (pad -1), nb_dist f32[n,k] (pad +inf). ---------------- [dev] */
int fal_filter_neighbors(fal_ctx* ctx, const float* sim, const int32_t* idx, int64_t n,
                         int k_ann, const float* precursor_mz_sorted, const float* rt_sorted,
                         double tol, int tol_is_da, double rt_tol, int n_neighbors,
                         int32_t* nb_idx, float* nb_dist);

/* ---- a7+a8 in one call: the same search with the neighbour filter applied to the k_ann
 *          selected candidates inside the selection kernel (only the survivors are sorted;
 *          the [n, k_ann] result never goes to HBM).  Output identical to
 *          fal_ivf_search_topk followed by fal_filter_neighbors; nb_count (optional)
 *          receives the number of stored neighbours of every row. ------------------ [dev] */
int fal_ivf_search_neighbors(fal_ctx* ctx, const fal_ivf* ivf, int n_probe, int k_ann,
                             const float* precursor_mz_sorted, const float* rt_sorted,
                             double tol, int tol_is_da, double rt_tol, int n_neighbors,
                             int32_t* nb_idx, float* nb_dist, int32_t* nb_count /*[n] or NULL*/);

/* ---- f4  exact re-scoring of the stored neighbours with the matched-peak cosine the
 *          reference ships: similarity.py:17-80 `cosine_fast` (pairs of peaks within
 *          fragment_tol, optimal assignment, sum of the positive pair scores), used as
 *          cluster.py:593-639 does: nb_dist = 1 - sim, sim = 0 when fewer than min_matches
 *          peaks match.  In place on nb_dist; entry order is not changed.  mz / intensity /
 *          indptr: the preprocessed spectra (dataset rows), row_order: sorted position ->
 *          dataset row.  Synchronises (FAL_EUNSUPPORTED if more than 32 peaks of one
 *          spectrum chain inside the tolerance). ------------------------------- [dev] */
int fal_rescore_neighbors(fal_ctx* ctx, const int32_t* nb_idx, float* nb_dist, int64_t n, int k,
                          const float* mz, const float* intensity, const int64_t* indptr,
                          const int64_t* row_order, double fragment_tol, int min_matches);

/* ---- e   neighbour lists ELL -> CSR, ids shifted by id_offset to global rows: the
 *          payload of the one multi-GPU exchange step (all-gatherv of the
 *          sparse neighbour lists; the reference's per-block results are likewise
 *          concatenated with offsets, cluster.py:115-141).  Entry order within a row is
 *          kept.  Segments (e.g. the charge partitions of falcon.py:151-160) chain on
 *          the device: a call writes rows [row0, row0 + n) of indptr_out and continues
 *          at nnz = indptr_out[row0] (row0 = 0 starts a new graph).  indptr i64[rows+1];
 *          idx_out / dist_out need room for every segment's n*k entries. ---------- [dev] */
int fal_neighbors_to_csr(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist,
                         const int32_t* nb_count /*[n] lengths of front-packed rows, or NULL*/,
                         int64_t n, int k, int64_t id_offset, int64_t row0, int64_t* indptr_out,
                         int32_t* idx_out, float* dist_out);
/*          Same with an id map: stored id -> id_map[id] + id_offset.  A rank that ran the path on a
 *          SUBSET of a dataset's buckets (its share of one precursor-sorted dataset) maps
 *          the subset positions back to dataset rows here (id_map = the subset's row order). -- [dev] */
int fal_neighbors_to_csr_mapped(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist,
                                const int32_t* nb_count, int64_t n, int k,
                                const int64_t* id_map /*[ids] or NULL*/, int64_t id_offset, int64_t row0,
                                int64_t* indptr_out, int32_t* idx_out, float* dist_out);

/* ---- a9  DBSCAN(eps, min_samples = 2 as reference cluster.py:66) on the sparse
 *          neighbour graph; spec README.md:143-146.  Order-independent form:
 *          clusters = components of core points, border -> lowest-index core
 *          in-neighbour, clusters numbered by lowest core row, noise = -1. -------- [dev] */
int fal_dbscan(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k,
               float eps, int32_t* labels, int64_t* n_clusters /*[host]*/);

/* ---- a10 precursor / RT refinement of every DBSCAN cluster: reference
 *          cluster.py:362-455 `_postprocess_cluster` + cluster.py:458-509 `_linkage`
 *          (1-D complete linkage cut at the tolerance; groups < 2 -> noise);
 *          final clusters numbered in (DBSCAN label, first member) order like
 *          cluster.py:293-313.  labels in/out i32[n] (sorted-row space). ---------- [dev] */
int fal_refine_clusters(fal_ctx* ctx, int32_t* labels, int64_t n,
                        const float* precursor_mz_sorted, const float* rt_sorted,
                        double tol, int tol_is_da, double rt_tol,
                        int64_t* n_clusters /*[host]*/);

/* ---- a11+a12 medoids (reference cluster.py:512-553 on the sparse graph) and label
 *          globalisation (cluster.py:556-590, 144-155): labels_sorted -> labels by DATASET
 *          row with noise renumbered n_clusters.. in dataset-row order; medoids[c] =
 *          dataset row of cluster c's medoid (c < n_clusters), then the noise rows.
 *          Every id in [0, n_clusters) must have a member: the kernel indexes row_order with
 *          the cluster's best row unconditionally. ---------------------------------- [dev] */
int fal_finalize(fal_ctx* ctx, const int32_t* labels_sorted, int64_t n, int64_t n_clusters,
                 const int64_t* row_order, const int32_t* nb_idx, const float* nb_dist, int k,
                 int32_t* labels_out, int32_t* medoids_out, int64_t* n_labels /*[host]*/);

/* ---- a9 + a10 + a11 + a12 in one call (same kernels; all intermediate counts stay on the
 *          device, a single host synchronisation at the end).  labels_sorted_scratch i32[n]
 *          receives the refined labels in sorted-row space (-1 = noise). ------------- [dev] */
int fal_cluster_graph(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k,
                      float eps, const float* precursor_mz_sorted, const float* rt_sorted,
                      double tol, int tol_is_da, double rt_tol, const int64_t* row_order,
                      int32_t* labels_sorted_scratch, int32_t* labels_out, int32_t* medoids_out,
                      int64_t* n_clusters /*[host]*/, int64_t* n_labels /*[host]*/);

/* The same for FRONT-PACKED neighbour rows of known length (what fal_ivf_search_neighbors leaves: nb_count[i] stored
 * neighbours in slots 0 .. nb_count[i] - 1, padding behind): the graph passes read the stored slots only. --- [dev] */
int fal_cluster_graph_counted(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, const int32_t* nb_count,
                              int64_t n, int k, float eps, const float* precursor_mz_sorted, const float* rt_sorted,
                              double tol, int tol_is_da, double rt_tol, const int64_t* row_order,
                              int32_t* labels_sorted_scratch, int32_t* labels_out, int32_t* medoids_out,
                              int64_t* n_clusters /*[host]*/, int64_t* n_labels /*[host]*/);

/* fal_cluster_graph_counted given the precursor buckets of the rows (bucket_off: HOST, n_buckets + 1 ascending row offsets,
 * 0 .. n -- the table the search ran on): the same results bit for bit, computed per TILE of consecutive whole buckets, one
 * workgroup per tile with the per-row state in LDS.  Contract: every stored neighbour of a row lies in the
 * row's bucket (the search is bucket by bucket).  A stored id inside [0, n) but outside its row's tile is never followed and
 * fails the call with FAL_EINVAL; the context stays usable.  A bucket of more than max_tile_rows rows, or FALCON_GRAPH_TILED=0 in
 * the environment (read per call), sends the whole call down fal_cluster_graph_counted's path.
 * fal_ctx_counter(10): 1 when the last call ran per tile, 0 when it took that path.
 * fal_ctx_counter(11): the tiles of the last call whose eps-edges did not fit the tile's edge list in LDS
 * (fal_graph_tile_capacity) and whose core rows were read a second time; 0 when the per-row path ran. --- [dev] */
int fal_cluster_graph_tiled(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, const int32_t* nb_count,
                            int64_t n, int k, float eps, const int64_t* bucket_off /*[host]*/, int64_t n_buckets,
                            const float* precursor_mz_sorted, const float* rt_sorted,
                            double tol, int tol_is_da, double rt_tol, const int64_t* row_order,
                            int32_t* labels_sorted_scratch, int32_t* labels_out, int32_t* medoids_out,
                            int64_t* n_clusters /*[host]*/, int64_t* n_labels /*[host]*/);
/* the rows that close a tile, and the most rows of one bucket the tiled path takes --- [host] */
void fal_graph_tile_limits(int* tile_rows, int* max_tile_rows);
/* *lds_bytes = the dynamic LDS of the DBSCAN tile kernel in a call whose largest tile has max_rows rows; *edge_capacity =
 * the eps-edges (stored slots below the count that hold another row of the tile within eps, one per slot) a tile of `rows`
 * rows of that call keeps in its list: 4 per row of the largest tile up to 4,864 rows, down to 6,144 at 8,192 rows, and a
 * smaller tile of the same call has the rest of the block.  Either pointer may be NULL. --- [host] */
void fal_graph_tile_capacity(int64_t max_rows, int64_t rows, int64_t* lds_bytes, int64_t* edge_capacity);

/* ---- f4  hierarchical clustering of the neighbour graph: the clustering the reference snapshot ships,
 *          fcluster(fastcluster.linkage(pdist, linkage), distance_threshold, "distance") (cluster.py:283-290), on the
 *          sparse graph with "missing pair = distance 1" (cluster.py:621-626), normally after fal_rescore_neighbors
 *          put the exact matched-peak distances into it.  method: 0 single, 1 complete, 2 average; threshold < 1.
 *          Same output contract as fal_dbscan (clusters numbered by lowest row, groups of one row = -1), so
 *          fal_refine_clusters / fal_finalize follow unchanged; fal_cluster_graph_linkage is the fused a9..a12
 *          form.  Tie order between equal merge heights is the build's own: the pair with the lowest (a, b) in the group's
 *          ascending-row numbering (pinned by tests/linkage_cases.py; PARITY with fastcluster / scipy on ties UNPINNED).
 *          The neighbour ids within a row must be DISTINCT (-1 padding aside): two slots of one row to the same neighbour
 *          are one matrix cell that two lanes would store different distances to.  Every producer in the library (top-k,
 *          filter, re-scoring) keeps them distinct.
 *          The complete / average forms synchronise the stream once more than fal_dbscan does (the sizes of the connected
 *          groups decide their scratch); a connected group of up to 256 rows is agglomerated by one wave, a larger one by
 *          a 1,024-thread workgroup, with no cap on its size beyond the memory of its m x m float64 matrix. [dev] */
int fal_linkage_cluster(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k,
                        float threshold, int method, int32_t* labels, int64_t* n_clusters /*[host]*/);
int fal_cluster_graph_linkage(fal_ctx* ctx, const int32_t* nb_idx, const float* nb_dist, int64_t n, int k,
                              float threshold, int method, const float* precursor_mz_sorted,
                              const float* rt_sorted, double tol, int tol_is_da, double rt_tol,
                              const int64_t* row_order, int32_t* labels_sorted_scratch, int32_t* labels_out,
                              int32_t* medoids_out, int64_t* n_clusters /*[host]*/, int64_t* n_labels /*[host]*/);

/* ---- f5  exact mode: the snapshot's own clustering -- the matched-peak cosine (fal_rescore_neighbors' arithmetic) of EVERY
 *          pair inside every bucket [splits[b], splits[b + 1]) of the bucket table (splits [host], first 0, last n), then the
 *          hierarchical clustering cut at threshold < 1 (cluster.py:212-331, 593-639).  Rows and ids are sorted positions;
 *          row_order maps them to the rows of the peaks CSR (mz / intensity f32, indptr i64).  A pair whose peaks chain into a
 *          component of more than 32 peaks a side fails the call with FAL_EUNSUPPORTED, as in fal_rescore_neighbors.
 *          fal_exact_edges: the pairs with d = 1 - sim <= threshold (sim = 0 below min_matches) as a symmetric CSR,
 *          rows and columns ascending: csr_indptr i64[n+1], csr_idx i32 / csr_dist f64 [max_edges]; *n_edges = directed
 *          entries (FAL_EINVAL with *n_edges set when they exceed max_edges: call again with room for them).
 *          fal_linkage_cluster_csr: fal_linkage_cluster's contract on that CSR; average linkage (method 2) scores every
 *          member pair of a connected group again (the peak arguments are needed for it only).
 *          fal_cluster_exact: edges -> linkage -> fal_refine_clusters -> medoids over all member pairs (float32 sums in
 *          ascending member order, ties to the lowest row) -> fal_finalize's labels; the edges stay in library scratch.
 *          [dev] except splits and the counts */
int fal_exact_edges(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, const int64_t* row_order,
                    int64_t n, const int64_t* splits /*[host]*/, int64_t n_splits, double fragment_tol, int min_matches,
                    double threshold, int64_t* csr_indptr, int32_t* csr_idx, double* csr_dist, int64_t max_edges,
                    int64_t* n_edges /*[host]*/);
int fal_linkage_cluster_csr(fal_ctx* ctx, const int64_t* csr_indptr, const int32_t* csr_idx, const double* csr_dist, int64_t n,
                            double threshold, int method, const float* mz, const float* intensity, const int64_t* indptr,
                            const int64_t* row_order, double fragment_tol, int min_matches, int32_t* labels,
                            int64_t* n_clusters /*[host]*/);
int fal_cluster_exact(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, const int64_t* row_order,
                      int64_t n, const int64_t* splits /*[host]*/, int64_t n_splits, double fragment_tol, int min_matches,
                      double threshold, int method, const float* precursor_mz_sorted, const float* rt_sorted, double tol,
                      int tol_is_da, double rt_tol, int32_t* labels_sorted_scratch, int32_t* labels_out, int32_t* medoids_out,
                      int64_t* n_clusters /*[host]*/, int64_t* n_labels /*[host]*/);

/* ---- f1  spectrum preprocessing, the step in front of the path: reference
 *          spectrum.py:73-169 `process_spectrum` over a CSR of raw peaks (m/z float64
 *          sorted per spectrum, intensity float32): m/z range cut (135), precursor-peak
 *          removal for charge states z..1 (139-149; charge 0 = unknown -> 1), base-peak
 *          intensity filter + the max_peaks_used most intense (151-155), validity check
 *          after every step (27-52), scaling 0 none / 1 root / 2 log / 3 rank (157), L2
 *          normalisation (55-70, 158).  Unset options: mz_min / mz_max = NaN,
 *          remove_precursor_tol < 0, min_intensity < 0, max_peaks_used = 0.
 *          valid_out i32[n]; out_indptr i64[n+1] (invalid spectra hold 0 peaks);
 *          out_mz / out_intensity f32 with room for nnz peaks. ---------------- [dev] */
int fal_process_spectra(fal_ctx* ctx, const double* mz, const float* intensity,
                        const int64_t* indptr, int64_t n, int64_t nnz,
                        const double* precursor_mz, const int32_t* precursor_charge,
                        int min_peaks, double min_mz_range, double mz_min, double mz_max,
                        double remove_precursor_tol, double min_intensity, int max_peaks_used,
                        int scaling, int32_t* valid_out, int64_t* out_indptr, float* out_mz,
                        float* out_intensity);

/* ---- peak-file payload decode (mzML / mzXML binary arrays) ------------------------------------------------------------------
 * payload: the base64 text of every array of the call, concatenated (u8[payload_bytes]).
 * arrays:  i64[n_arrays][4] = {offset into payload (multiple of 8), base64 length (multiple of 4, no whitespace),
 *          declared value count (mzML defaultArrayLength / arrayLength, mzXML peaksCount = pairs), FAL_PEAK_* flags}.
 * spectra: i64[n_spectra][2] = {m/z array, intensity array} (rows of `arrays`; an mzXML pair array is named twice).
 * inflate_bytes: device scratch for the zlib and MS-Numpress arrays, at least the sum over arrays of two terms, each rounded
 *          up to 8: the inflated capacity of a zlib array -- count x element size (x 2 for pairs); of a numpress stream, whose
 *          inflated size is not declared, the longest stream of `count` values: linear 8 (count 0), 12 (count 1), else
 *          16 + ceil(9 (count - 2) / 2); pic ceil(9 count / 2); slof 8 + 2 count -- and count x 8 for a numpress array (its
 *          decoded float64 values).  nnz_cap: room of out_mz / out_intensity (the sum of the m/z arrays' counts).
 * MS-Numpress (FAL_PEAK_NUMPRESS_*, DESIGN.md "MS-Numpress" states the format): the array's bytes (after base64, and after
 *          zlib when FAL_PEAK_ZLIB is set as well) are a numpress stream of `count` values, decoded to float64 (m/z as is,
 *          intensity rounded to float32).  A codec together with F64, BIG_ENDIAN or PAIRS is FAL_PEAK_ST_DESC.
 * -> out_indptr i64[n_spectra + 1] (the declared counts), out_mz f64, out_intensity f32 (sorted by m/z inside every spectrum,
 *    stable: the order of np.lexsort((mz, row))), status_out i32[n_spectra]: 0, or FAL_PEAK_ST_* bits (that spectrum's peaks
 *    are zeros).  A corrupt array never makes the call fail or write outside its slot. ------------------------------ [dev] */
#define FAL_PEAK_F64         1   /* 64-bit values (else 32-bit) */
#define FAL_PEAK_ZLIB        2   /* zlib stream (RFC 1950) */
#define FAL_PEAK_BIG_ENDIAN  4   /* network byte order (mzXML) */
#define FAL_PEAK_PAIRS       8   /* interleaved m/z-intensity pairs (mzXML) */
#define FAL_PEAK_NUMPRESS_LINEAR 16 /* MS:1002312 linear prediction: fixed point + two values + half-byte second differences */
#define FAL_PEAK_NUMPRESS_PIC    32 /* MS:1002313 positive integer: half-byte integers */
#define FAL_PEAK_NUMPRESS_SLOF   48 /* MS:1002314 short logged float: fixed point + 16-bit logarithms */
#define FAL_PEAK_NUMPRESS_MASK   48 /* the 2-bit codec field (0 = none); bit 64 is unassigned */
#define FAL_PEAK_ST_DESC      1  /* bad descriptor: range outside the payload, misaligned, unknown flags, count mismatch */
#define FAL_PEAK_ST_BASE64    2  /* a character outside the base64 alphabet, or misplaced padding */
#define FAL_PEAK_ST_HEADER    4  /* bad zlib header */
#define FAL_PEAK_ST_CODE      8  /* bad block type / Huffman code / distance, or the stream ends inside a block */
#define FAL_PEAK_ST_OVERFLOW 16  /* more data than the declared count */
#define FAL_PEAK_ST_SHORT    32  /* less data than the declared count */
#define FAL_PEAK_ST_ADLER    64  /* Adler-32 trailer mismatch or missing */
#define FAL_PEAK_ST_CAPACITY 128 /* inflate_bytes / nnz_cap too small */
#define FAL_PEAK_ST_NUMPRESS 256 /* bad MS-Numpress stream: header length, fixed point, or the stream ends inside a value */
int fal_decode_peaks(fal_ctx* ctx, const uint8_t* payload, int64_t payload_bytes,
                     const int64_t* arrays, int64_t n_arrays, const int64_t* spectra, int64_t n_spectra,
                     int64_t inflate_bytes, int64_t nnz_cap, int64_t* out_indptr, double* out_mz,
                     float* out_intensity, int32_t* status_out);

/* ---- MGF text -> raw peak CSR + per-spectrum columns (the device reader; DESIGN.md "MGF on the device" states the grammar;
 *          falcon_amd/ms_io/mgf_io.get_spectra is the reader it mirrors and the one that decides whatever it leaves open).
 * text: u8[n_bytes] on the device, 16-byte aligned, n_bytes < 2^31 - 1 (the caller cuts larger files behind an END IONS line).
 * fal_mgf_index: line table, line classes and spectrum table of the text -> counts_out[4] (host) = {spectra, peak lines of
 *          those spectra, FAL_MGF_FLAG_* bits, lines}.  One stream synchronisation.  A flag means "this text is the host
 *          reader's": BYTES -- a byte outside \t, \n, 0x20-0x7E, \r directly followed by \n; LINES -- more lines than one per
 *          4 bytes (the line table is sized before the count is known; the counts are then 0).
 * fal_mgf_parse: fills the caller's outputs from the tables of the fal_mgf_index call before it, which stay in scratch
 *          slots of the context (kept, not recomputed: the call checks text, n_bytes and n_spectra against that index and
 *          fails with FAL_EINVAL when they are not its own, or when fal_ctx_trim ran in between).
 * -> out_indptr i64[n + 1] (a spectrum's count = its peak lines, whether or not their values parse), out_mz f64 / out_intensity
 *    f32 with room for nnz_cap >= the indexed peak count (sorted by m/z inside every spectrum, stable: the order of
 *    np.lexsort((mz, row)), as fal_decode_peaks), precursor_mz f64[n], charge i32[n] + has_charge i32[n], retention_time f64[n]
 *    (-1 when absent), title i64[n][2] / span i64[n][2]: byte ranges [from, to) of the title value and of the spectrum from its
 *    BEGIN IONS line to the end of its END IONS line, status i32[n]: 0, or FAL_MGF_ST_HOST -- the host reader decides this
 *    spectrum (a number or charge outside the fast forms, no TITLE / PEPMASS, an empty PEPMASS, a header or peak line longer
 *    than 4096 bytes); its columns and values are then placeholders, its slot already has the right size.
 * Malformed text never makes a call fail or write outside a slot.  No host work per line or per peak. ------------------ [dev] */
#define FAL_MGF_FLAG_BYTES 1
#define FAL_MGF_FLAG_LINES 2
#define FAL_MGF_ST_HOST    1
int fal_mgf_index(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t* counts_out);
int fal_mgf_parse(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, int64_t nnz_cap,
                  int64_t* out_indptr, double* out_mz, float* out_intensity, double* precursor_mz, int32_t* charge,
                  int32_t* has_charge, double* retention_time, int64_t* title, int64_t* span, int32_t* status_out);

/* ---- MGF header values by a key table, and byte ranges as fixed-width rows (the library and representative readers; DESIGN.md
 *          "MGF on the device" states the key rule; falcon_amd/ms_io/mgf_io.py holds the host readers they mirror).
 * fal_mgf_parse_ex: fal_mgf_parse with optional_keys, a set of FAL_MGF_OPT_* bits (any other bit: FAL_EINVAL).  FAL_MGF_OPT_TITLE:
 *          a spectrum without TITLE is not HOST on that account, its title range is (0, 0).  fal_mgf_parse is the call with 0.
 * fal_mgf_headers: a third consumer of the index fal_mgf_index left in the context, with fal_mgf_parse's handle check (FAL_EINVAL
 *          for another text, length or spectrum count, and after fal_ctx_trim); it may run before or after fal_mgf_parse.
 *          The table (host): keys u8 back to back with key_ptr i64[n_keys + 1], key k = keys[key_ptr[k], key_ptr[k + 1]); key_kind
 *          i32[n_keys]: FAL_MGF_KEY_SPAN or FAL_MGF_KEY_INT.  1 <= n_keys <= FAL_MGF_MAX_KEYS; a key has 1 to FAL_MGF_MAX_KEY_BYTES
 *          bytes of stripped lower-case printable ASCII without '=', is none of title / pepmass / charge / rtinseconds and
 *          appears once; anything else: FAL_EINVAL, nothing written.
 *          For every spectrum s of the index and every key k, from the spectrum's LAST header line whose key -- what stands before
 *          the first '=', stripped, compared without case -- equals the table's ("SMILES=C=O" has the value "C=O", "NAMES=" is
 *          not "name", "1=2" is a peak line):
 * -> span_out i64[n][n_keys][2]: the stripped value's byte range [from, to) in the text, (0, 0) when absent; value_out
 *    i64[n][n_keys]: for a decided FAL_MGF_KEY_INT key the integer of the fast form [+-]?D{1,18}, else 0; state_out
 *    i32[n][n_keys]: FAL_MGF_KEY_ABSENT, FAL_MGF_KEY_PRESENT (an empty value is present with from == to and the value 0), or
 *    FAL_MGF_KEY_HOST -- the host reads the value from its range: that line is longer than 4096 bytes, or the key is an INT key
 *    and its non-empty value is outside the fast form ("1_0", "1 2", 19 digits, "0x5": Python's int() decides, never a guess).
 *          No synchronisation.  Malformed text never makes the call fail or write outside n * n_keys entries.
 * fal_text_rows: rows_out u8[n][width] (device) = the bytes of range k = span[(k * stride + column) * 2 + {0, 1}] (device, i64:
 *          [from, to) in text u8[n_bytes], which needs no alignment), zero-padded to width, 1 <= width <= FAL_TEXT_MAX_WIDTH;
 *          long_out i32[n] = 1 where the range is longer than width (the row then holds its first width bytes).  A range
 *          outside [0, n_bytes] or with to < from gives a zero row and, behind the launch, FAL_EINVAL; nothing is read outside
 *          the text.  One stream synchronisation.  No host work per line or per row. ----------------------------------- [dev] */
#define FAL_MGF_OPT_TITLE     1
#define FAL_MGF_MAX_KEYS      16
#define FAL_MGF_MAX_KEY_BYTES 32
#define FAL_MGF_KEY_SPAN      0
#define FAL_MGF_KEY_INT       1
#define FAL_MGF_KEY_ABSENT    0
#define FAL_MGF_KEY_PRESENT   1
#define FAL_MGF_KEY_HOST      2
#define FAL_TEXT_MAX_WIDTH    256
int fal_mgf_parse_ex(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, int64_t nnz_cap,
                     int64_t* out_indptr, double* out_mz, float* out_intensity, double* precursor_mz, int32_t* charge,
                     int32_t* has_charge, double* retention_time, int64_t* title, int64_t* span, int32_t* status_out,
                     int optional_keys);
int fal_mgf_headers(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, const uint8_t* keys,
                    const int64_t* key_ptr, const int32_t* key_kind, int n_keys, int64_t* span_out, int64_t* value_out,
                    int32_t* state_out);
int fal_text_rows(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, const int64_t* span, int64_t stride, int64_t column,
                  int64_t n, int width, uint8_t* rows_out, int32_t* long_out);

/* ---- MSP library text -> raw peak CSR + per-entry columns (the device reader; DESIGN.md "MSP on the device" states the grammar;
 *          falcon_amd/ms_io/msp_io.read_annotation_library is the reader it mirrors and the one that decides whatever it leaves
 *          open).  text: as for fal_mgf_index (device, 16-byte aligned, n_bytes < 2^31 - 1; the caller cuts larger files in front
 *          of a Name: line).
 * fal_msp_index: line table, line kinds, per-line peak-segment counts and the entry table (an entry begins at a line whose key is
 *          `name` and ends before the next one) -> counts_out[4] (host) = {entries, peaks of those entries, FAL_MGF_FLAG_* bits,
 *          lines}.  One stream synchronisation.  The flags are fal_mgf_index's.  The tables live in an index handle and scratch
 *          slots of their own: an MGF index and an MSP index of one context stand side by side.
 * fal_msp_parse: fal_mgf_parse's handle check (FAL_EINVAL, nothing written, for another text, length or entry count, and after
 *          fal_ctx_trim).
 * -> out_indptr i64[n + 1] (an entry's count = the peak segments of its lines behind its first `Num Peaks:` line: what stands
 *    before a line's first '"', split at ';', non-empty after stripping), out_mz f64 / out_intensity f32 with room for nnz_cap >=
 *    the indexed peak count (sorted by m/z inside every entry, stable), precursor_mz f64[n] (precursormz, else precursor_mz, else
 *    pepmass: the first whitespace token), charge i32[n] + has_charge i32[n], span i64[n][2]: the entry's bytes from its Name:
 *    line to the next entry's, status i32[n]: 0, or FAL_MSP_ST_HOST -- the host reader decides this entry (a number or charge
 *    outside the fast forms, a Num Peaks value outside D{1,9} or different from the counted peaks, no Num Peaks line, no precursor
 *    key or an empty value, a line longer than 4096 bytes); its columns and values are then placeholders, its slot already has
 *    the right size.
 * fal_msp_headers: fal_mgf_headers over the MSP index: the separator is ':', the lines scanned are the entry's from its Name: line
 *          to its first Num Peaks line (both included), a key may hold any printable ASCII but ':' and upper-case letters
 *          ("num peaks", "db#"), and no key is reserved.  Outputs, states and limits are fal_mgf_headers'.
 * Malformed text never makes a call fail or write outside a slot.  No host work per line or per peak. ------------------ [dev] */
#define FAL_MSP_ST_HOST 1
int fal_msp_index(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t* counts_out);
int fal_msp_parse(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_entries, int64_t nnz_cap,
                  int64_t* out_indptr, double* out_mz, float* out_intensity, double* precursor_mz, int32_t* charge,
                  int32_t* has_charge, int64_t* span, int32_t* status_out);
int fal_msp_headers(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_entries, const uint8_t* keys,
                    const int64_t* key_ptr, const int32_t* key_kind, int n_keys, int64_t* span_out, int64_t* value_out,
                    int32_t* state_out);

/* ---- peak CSR + per-entry columns -> MGF text (the device writer; DESIGN.md "MGF out of the device" states the layout and the
 *          number form; falcon_amd/ms_io/mgf_io.write_spectra is the writer it mirrors: for the same entries the bytes are equal).
 * mz / intensity f32[nnz], indptr i64[n_rows + 1]: the peaks; rows i32[n]: the CSR row whose peaks entry k carries (any order,
 * repeats allowed); precursor_mz f32[n], retention_time f32[n], charge i32[n] (0: no CHARGE line; negative: printed with '-'),
 * cluster i64[n]; title u8[title_bytes] with title_ptr i64[n + 1]: entry k's title bytes [title_ptr[k], title_ptr[k + 1]).
 * Entry k: "BEGIN IONS\nTITLE=<title>\nPEPMASS=<num>\n[CHARGE=<|z|><+ or ->\n]RTINSECONDS=<num>\nCLUSTER=<id>\n", one
 * "<mz> <intensity>\n" per peak, "END IONS\n\n".  <num> of a float32 x: Python's repr(float(x)), at most 23 bytes.
 * fal_mgf_write_sizes -> sizes_out i64[n] (every entry's bytes), offsets_out i64[n + 1] (their exclusive scan, the total last)
 *          and *total_out (host).  One stream synchronisation.  FAL_EINVAL when a row lies outside the CSR or indptr / title_ptr
 *          do not ascend inside their arrays (such an entry counts as one without peaks / title).
 * fal_mgf_write: the text of entries [first, last) into out[0, out_bytes) at offsets[k] - offsets[first] (offsets: the array
 *          fal_mgf_write_sizes filled for the same columns).  out needs no alignment.  FAL_EINVAL, and nothing written, when
 *          out_bytes < offsets[last] - offsets[first]; no byte outside an entry's own range is ever stored, whatever the
 *          offsets hold.  host_out: NULL, or pinned host memory of out_bytes bytes that receives a copy of out before the call's
 *          one stream synchronisation.  No host work per entry or per peak. ----------------------------------------- [dev] */
int fal_mgf_write_sizes(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_rows, int64_t nnz,
                        const int32_t* rows, int64_t n, const float* precursor_mz, const float* retention_time,
                        const int32_t* charge, const int64_t* cluster, const int64_t* title_ptr, int64_t title_bytes,
                        int64_t* sizes_out, int64_t* offsets_out, int64_t* total_out);
int fal_mgf_write(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_rows, int64_t nnz,
                  const int32_t* rows, int64_t n, const float* precursor_mz, const float* retention_time, const int32_t* charge,
                  const int64_t* cluster, const uint8_t* title, const int64_t* title_ptr, int64_t title_bytes,
                  const int64_t* offsets, int64_t first, int64_t last, uint8_t* out, int64_t out_bytes, uint8_t* host_out);

/* ---- the cluster CSV's columns -> the order of its rows and their text (the device writer; DESIGN.md "Cluster CSV out of the
 *          device" states the key order, the number form and the quoting; falcon_amd/falcon.py's sort by _natural_key and its
 *          _write_cluster_info are what it mirrors: for the same rows the order and the bytes are equal).
 * n rows, n < 2^31.  id u8[id_bytes] with id_ptr i64[n + 1]: row r's spectrum id, ASCII bytes [id_ptr[r], id_ptr[r + 1]).
 * fal_csv_order: order_out i32[n] = the rows sorted by (file_rank[r], natural order of the id, r): text runs as byte strings (a
 *          proper prefix first), digit runs as integers of any length, ids that differ only in leading zeros equal -- the stable
 *          sort of the host.  *max_digit_run_out (host): the longest run of digits in an id.  A stable merge sort of the row
 *          indices whose first pass sorts blocks of FAL_CSV_SORT_BLOCK rows.  FAL_EINVAL when id_ptr does not ascend inside the
 *          blob; nothing outside the blob is ever read.  One stream synchronisation, in front of the sort.
 * The text's row k is input row order[k] (order i32[rows]; NULL: row k, rows <= n): "<file name>,<id>,<charge>,<precursor_mz>,
 *          <retention_time>,<cluster>\n" with file_id i32[n] into the names fn u8[fn_bytes] / fn_ptr i64[n_files + 1], charge i32[n]
 *          (0: None), precursor_mz / retention_time f32[n] as str(np.float32(x)) (at most 19 bytes), cluster i64[n]; the two text
 *          fields under csv.QUOTE_MINIMAL (a field with ',', '"' or '\n' -- and '\r' when quote_cr is set -- in quotes, its
 *          quotes doubled).
 * fal_csv_write_sizes -> sizes_out i64[rows], offsets_out i64[rows + 1] (their exclusive scan, the total last) and *total_out
 *          (host).  One stream synchronisation.  FAL_EINVAL when an order entry, a file id or a byte range lies outside its array.
 * fal_csv_write: the text of rows [first, last) into out[0, out_bytes) at offsets[k] - offsets[first].  out needs no alignment.
 *          FAL_EINVAL, and nothing written, when out_bytes < offsets[last] - offsets[first]; no byte outside a row's own range
 *          is ever stored, whatever the offsets hold.  host_out: NULL, or pinned host memory of out_bytes bytes that receives a
 *          copy of out before the call's one stream synchronisation.  No host work per row. ---------------------------- [dev] */
#define FAL_CSV_SORT_BLOCK 1024
int fal_csv_order(fal_ctx* ctx, const int32_t* file_rank, const uint8_t* id, const int64_t* id_ptr, int64_t id_bytes, int64_t n,
                  int32_t* order_out, int64_t* max_digit_run_out);
int fal_csv_write_sizes(fal_ctx* ctx, const int32_t* order, int64_t rows, const int32_t* file_id, const uint8_t* fn, const int64_t* fn_ptr,
                        int64_t n_files, int64_t fn_bytes, const uint8_t* id, const int64_t* id_ptr, int64_t id_bytes,
                        const int32_t* charge, const float* precursor_mz, const float* retention_time, const int64_t* cluster, int64_t n,
                        int quote_cr, int64_t* sizes_out, int64_t* offsets_out, int64_t* total_out);
int fal_csv_write(fal_ctx* ctx, const int32_t* order, int64_t rows, const int32_t* file_id, const uint8_t* fn, const int64_t* fn_ptr,
                  int64_t n_files, int64_t fn_bytes, const uint8_t* id, const int64_t* id_ptr, int64_t id_bytes, const int32_t* charge,
                  const float* precursor_mz, const float* retention_time, const int64_t* cluster, int64_t n, int quote_cr,
                  const int64_t* offsets, int64_t first, int64_t last, uint8_t* out, int64_t out_bytes, uint8_t* host_out);

/* ---- columns -> the text of n units, each a record of fields (the device writer of <out>.network.graphml; DESIGN.md "Records of
 *          fields out of the device" states the field model; falcon_amd/ms_io/graphml_io.py's node_units / edge_units are what it
 *          mirrors: for the same columns the bytes are equal).
 * A unit's text: the head literal, every present field in turn as prefix literal, value, suffix literal, then the tail literal.
 *          Literals are [begin, end) ranges of one blob literals u8[literal_bytes] on the device, literal_bytes <=
 *          FAL_REC_MAX_LITERALS.  fields: n_fields <= FAL_REC_MAX_FIELDS entries in host memory whose pointers are device memory.
 * A field: kind FAL_REC_I32 / I64 / F32 with column i32 / i64 / f32 [rows], or FAL_REC_TEXT with column u8[blob_bytes] and ptr
 *          i64[rows + 1] (row r's bytes [ptr[r], ptr[r + 1])).  index: NULL (unit u reads row u; rows >= n), or i32[n]: unit u reads
 *          row index[u], a negative entry means the field is absent.  A field is also absent when its float32 is not finite or its
 *          text is empty.  Integers are decimal, a float32 is str(np.float32(x)), text is XML character data: & < > become &amp;
 *          &lt; &gt;, '\r' becomes &#13;, '\t', '\n' and every byte from 0x20 up are copied.
 * fal_records_write_sizes -> sizes_out i64[n], offsets_out i64[n + 1] (their exclusive scan, the total last) and *total_out (host).
 *          One stream synchronisation.
 * fal_records_write: the text of units [first, last) into out[0, out_bytes) at offsets[k] - offsets[first].  out needs no
 *          alignment.  FAL_EINVAL, and nothing written, when out_bytes < offsets[last] - offsets[first]; no byte outside a unit's
 *          own range is ever stored, whatever the offsets hold.  host_out: NULL, or pinned host memory of out_bytes bytes that
 *          receives a copy of out before the call's one stream synchronisation.  No host work per unit.
 * FAL_EINVAL also, with nothing read outside an array: an index at or beyond its column's rows, a ptr that does not ascend inside
 *          its blob, a text byte below 0x20 other than '\t', '\n', '\r', more than FAL_REC_MAX_FIELDS fields, a literal range outside
 *          the literal blob.  FAL_EINTERNAL: a unit's text is not the size the sizing call gave. ----------------------- [dev] */
#define FAL_REC_MAX_FIELDS 32
#define FAL_REC_MAX_LITERALS 4096
#define FAL_REC_I32 0
#define FAL_REC_I64 1
#define FAL_REC_F32 2
#define FAL_REC_TEXT 3
typedef struct fal_rec_field {
    const void* column;
    const int64_t* ptr;
    const int32_t* index;
    int64_t rows, blob_bytes;
    int32_t kind;
    int32_t prefix[2], suffix[2];
} fal_rec_field;
int fal_records_write_sizes(fal_ctx* ctx, int64_t n, const fal_rec_field* fields, int n_fields, const uint8_t* literals,
                            int64_t literal_bytes, int head_begin, int head_end, int tail_begin, int tail_end, int64_t* sizes_out,
                            int64_t* offsets_out, int64_t* total_out);
int fal_records_write(fal_ctx* ctx, int64_t n, const fal_rec_field* fields, int n_fields, const uint8_t* literals, int64_t literal_bytes,
                      int head_begin, int head_end, int tail_begin, int tail_end, const int64_t* offsets, int64_t first, int64_t last,
                      uint8_t* out, int64_t out_bytes, uint8_t* host_out);

/* ---- mzML structure -> per-spectrum columns + the tables of fal_decode_peaks (the device reader; DESIGN.md "mzML on the
 *          device" states the grammar; falcon_amd/ms_io/mzml_io.read_chunks is the reader it mirrors and the one that decides
 *          whatever it leaves open).
 * text: u8[n_bytes] on the device, 16-byte aligned, n_bytes < 2^31 - 1 (the caller cuts larger files behind a </spectrum>).
 * fal_mzml_index: tag table ('<' positions), one fixed-size record per tag (kind and form, cvParam accession code, value span,
 *          array length, a not-decided bit) and the spectrum table (<spectrum ...> paired with the next </spectrum>)
 *          -> counts_out[4] (host) = {spectra, tags inside spectra, FAL_MZML_FLAG_* bits, tags}.  One stream synchronisation.
 *          A flag means "this text is the host reader's" (the spectrum count is then 0): STRUCT -- spectrum opens and closes do
 *          not alternate, or an open has no close; MARKUP -- a <!, a <? or a prefixed tag or attribute name anywhere; TAGS --
 *          more tags than one per 4 bytes (the tag table is sized before the count is known).
 * fal_mzml_parse: fills the caller's outputs from the tables of the fal_mzml_index call before it, which stay in scratch slots
 *          of the context (the call checks text, n_bytes and n_spectra against that index and fails with FAL_EINVAL when they
 *          are not its own, or when fal_ctx_trim ran in between).
 * -> status i32[n]: FAL_MZML_ST_OK, FAL_MZML_ST_SKIP (MS1 or no ms level: no spectrum, nothing else of it was read) or
 *    FAL_MZML_ST_HOST (the host reader decides this spectrum from its bytes); id i64[n][2] / span i64[n][2]: byte ranges
 *    [from, to) of the id attribute's value and of the spectrum from its '<' to behind its </spectrum>; precursor_mz f64[n],
 *    charge i32[n] (0: none), retention_time f64[n] (-1 when absent); arrays i64[2n][4]: rows 2s (m/z) and 2s + 1 (intensity)
 *    of spectrum s in fal_decode_peaks' format, their base64 text copied into payload u8[payload_cap] at 8-byte aligned offsets
 *    (gaps zero-filled; payload_cap >= n_bytes + 16 n_spectra always suffices and is required).  The columns and rows of a
 *    spectrum that is not OK are zeros.
 * Malformed text never makes a call fail or write outside a slot.  No host work per spectrum, tag or attribute. --------- [dev] */
#define FAL_MZML_FLAG_STRUCT 1
#define FAL_MZML_FLAG_MARKUP 2
#define FAL_MZML_FLAG_TAGS   4
#define FAL_MZML_ST_OK   0
#define FAL_MZML_ST_SKIP 1
#define FAL_MZML_ST_HOST 2
int fal_mzml_index(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t* counts_out);
int fal_mzml_parse(fal_ctx* ctx, const uint8_t* text, int64_t n_bytes, int64_t n_spectra, uint8_t* payload, int64_t payload_cap,
                   int32_t* status_out, int64_t* id, int64_t* span, double* precursor_mz, int32_t* charge,
                   double* retention_time, int64_t* arrays);

/* ---- consensus representatives: the members of every cluster merged peak by peak (the reference exports medoids only,
 *          falcon.py:198-203; DESIGN.md "Consensus representatives" states the definition).
 * mz / intensity f32, indptr i64[n+1]: the preprocessed peaks in dataset-row order (fewer than 2^31 in all); labels i32[n]:
 * one cluster id in [0, n_clusters) per row (a row with another value belongs to no cluster); medoids i32[n_clusters].
 * Cluster c of m members: m = 1 -> its member's peaks as they are.  Else the members' peaks are pooled in the order (m/z,
 * dataset row, peak index); a group is a maximal run whose neighbours lie within fragment_tol ((double)mz[k] - (double)mz[k-1]
 * > fragment_tol starts a new one: peaks chain); it is kept when min(peaks of the group, m) >= max(1, ceil(min_fraction m))
 * (support counts peaks, not members); a kept group gives m/z = sum(mz * intensity) / sum(intensity) (the plain mean when the
 * intensities sum to 0) and intensity = sum(intensity) / m, float64 sums in pooled order, then L2-normalised over the kept
 * groups in m/z order (all 0 when the norm is 0).  No group kept (or no member): the medoid's peaks as they are,
 * FAL_CONS_ST_FALLBACK.
 * -> out_indptr i64[n_clusters + 1] (always the true sizes), out_mz / out_intensity f32 with room for nnz_cap peaks
 *    (indptr[n] always suffices), status_out i32[n_clusters] of FAL_CONS_ST_* bits.  A cluster whose peaks would end behind
 *    nnz_cap gets FAL_CONS_ST_CAPACITY and writes nothing; the others are complete.  FAL_CONS_ST_GLOBAL marks the clusters
 *    with more than FAL_CONS_LDS_PEAKS pooled peaks, sorted by the device-wide radix sort instead of inside one workgroup:
 *    same bits either way.  One stream synchronisation (the pooled sizes decide the scratch); no per-cluster host work. [dev] */
#define FAL_CONS_LDS_PEAKS 4096
#define FAL_CONS_ST_FALLBACK 1   /* no group reached the quorum: the medoid's peaks */
#define FAL_CONS_ST_GLOBAL   2   /* pooled peaks sorted by the device-wide sort */
#define FAL_CONS_ST_CAPACITY 4   /* nnz_cap too small for this cluster: nothing written for it */
int fal_consensus_spectra(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n,
                          const int32_t* labels, const int32_t* medoids, int64_t n_clusters, double fragment_tol,
                          double min_fraction, int64_t nnz_cap, int64_t* out_indptr, float* out_mz, float* out_intensity,
                          int32_t* status_out);

/* ---- nearest representative: for every query spectrum the library spectrum with the smallest matched-peak cosine distance
 *          among its candidates (DESIGN.md "Assigning to representatives").  Both sides: peaks CSR (mz / intensity f32, indptr
 *          i64[n+1]), precursor m/z f32[n], retention time f32[n] or NULL; one precursor charge; nq, nl < 2^31.
 *          Library row l is a candidate of query q when it passes the per-pair test of fal_filter_neighbors with q in the query
 *          role: diff = f32(pmz_q - pmz_l); Da: |diff| <= tol; ppm: |f32(diff / pmz_l) * 1e6| <= tol; and, with rt_tol >= 0
 *          (negative = none, as fal_filter_neighbors), |f32(rt_q - rt_l)| <= rt_tol.  Only candidates are scored.
 *          d(q, l) = float32(1 - cosine(q's peaks, l's peaks)) with fal_rescore_neighbors' arithmetic, the query first (d = 1
 *          below min_matches or without peaks).  The winner minimises (d, precursor m/z of l, row of l).
 * -> best_row i32[nq] (library row, -1 without a candidate), best_dist f32[nq] (1.0 without one), n_cand i32[nq] (candidates).
 *    A candidate pair whose peaks chain into a component of more than 32 peaks a side fails the call with FAL_EUNSUPPORTED.
 *    nl = 0 is legal (all -1 / 1.0 / 0), nq = 0 a no-op.  One stream synchronisation (error word and solver-pair count;
 *    fal_ctx_counter 9 = the pairs the Hungarian solver finished). ------------------------------------------------- [dev] */
int fal_assign_nearest(fal_ctx* ctx, const float* q_mz, const float* q_intensity, const int64_t* q_indptr,
                       const float* q_precursor_mz, const float* q_rt, int64_t nq, const float* l_mz, const float* l_intensity,
                       const int64_t* l_indptr, const float* l_precursor_mz, const float* l_rt, int64_t nl, double tol,
                       int tol_is_da, double rt_tol, double fragment_tol, int min_matches, int32_t* best_row, float* best_dist,
                       int32_t* n_cand);

/* ---- member scores: every spectrum of a clustered partition scored against the representative of its cluster (DESIGN.md
 *          "Member scores and cluster summary").  mz / intensity f32, indptr i64[n+1]: the partition's peaks by dataset row;
 *          labels i32[n]: cluster c is label value c in [0, n_clusters) (as fal_consensus_spectra takes them; a row with another
 *          value scores 0 with 0 matches).  The representatives are rows of a second peaks CSR (rep_mz / rep_intensity f32,
 *          rep_indptr i64[n_rep+1]): cluster c's is row rep_row[c] (i32[n_clusters]) -- the partition's own CSR with rep_row =
 *          the medoids, or what fal_consensus_spectra returned with rep_row = 0, 1, ...; a rep_row outside [0, n_rep) is a
 *          representative without peaks.
 * -> similarity f32[n]: float32(cosine(member's peaks, representative's peaks)) with fal_rescore_neighbors' arithmetic, the
 *    member first, clipped to [0, 1]; matched i32[n]: the matched peaks.  min_matched_peaks is not applied; a medoid is scored
 *    against itself like any other pair; a side without peaks gives 0 and 0.
 *    A pair whose peaks chain into a component of more than 32 peaks a side fails the call with FAL_EUNSUPPORTED.  n = 0 is a
 *    no-op.  One stream synchronisation (error word and solver-pair count; fal_ctx_counter 9 = the pairs the Hungarian solver
 *    finished, as after fal_assign_nearest). ------------------------------------------------------------------------ [dev] */
int fal_member_scores(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n,
                      const int32_t* labels, int64_t n_clusters, const float* rep_mz, const float* rep_intensity,
                      const int64_t* rep_indptr, int64_t n_rep, const int32_t* rep_row, double fragment_tol, float* similarity,
                      int32_t* matched);

/* ---- cluster summary: the per-cluster columns over a partition's member scores.  labels i32[n] as above; similarity,
 *          precursor_mz f32[n]; retention_time f32[n] or NULL (rt_min / rt_max are 0 then).
 * -> per cluster c in [0, n_clusters): size i32; sim_min f32 and worst_row i32 (the member with sim_min, the lowest row among
 *    equals); sim_mean f64 = (float64 sum of the float32 similarities) / size, summed in the one order DESIGN.md states: the
 *    members in row order, member p added to chain p mod 64, the 64 chain sums added in chain order; pmz_min / pmz_max /
 *    rt_min / rt_max f32.  A cluster without members: zeros, worst_row -1.  No synchronisation. ------------------------- [dev] */
int fal_cluster_summary(fal_ctx* ctx, const int32_t* labels, int64_t n, int64_t n_clusters, const float* similarity,
                        const float* precursor_mz, const float* retention_time, int32_t* size, float* sim_min,
                        int32_t* worst_row, double* sim_mean, float* pmz_min, float* pmz_max, float* rt_min, float* rt_max);

/* ---- representative network: the pairs of `n` nodes whose greedy modified cosine is high (DESIGN.md "Representative
 *          network").  Node v is row rows[v] (i32[n]) of the peaks CSR mz / intensity f32, indptr i64[n_csr_rows + 1] (m/z
 *          ascending inside a row) with precursor m/z precursor_mz[v] (f32[n]); one precursor charge; n < 2^31.
 *          A pair (a, b), a in front of b in (precursor m/z, node index) order, is in scope when
 *          fabs((double)(float)(pmz[b] - pmz[a])) <= max_shift; only pairs in scope are scored.  shift = (float)(pmz[a] - pmz[b]).
 *          Peaks i of a and j of b are a candidate when (double)fabsf(amz[i] - bmz[j]) <= fragment_tol or
 *          (double)fabsf((amz[i] - shift) - bmz[j]) <= fragment_tol (float32 subtractions in this order) and the float32 product
 *          w = ait[i] * bit[j] is > 0.  Candidates are taken by (w descending, i ascending, j ascending) and accepted when
 *          neither peak was accepted before: the greedy modified cosine of GNPS and matchms, NOT the optimal assignment.
 *          score = the float64 sum of the accepted w in ascending i; sim = (float)fmax(0, fmin(score, 1)); matched = the number
 *          accepted.  The pair is an edge when matched >= max(min_matched, 1) and sim >= (float)min_cosine.  top_k > 0: a
 *          node's edges are ranked by (sim descending, other node ascending), an edge stays when its rank is below top_k at both
 *          of its nodes; top_k = 0: no such filter.
 * -> the edges (edge_u i32 < edge_v i32 node indices, edge_sim f32, edge_matched i32; room for max_edges each) in (u, v) order
 *    and *n_edges (host).  The result depends on the arguments alone.  More edges than max_edges: FAL_EINVAL with *n_edges set
 *    (call again with room for them); nothing is written then.  A pair in scope with a side of more than FAL_NET_MAX_PEAKS
 *    peaks fails the call with FAL_EUNSUPPORTED (the same node outside every scope fails nothing); a row outside the CSR, or
 *    of more than 2^24 peaks: FAL_EINVAL.  n = 0 is a no-op.  At most five stream synchronisations: the tile count; the list
 *    and edge counts (again, up to twice, when a list or the edge buffer was too short); with top_k > 0 the kept edges.
 *    fal_ctx_counter 12 = the pairs the greedy kernel finished. --------------------------------------------------------- [dev] */
#define FAL_NET_MAX_PEAKS 4096
int fal_network_edges(fal_ctx* ctx, const float* mz, const float* intensity, const int64_t* indptr, int64_t n_csr_rows,
                      const int32_t* rows, const float* precursor_mz, int64_t n, double fragment_tol, double max_shift,
                      double min_cosine, int min_matched, int top_k, int32_t* edge_u, int32_t* edge_v, float* edge_sim,
                      int32_t* edge_matched, int64_t max_edges, int64_t* n_edges);

/* ---- molecular families: the connected components of `n` nodes under the `m` edges (edge_u, edge_v i32[m], edge_sim f32[m];
 *          fal_network_edges' output is the normal input, any order and duplicates give the same result), broken up until none
 *          has more than max_size nodes (DESIGN.md "Molecular families"; max_size = 0: no cap).  Every edge starts alive.  A
 *          pass takes the components of the alive edges; while one has more than max_size nodes the pass is a cutting round
 *          r = 1, 2, ...: lo = the smallest sim among the alive edges of such a component (float32), and its alive edges with
 *          (double)sim <= (double)lo + delta are cut in round r.  Components within the cap keep their edges.
 * -> node_family i32[n]: the components of two or more nodes numbered 0, 1, ... by their smallest node, -1 for a node without a
 *    surviving edge; node_size i32[n]: the nodes of the node's component (1 for those); edge_round i32[m]: 0 for a surviving
 *    edge, else the round that cut it; *n_families and *n_rounds (host).  The result depends on the arguments alone.  m = 0:
 *    every node -1 / 1.  n = 0 (with m = 0) is a no-op.  FAL_EINVAL, with nothing written and the context usable: an end
 *    outside [0, n), u == v, a sim that is NaN, infinite or negative, max_size < 0, delta negative or NaN.  One stream
 *    synchronisation per pass (*n_rounds + 1 passes: whether a component is above the cap) plus one for the counts.
 *    fal_ctx_counter 13 = the edges cut. -------------------------------------------------------------------------------- [dev] */
int fal_network_families(fal_ctx* ctx, const int32_t* edge_u, const int32_t* edge_v, const float* edge_sim, int64_t m, int64_t n,
                         int max_size, double delta, int32_t* node_family, int32_t* node_size, int32_t* edge_round,
                         int64_t* n_families, int64_t* n_rounds);

/* ---- library search: for each of `nq` queries its best hits among `nl` library spectra, by greedy (modified) cosine (DESIGN.md
 *          "Library search").  Query v is row q_rows[v] (i32[nq]) of the peaks CSR q_mz / q_intensity f32, q_indptr
 *          i64[q_csr_rows + 1] (m/z ascending inside a row) with precursor m/z q_precursor_mz[v] (f32[nq]); library entry w is
 *          row l_rows[w] (i32[nl]) of a second, separate peaks CSR l_* with precursor l_precursor_mz[w]; both sides are of one
 *          precursor charge; nq, nl < 2^31.
 *          A pair (query, library) with precursors pq, pl is in scope when, analog = 0 (exact mode): with diff = (float)(pq - pl),
 *          fabs(tol_is_da ? (double)diff : (double)(diff / pl) * 1e6) <= precursor_tol (fal_assign_nearest's test without a
 *          retention-time rule); analog = 1: fabs((double)(float)(pl - pq)) <= max_shift (fal_network_edges' test).  Only pairs
 *          in scope are scored.  The pair's a is the side with the lower float32 precursor, with equal precursors the query;
 *          shift = analog ? (float)(pmz[a] - pmz[b]) : 0.0f (<= 0).
 *          Peaks i of a and j of b are a candidate when (double)fabsf(amz[i] - bmz[j]) <= fragment_tol or
 *          (double)fabsf((amz[i] - shift) - bmz[j]) <= fragment_tol (float32 subtractions in this order; one test in exact mode)
 *          and the float32 product w = ait[i] * bit[j] is > 0.  Candidates are taken by (w descending, i ascending, j ascending)
 *          and accepted when neither peak was accepted before: the greedy (modified) cosine of GNPS and matchms, NOT the optimal
 *          assignment.  score = the float64 sum of the accepted w in ascending i; sim = (float)fmax(0, fmin(score, 1)); matched
 *          = the number accepted.  The pair is a hit when matched >= max(min_matched, 1) and sim >= (float)min_cosine.  A
 *          query's hits are ranked by (sim descending, library index ascending); top_n > 0: a hit stays when its rank is below
 *          top_n; top_n = 0: every hit stays.  There is no mutual rule.
 * -> the hits (hit_query i32, hit_library i32 indices, hit_sim f32, hit_matched i32; room for max_hits each) in (query, rank)
 *    order and *n_hits (host).  The result depends on the arguments alone.  More hits than max_hits: FAL_EINVAL with *n_hits set
 *    (call again with room for them); nothing is written then.  A pair in scope with a side of more than FAL_NET_MAX_PEAKS
 *    peaks fails the call with FAL_EUNSUPPORTED (the same row outside every scope fails nothing); a row outside its CSR, or of
 *    more than 2^24 peaks: FAL_EINVAL.  nq = 0 or nl = 0 is a no-op with *n_hits = 0.  At most five stream synchronisations: the
 *    tile count; the list and hit counts (again, up to twice, when a list or the hit buffer was too short); with top_n > 0 the
 *    kept hits.  fal_ctx_counter 14 = the pairs the greedy kernels finished. ---------------------------------------------- [dev] */
int fal_library_search(fal_ctx* ctx, const float* q_mz, const float* q_intensity, const int64_t* q_indptr, int64_t q_csr_rows,
                       const int32_t* q_rows, const float* q_precursor_mz, int64_t nq, const float* l_mz, const float* l_intensity,
                       const int64_t* l_indptr, int64_t l_csr_rows, const int32_t* l_rows, const float* l_precursor_mz, int64_t nl,
                       double fragment_tol, double precursor_tol, int tol_is_da, int analog, double max_shift, double min_cosine,
                       int min_matched, int top_n, int32_t* hit_query, int32_t* hit_library, float* hit_sim, int32_t* hit_matched,
                       int64_t max_hits, int64_t* n_hits);

/* ---- annotation propagation: from the annotated nodes of `n` nodes along the `m` undirected links (edge_u, edge_v i32[m], edge_sim
 *          f32[m]; the surviving links of fal_network_families are the normal input, any order and duplicates give the same
 *          result), level by level (DESIGN.md "Annotation propagation").  node_seed i32[n]: >= 0 marks an annotated node (the
 *          value is the caller's and is not interpreted), -1 one that is not.  Level 0: every annotated node has hops 0, source
 *          itself, parent -1, score 1.0f.  Level d = 1 .. max_hops in this order: a link {a, b} with hops[a] == d - 1 and b not
 *          yet reached offers b the candidate (a, c), c = score[a] * sim (one float32 product, not clamped); it counts when
 *          c >= (float)min_score; a node with a counting candidate takes the one of the greatest c, equal c the lowest a, and
 *          has hops d, parent a, source source[a], score c (a zero of either sign is +0).  A node reached at level d is no
 *          parent within level d; levels win over scores.
 * -> node_source, node_hops, node_parent i32[n], node_score f32[n] (a node not reached: -1, -1, -1, 0.0f); *n_reached = the nodes
 *    with hops >= 1, *n_levels = the last level that reached a node (host).  The result depends on the arguments alone.  m = 0:
 *    the annotated nodes at level 0, everything else not reached.  n = 0 (with m = 0) is a no-op.  FAL_EINVAL, with nothing
 *    written and the context usable: an end outside [0, n), u == v, a sim that is NaN, infinite or negative, a seed below -1,
 *    max_hops outside [1, 64], min_score NaN or outside [0, 1].  All levels are enqueued at once (a level behind one that reached
 *    nothing returns at once); one stream synchronisation, for the error word and the counts.  fal_ctx_counter 15 = the nodes
 *    reached. ------------------------------------------------------------------------------------------------------------ [dev] */
int fal_network_propagate(fal_ctx* ctx, const int32_t* edge_u, const int32_t* edge_v, const float* edge_sim, int64_t m, int64_t n,
                          const int32_t* node_seed, int max_hops, double min_score, int32_t* node_source, int32_t* node_hops,
                          int32_t* node_parent, float* node_score, int64_t* n_reached, int64_t* n_levels);

/* ---- sort by precursor m/z (reference cluster.py:73-85 `.sort_values`): stable.
 *          order_out i64[n] (dataset row of sorted position), mz_sorted_out f32[n]. [dev] */
int fal_sort_by_precursor(fal_ctx* ctx, const float* precursor_mz, int64_t n,
                          int64_t* order_out, float* mz_sorted_out);
/* out[i] = src[order[i]] for float arrays (retention times). -------------------- [dev] */
int fal_gather_f32(fal_ctx* ctx, const float* src, const int64_t* order, int64_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* FALCON_HIP_H */
