/*
 * imgrec_knn.h — C ABI of the MI355X exact k-NN index (the image_recommender hot path).
 *
 * This is the drop-in boundary for the faiss calls the reference makes on its search/index path
 * (SURVEY.md §8b).  Every entry point below replaces one faiss call site of the reference:
 *
 *   knn_create(d, KNN_METRIC_L2, ...)   faiss.IndexFlatL2(d) — the parity target named by north_star; the
 *                                        reference default IndexIVFPQ(IndexHNSWFlat(d,32),d,2048,m,12) is
 *                                        built at /root/reference/main/create_index.py:218-228
 *   knn_train                            index.train(train_vecs)       main/create_index.py:296-299
 *   knn_add / knn_add_device             index.add(arr)                main/create_index.py:311
 *   knn_search / knn_search_device       index.search(query_vec, k)    main/search_from_image.py:247,
 *                                                                      Analytics/rt_Search.py:63
 *   knn_range_search / _device           index.range_search(x, thresh) (every faiss flat index; the
 *                                                                      near-duplicate query)
 *   knn_ntotal / knn_dim                 index.ntotal / index.d        main/search_from_image.py:340,
 *                                                                      main/create_index.py:321
 *   knn_write                            faiss.write_index(index, f)   main/create_index.py:320
 *   knn_read                             faiss.read_index(f)           main/search_from_image.py:339
 *   knn_normalize_L2                     faiss.normalize_L2(x)         main/search_from_image.py:322
 *   knn_merge_device                     (new) per-shard top-k merge after the RCCL all-gather (§8e)
 *   knn_packed_bytes / knn_merge_packed_device  (new) the same over one packed key|label buffer,
 *                                        so the all-gather is a single collective
 *   knn_create_multi / knn_read_multi    (new) one index over several devices of one process, so
 *                                        the reference's single-process CLI
 *                                        (main/search_from_image.py:430-441) can use every GPU
 *
 * Conventions
 *   - All functions return 0 on success and a negative KNN_E* code on failure; the message of the
 *     last failure on the calling thread is returned by knn_last_error().
 *   - Host-pointer functions (knn_add, knn_search, knn_write, ...) synchronise before returning.
 *     *_device functions take device pointers and a hipStream_t (passed as void*; NULL = the
 *     HIP null stream, like any HIP API), enqueue asynchronously and never wait for the GPU: the
 *     candidate paths' certificate, its second chance and the exact re-run of the queries it
 *     cannot settle are all decided on the device.  They allocate only when the workspace must
 *     grow.
 *   - Operations on one index may come from different streams and threads: an operation on
 *     another stream than the previous operation's first waits for that operation (an add on
 *     stream A is complete before a search on stream B reads the rows; two searches never share
 *     the workspace concurrently).  A call on the index's host entry points is ordered after
 *     earlier device-stream calls the same way.  By default (KNN_FENCE_EAGER) every *_device call
 *     records an event on its stream as its last step and the next call on another stream waits
 *     for it, so a stream may be destroyed as soon as the call returns.  knn_set_fence_mode
 *     (KNN_FENCE_LAZY) records the event only when the stream changes: one stream used back to
 *     back then records none (~6 us of GPU time per call saved on MI355X), but the previous
 *     call's stream must stay valid until the next call on the index, and the wait then also
 *     covers work the caller queued on that stream in between.  A call that fails keeps this
 *     order too: what it had enqueued is waited for like a successful call's, and a failing
 *     host-pointer call returns with no copy into the caller's arrays still in flight.
 *   - Vectors are row-major float32, n rows × d.  Labels are int64.  Result rows are sorted by
 *     ascending distance (L2) or descending inner product (IP/COSINE); exact ties are broken by the
 *     smaller label.  When fewer than k vectors exist, the tail of a result row holds label -1 and
 *     distance FLT_MAX (L2) or -FLT_MAX (IP/COSINE), as faiss's heaps do.
 *   - L2 distances are squared L2, evaluated as (|q|^2 + |x|^2) - 2 q.x and clamped at 0, as in
 *     faiss's exhaustive_L2sqr_blas.
 */
#ifndef IMGREC_KNN_H
#define IMGREC_KNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct knn_index knn_index_t;

enum knn_metric {
    KNN_METRIC_IP = 0,     /* faiss METRIC_INNER_PRODUCT (IndexFlatIP) */
    KNN_METRIC_L2 = 1,     /* faiss METRIC_L2 (IndexFlatL2) */
    KNN_METRIC_COSINE = 2  /* rows and queries L2-normalised on entry, then IP */
};

enum knn_error {
    KNN_OK = 0,
    KNN_EINVAL = -1,   /* bad argument (d <= 0, k <= 0, NULL pointer, unsupported k, ...) */
    KNN_EHIP = -2,     /* HIP runtime error */
    KNN_ENOMEM = -3,   /* device allocation failed */
    KNN_EIO = -4,      /* file could not be read/written or has a bad layout */
    KNN_ENOSYS = -5    /* not supported (e.g. no GPU visible) */
};

/* Search arithmetic.  Every mode returns the exact search's result up to the fp32 tie window:
 * a candidate pass proposes K' rows per query, an fp32 rerank computes their exact keys and a
 * per-query error-bound certificate proves that no row outside the candidates can rank before a
 * returned one.  The returned labels are those of the fp32 keys of the rerank.  Tie windows, as
 * tested (tests/knn_check.py):
 *   - rigorous (every parity test): every returned distance is within the worst-case fp32 bound
 *     gamma_D (|q|^2 + |x|^2 + 2 sum|q_i x_i|) + rounding of the norm terms (gamma_D = D u /
 *     (1 - D u), u = 2^-24: about 1e-4 relative at D = 1968) of its row's exact distance, and
 *     labels equal the float64 oracle's at every rank separated from both neighbours by twice it;
 *   - empirical (check_knn_tight: the full-size configs 2-4 and the int8 path at d >= 1024):
 *     labels equal BOTH the float64 oracle's and faiss IndexFlatL2's fp32 result (its
 *     exhaustive_L2sqr_blas restated, oracle.flat_knn.search_blas_fp32_blocked) at every rank
 *     separated from both neighbours by more than w = max(8 x the measured max |fp32 key -
 *     float64 key| of both, 1e-6 x the query's key scale) — about 1e-6 relative on the bench
 *     data — and the top-k label SETS are equal wherever the k-th / (k+1)-th gap exceeds w; at
 *     least 95 % of ranks are so checked at the full-size configurations.
 * Inside the window modes may order near-equal rows differently.  A query whose certificate fails gets a second chance (every
 * per-split list entry reranked, certified against the list floor); if that fails too it is
 * re-run on the exact fp32 kernel, planned on the device.
 * AUTO: the bf16 path (d >= 64; one bf16 MFMA per product, K' = 64) for every batch at every
 *       corpus size (large batches: bf16 MFMA; small ones: the bf16 copy streams half the
 *       bytes; small corpora: the exact kernel's latency floor of ~0.16 ms per search); the
 *       split path when bf16 is unavailable and the batch is large; everything else (d < 64,
 *       k > KNN_MAX_K) the exact fp32 kernel.
 *       Batches of <= 8 queries (the reference CLI's one-query searches) take the int8 path
 *       instead (64 <= d <= 4096; at d <= 512, where an int8 row's 1-KiB group is wider than
 *       its bf16 row, only while the int8 copy is <= 64 MB): a block-scaled int8 copy of the rows (one fp32 scale per 64
 *       elements, about half the bf16 copy's bytes, built on the first such search), a
 *       two-level int8 query and exact int32 dot4 products, K' = 64, the same certificate with
 *       the int8 copy's and the query's residual bounds (csrc/knn_i8.hip).
 * EXACT: always the fp32 kernel.  SPLIT: the split path (bf16 hi/lo, three MFMAs per product,
 *       K' = 16/32) whenever k <= 16 and d >= 256.  BF16: the bf16 path for every batch (tests).
 * I8:   the int8 path for batches of <= 8 queries (64 <= d <= 4096; tests), else as AUTO. */
enum knn_search_mode {
    KNN_SEARCH_AUTO = 0,
    KNN_SEARCH_EXACT = 1,
    KNN_SEARCH_SPLIT = 2,
    KNN_SEARCH_BF16 = 3,
    KNN_SEARCH_I8 = 4
};

/* Largest k the fused top-k kernels serve (they keep per-lane lists of this length). */
#define KNN_MAX_K 32
/* Every k >= 1 is served (faiss IndexFlat's range; past ntotal the tail is label -1, distance
 * +-FLT_MAX).  KNN_MAX_K < k <= KNN_MAX_K_LARGE runs the exact fp32 fused kernel with 32-entry
 * lists, the k best of their union by an exact per-query radix select, certified against the
 * lists' floor; the queries the certificate cannot settle are re-run by an exact corpus scan whose
 * fixed grid walks the failed queries the device counted (csrc/knn_largek.hip: no key block
 * reaches HBM, the host never waits).  k > KNN_MAX_K_LARGE keys every (query, row) pair in fp32
 * and sorts each query's keys (csrc/knn_hugek.hip: coverage of faiss's k range, not a fast path).
 * Merges of k-lists (multi-device shards, knn_merge_*_device) use the in-LDS select up to 8192
 * gathered entries per query and the sort beyond. */
#define KNN_MAX_K_LARGE 1024

/* Create an empty index of dimension d on HIP device `device` (-1 = current device). */
int knn_create(int d, int metric, int device, knn_index_t** out);
/* Create an empty index whose rows are split over ndev devices (entries may repeat: several
 * shards on one device).  Every add is cut into ndev contiguous pieces, one per shard; labels are
 * the dense row offsets as for one device.  A search runs all shards concurrently (each on its own
 * device and stream) and merges their top-k on devices[0]; *_device pointers live on devices[0].
 * Every other entry point works unchanged on the returned handle. */
int knn_create_multi(int d, int metric, const int* devices, int ndev, knn_index_t** out);
/* Row shards of an index (1 for knn_create). */
int knn_num_shards(const knn_index_t* index);
int knn_free(knn_index_t* index);

int knn_dim(const knn_index_t* index);
int knn_metric(const knn_index_t* index);
int64_t knn_ntotal(const knn_index_t* index);
int knn_is_trained(const knn_index_t* index);

/* Labels returned by search are (row offset + id_offset); a row shard sets its global base here. */
int knn_set_id_offset(knn_index_t* index, int64_t id_offset);

/* Flat index: training only marks the index trained (faiss IndexFlat is always trained). */
int knn_train(knn_index_t* index, const float* x, int64_t n);

/* Append n rows; ids are implicitly ntotal .. ntotal+n-1 (faiss Index::add). */
int knn_add(knn_index_t* index, const float* x_host, int64_t n);
int knn_add_device(knn_index_t* index, const float* x_dev, int64_t n, void* stream);
/* Pre-size the corpus buffer for n rows (avoids regrowth copies during streamed adds). */
int knn_reserve(knn_index_t* index, int64_t n);
int knn_reset(knn_index_t* index);

/* faiss Index::remove_ids on a bitmap over the stored rows (knn_search_filtered's layout and rules:
 * row i is removed iff i < nbits and bit i is set; bits at or past ntotal are ignored).  Survivors keep
 * their order; labels become dense again (row offset + id_offset).  Host bitmap; waits.
 *   - In place (csrc/knn_remove.hip): the fp32 rows, the norms and every derived copy that exists
 *     (bf16, split, int8) are compacted by moving row bytes through a bounded bounce buffer (the
 *     64 MB add staging), so no copy is re-derived and memory does not grow with ntotal; the state
 *     afterwards is the one the same adds without the removed rows would have left.
 *   - *nremoved (may be NULL) receives the number of rows removed.  An empty index, nbits = 0 or no
 *     set bit remove nothing and return KNN_OK; removing every row leaves a usable empty index.
 *   - KNN_EINVAL for a NULL index, nbits < 0, and a NULL bitmap with nbits > 0.
 *   - Exclusive, like knn_add: ordered after earlier operations on any stream.
 *   - A multi-device index: the bitmap addresses global rows; every shard compacts its own rows, so
 *     shards may afterwards hold different numbers of rows (later adds are still cut evenly). */
int knn_remove_ids(knn_index_t* index, const uint8_t* bitmap_host, int64_t nbits, int64_t* nremoved);

/* Copy rows [i0, i0+n) back to the host as stored (normalised for COSINE). */
int knn_reconstruct_n(const knn_index_t* index, int64_t i0, int64_t n, float* x_host);

/* k nearest neighbours of nq queries.  D, I: nq*k, row-major. */
int knn_search(knn_index_t* index, const float* q_host, int64_t nq, int k,
               float* D_host, int64_t* I_host);
int knn_search_device(knn_index_t* index, const float* q_dev, int64_t nq, int k,
                      float* D_dev, int64_t* I_dev, void* stream);

/* Range search (faiss Index::range_search): every stored row within a radius of each query.
 *   - L2: the rows whose fp32 key (|q|^2 + |x|^2) - 2 q.x, clamped at 0, is < radius (squared L2,
 *     as knn_search returns it).  IP / COSINE: the rows with q.x > radius (cosine normalises rows
 *     and queries on entry, as knn_search does); D holds the inner product.  Both comparisons are
 *     strict, as in faiss.  A pair whose key is NaN is never returned.
 *   - Layout, as faiss's RangeSearchResult: lims is int64[nq + 1] with lims[0] = 0; query i's hits
 *     are D[lims[i] .. lims[i + 1]) (float32) and I[lims[i] .. lims[i + 1]) (int64, row offset +
 *     id_offset).
 *   - Order (faiss leaves it unspecified): knn_search's — best first, exact ties by the smaller
 *     label.  The output is deterministic, and its first k entries are a valid top-k.
 *   - Arithmetic: exact fp32, no candidate pass and no certificate.  A pair's key depends on
 *     (q, x, d, metric) only — not on ntotal, nq, the query's place in the batch or the row
 *     sharding — so the same pair gets the same bits from any call (it need not equal the bits
 *     knn_search returns for the pair: that kernel's summation order depends on its launch plan).
 *   - nq = 0 gives lims = {0}; an empty index, or L2 with radius <= 0, gives all-zero lims;
 *     radius = +inf (L2) / -inf (IP) returns every stored row for every query.  A NaN radius is
 *     KNN_EINVAL.  So is a shard of 2^32 rows or more, and a chunk of 8192 queries with 2^32 hits
 *     or more ("lower the radius or split the batch"): entries pack a 32-bit row beside the key.
 * The result object owns device buffers on the index's device (devices[0] of a multi-device
 * index, which searches its shards concurrently and merges per query into the same order). */
typedef struct knn_range_result knn_range_result_t;
/* faiss Index::range_search.  Host queries; waits; result buffers live on the index's device. */
int knn_range_search(knn_index_t* index, const float* q_host, int64_t nq, float radius,
                     knn_range_result_t** out);
/* Device queries on `stream`.  Unlike the other *_device calls this one waits once on the stream
 * (per chunk of 8192 queries): the result size must reach the host before the result can be
 * allocated.  The last kernels may still run when it returns; knn_range_copy and
 * knn_range_device wait for them. */
int knn_range_search_device(knn_index_t* index, const float* q_dev, int64_t nq, float radius,
                            void* stream, knn_range_result_t** out);
int64_t knn_range_nq(const knn_range_result_t* result);
int64_t knn_range_size(const knn_range_result_t* result);     /* = lims[nq] */
/* Host copies; any pointer may be NULL. */
int knn_range_copy(const knn_range_result_t* result, int64_t* lims, float* D, int64_t* I);
/* Device pointers, valid until knn_range_free (D and I are never NULL; an empty result's hold one
 * unused element). */
int knn_range_device(const knn_range_result_t* result, const int64_t** lims, const float** D,
                     const int64_t** I);
int knn_range_free(knn_range_result_t* result);

/* Filtered search (faiss SearchParameters::sel): the k nearest rows among the rows a bitmap selects.
 *   - Bitmap: faiss IDSelectorBitmap's layout.  Stored row i (label i + id_offset) is selected iff
 *     i < nbits and (bitmap[i >> 3] >> (i & 7)) & 1.  The bitmap holds ceil(nbits / 8) bytes; rows
 *     at or past nbits are unselected, bits at or past ntotal are ignored.  One bitmap serves every
 *     query of the call.  For a multi-device index it addresses global rows and, in the device
 *     form, lives on devices[0].
 *   - Result: knn_search's in every respect except the candidate set: nq * k, best first, exact
 *     ties by the smaller label.  When fewer than k rows are selected the tail holds label -1 and
 *     +-FLT_MAX (zero selected, an empty index and nbits = 0 included).  A pair whose key is NaN
 *     is never returned.
 *   - Arithmetic: exact fp32, no candidate pass and no certificate.  A pair's key is the bits
 *     knn_range_search returns for it (the same MFMA, the same depth order, chosen from the row
 *     stride alone, the same fmaf(-2, q.x, |q|^2 + |x|^2) clamped at 0), so a result does not
 *     depend on ntotal, the batch, the mask's other bits, the order of adds or the sharding.
 *   - Cost: the rows are compacted into a list once per call (work proportional to ntotal bits)
 *     and the distance kernel walks that list: its work follows the number of selected rows.
 *   - Errors: KNN_EINVAL for k <= 0, nbits < 0, a NULL bitmap with nbits > 0, NULL queries or
 *     outputs with nq > 0, and a shard of 2^32 rows or more.
 *   - Waiting: the host form synchronises before it returns.  The device form enqueues on
 *     `stream` and never waits for the GPU while k <= KNN_MAX_K (the selected count stays on the
 *     device); stream ordering and fences are those of knn_search_device.  For k > KNN_MAX_K
 *     (every selected pair's key, one segmented sort: coverage of faiss's k range, not a fast path)
 *     the selected count must reach the host to size the sort: that route waits once per call on
 *     the stream (a multi-device index: once per shard).
 *   - Reports: knn_set_timing / knn_kernel_time cover the gathered tile kernel; knn_last_path
 *     reports 0 after a filtered search. */
int knn_search_filtered(knn_index_t* index, const float* q_host, int64_t nq, int k,
                        const uint8_t* bitmap_host, int64_t nbits, float* D_host, int64_t* I_host);
int knn_search_filtered_device(knn_index_t* index, const float* q_dev, int64_t nq, int k,
                               const uint8_t* bitmap_dev, int64_t nbits, float* D_dev,
                               int64_t* I_dev, void* stream);

/* Merge nlists candidate lists per query into the top k.  cand_D/cand_I are laid out
 * [nlists][nq][kin] (the layout of an all-gather of per-shard [nq][kin] results); entries with
 * label -1 are ignored.  Output nq*k, same ordering/padding rules as knn_search: the k best by
 * (key, label), keys compared as floats (-0.0 ties +0.0, the smaller label first), then label -1
 * and +-FLT_MAX.
 * Labels: k <= KNN_MAX_K carries any non-negative int64.  For k > KNN_MAX_K every label must lie
 * in [0, 2^32): those kernels pack a label into 32 bits beside its key, and a larger one comes
 * back without its upper bits.  The device cannot refuse without a host read, so the callers that
 * know their label range do: a multi-device index returns KNN_EINVAL for a k > KNN_MAX_K search
 * when ntotal + id_offset > 2^32, ShardedIndex.search raises when ntotal_global > 2^32. */
int knn_merge_device(const float* cand_D, const int64_t* cand_I, int nlists, int64_t nq, int kin,
                     int k, int metric, float* D_dev, int64_t* I_dev, void* stream);

/* Packed per-shard results: one chunk of knn_packed_bytes(nq, k) bytes per shard holding the nq*k
 * float keys (padded to an even count), then the nq*k int64 labels (8-byte aligned).  A shard
 * searches straight into its chunk (D = chunk, I = chunk + 4 * (nq*k rounded up to even)); one
 * all-gather of the chunks gives knn_merge_packed_device its [nlists] chunks.  The padding float
 * is never read.  Order, padding and the label contract are knn_merge_device's: any non-negative
 * int64 label for k <= KNN_MAX_K, labels in [0, 2^32) for k > KNN_MAX_K. */
int64_t knn_packed_bytes(int64_t nq, int k);
int knn_merge_packed_device(const void* packed, int nlists, int64_t nq, int kin, int k, int metric,
                            float* D_dev, int64_t* I_dev, void* stream);

/* faiss IndexFlat on-disk layout ("IxF2" for L2, "IxFI" for IP/COSINE). */
int knn_write(const knn_index_t* index, const char* path);
int knn_read(const char* path, int device, knn_index_t** out);
int knn_read_multi(const char* path, const int* devices, int ndev, knn_index_t** out);

/* In-place row normalisation of a host array (faiss.normalize_L2: rows with norm 0 unchanged). */
int knn_normalize_L2(float* x_host, int64_t n, int d);

/* Kernel timing for the live roofline figure in bench.py.  While enabled, every search records a
 * HIP event pair around its fused distance+top-k launch, on the stream that launch uses.
 * knn_kernel_time waits for the recorded events, returns the summed duration (ms) and launch
 * count since the last call, and clears them. */
int knn_set_timing(knn_index_t* index, int enable);

/* Cross-stream fence of the *_device entry points (Conventions above). */
enum knn_fence_mode { KNN_FENCE_EAGER = 0, KNN_FENCE_LAZY = 1 };
int knn_set_fence_mode(knn_index_t* index, int mode);
int knn_kernel_time(knn_index_t* index, double* total_ms, int* launches);

int knn_set_search_mode(knn_index_t* index, int mode);
/* Queries of the last search that took a candidate path (split or bf16), how many of them were
 * re-run on the exact kernel because neither certificate held, and (may be NULL) the largest
 * observed |approximate key - fp32 key| / (error bound of both) over all reranked candidates:
 * <= 1 whenever the certificate's bounds hold, in practice far below.  Waits for that search.
 * knn_search_stats2 also returns the queries whose first certificate failed and whose second
 * chance certified them (may be NULL).  A multi-device index sums re-runs over its shards. */
int knn_search_stats(knn_index_t* index, int64_t* split_queries, int64_t* fallback_queries,
                     float* max_err_ratio);
int knn_search_stats2(knn_index_t* index, int64_t* split_queries, int64_t* fallback_queries,
                      int64_t* second_chance_queries, float* max_err_ratio);

/* Arithmetic the last search's first query chunk ran: 0 = exact fp32 kernel, 1 = split path,
 * 2 = bf16 path, 3 = int8 path (the candidate paths' fallbacks are counted by knn_search_stats). */
int knn_last_path(const knn_index_t* index);

/* Queries of the last k > KNN_MAX_K search that its certificate could not settle from the fused
 * kernel's 32-entry lists and that were re-run by the exact corpus scan (csrc/knn_largek.hip);
 * summed over the shards of a multi-device index. */
int knn_large_k_fallbacks(const knn_index_t* index, int64_t* queries);

/* Launch geometry chosen for a search of nq queries (for reports): workgroup tile rows/queries,
 * row splits and workgroup count. */
int knn_plan(const knn_index_t* index, int64_t nq, int k, int* tile_rows, int* tile_queries,
             int* splits, int* workgroups);

/* Name of the fused candidate/distance kernel a search of nq queries launches, as profilers print
 * it (e.g. "knn_b16w_tile_kernel<10, 1, true>"), NUL-terminated into name[cap].  Whether a large
 * batch runs the int8-tail sibling ("knn_b16w_tile_kernel_i8t<...>") is decided from the corpus by
 * the first such search (it builds the copy and judges its own certificate counts): before that
 * search this reports the bf16 kernel, after it the kernel that later searches run. */
int knn_plan_kernel(const knn_index_t* index, int64_t nq, int k, char* name, int cap);

/* Read-only view of the int8 tail copy of the 256 x 256 candidate kernel, for tests (NULL outputs
 * are skipped): the split column `head` and the codes per row `dpt`, and rows [i0, i0 + n) of the
 * codes (n x dpt int8), the scales (n floats) and the per-row statistics (n x 4 floats: tail
 * residual, head residual, tail norm, head norm, each rounded up).  KNN_EINVAL while the copy does
 * not exist (no search has taken the route yet, or the index is not eligible). */
int knn_debug_i8tail(knn_index_t* index, int* head, int* dpt, int64_t i0, int64_t n, int8_t* codes,
                     float* scales, float* stats);
/* The same copy's raw rows, read-only, for tests (NULL outputs are skipped).  The copy stores one
 * joint row per corpus row: its dpt tail codes, then its first `head` columns as bf16 (the values of
 * the bf16 rows), *row_bytes = dpt + 2 head bytes in all; rows [i0, i0 + n) of them go to `rows`
 * (n x row_bytes).  KNN_EINVAL while the copy does not exist. */
int knn_debug_i8tail_rows(knn_index_t* index, int64_t i0, int64_t n, int* row_bytes, uint8_t* rows);

const char* knn_last_error(void);
const char* knn_version(void);

#ifdef __cplusplus
}
#endif

#endif /* IMGREC_KNN_H */
