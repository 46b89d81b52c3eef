// knn_multi.h — one k-NN index over several HIP devices in one process (knn_create_multi):
// the corpus is split into per-device row shards, a search runs every shard concurrently on its
// own device and stream and merges the per-shard top-k on the first device.  Internal to the C
// ABI (knn_capi.cpp dispatches here when knn_index::multi is set).
#pragma once

#include "knn_index.h"

namespace imgrec {

int multi_create(int d, int metric, const int* devices, int ndev, knn_index** out);
int multi_free(knn_index* ix);
int multi_reserve(knn_index* ix, int64_t n);
int multi_add(knn_index* ix, const float* x, int64_t n);
int multi_add_device(knn_index* ix, const float* x, int64_t n, hipStream_t st);
int multi_reset(knn_index* ix);
int multi_reconstruct_n(knn_index* ix, int64_t i0, int64_t n, float* x);
int multi_search(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I);
int multi_search_device(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                        hipStream_t st);
// range search over every shard concurrently, merged per query on the host into the (key, label)
// order; q on the host (q_on_host; `st` unused) or on the first device, ready on `st`
int multi_range_search(knn_index* ix, const float* q, bool q_on_host, int64_t nq, float radius,
                       hipStream_t st, knn_range_result** out);
// filtered search: the bitmap (global rows; on the host with q when q_on_host, else on the first
// device, ready on `st`) reaches every shard's device, every shard compacts it through its local ->
// global map and searches concurrently; merged as multi_search merges
int multi_search_filtered(knn_index* ix, const float* q, bool q_on_host, int64_t nq, int k,
                          const uint8_t* bitmap, int64_t nbits, float* D, int64_t* I, hipStream_t st);
// remove_ids: the host bitmap addresses global rows; every shard compacts its own rows and its label
// map through that map, the surviving labels are renumbered densely and the runs rebuilt.  Shards
// may end up holding different numbers of rows.  Waits.
int multi_remove_ids(knn_index* ix, const uint8_t* bitmap, int64_t nbits, int64_t* nremoved);
int multi_set_metric(knn_index* ix, int metric);
int multi_set_trained(knn_index* ix, bool trained);
int multi_set_timing(knn_index* ix, int enable);
int multi_kernel_time(knn_index* ix, double* total_ms, int* launches);
int multi_set_search_mode(knn_index* ix, int mode);
int multi_set_fence_mode(knn_index* ix, int mode);
int multi_search_stats(knn_index* ix, int64_t* split_q, int64_t* fallback_q, int64_t* second_q,
                       float* ratio);
int multi_last_path(const knn_index* ix);
const knn_index* multi_shard(const knn_index* ix, int s);
int multi_num_shards(const knn_index* ix);

}  // namespace imgrec
