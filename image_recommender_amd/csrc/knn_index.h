// knn_index.h — internal state of one k-NN index and the helpers the C-ABI translation units
// share (knn_capi.cpp: entry points; knn_plan.h / knn_plan.cpp: the HIP-free route choice, launch
// geometry and error-bound coefficients; knn_search.cpp: the search paths; knn_io.cpp: the faiss
// file layout; knn_multi.cpp: one index over several devices; knn_range.hip: range search;
// knn_filter.hip: filtered search; knn_remove.hip: remove_ids).  Not part of the public ABI
// (include/imgrec_knn.h).
//
// Ownership: every device or page-locked allocation the index keeps is a DevBuf / PinBuf member
// (dev_buf.h over the two memory spaces below), released by the index's destructor; there is no
// free list to keep in step.  The per-row corpus arrays are listed once, by corpus_columns().
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "dev_buf.h"
#include "knn_kernels.h"
#include "knn_plan.h"      // (and with it include/imgrec_knn.h)
#include "stream_fence.h"

namespace imgrec {

void set_err(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// the value of a test / A-B environment knob, logged once on stderr when set (knn_capi.cpp)
const char* test_knob(const char* name);

#define KNN_FAIL(code, ...)              \
    do {                                 \
        ::imgrec::set_err(__VA_ARGS__);  \
        return (code);                   \
    } while (0)

#define KNN_HIP(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            ::imgrec::set_err("%s failed: %s", #expr, hipGetErrorString(e_));          \
            return e_ == hipErrorOutOfMemory ? KNN_ENOMEM : KNN_EHIP;                  \
        }                                                                              \
    } while (0)

struct DeviceGuard {
    int old = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&old) != hipSuccess) old = -1;
        if (dev >= 0 && dev != old) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (old >= 0 && hipGetDevice(&cur) == hipSuccess && cur != old) (void)hipSetDevice(old);
    }
};

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// The two memory spaces of dev_buf.h: device memory (regrowth reserves half as much again) and
// page-locked host memory (exact sizes).  The only callers of hipFree / hipHostFree.
inline int hip_result(hipError_t e, const char* call) {
    if (e == hipSuccess) return KNN_OK;
    set_err("%s failed: %s", call, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? KNN_ENOMEM : KNN_EHIP;
}
struct DeviceSpace {
    static constexpr bool kSlack = true;
    static int alloc(void** p, size_t bytes) {
        return hip_result(hipMalloc(p, bytes), "hipMalloc((void**)p, n * sizeof(T))");
    }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedSpace {
    static constexpr bool kSlack = false;
    static int alloc(void** p, size_t bytes) {
        return hip_result(hipHostMalloc(p, bytes, hipHostMallocDefault),
                            "hipHostMalloc(p, need_bytes, hipHostMallocDefault)");
    }
    static void free(void* p) { (void)hipHostFree(p); }
};
template <typename T> using DevBuf = Buf<T, DeviceSpace>;
template <typename T> using PinBuf = Buf<T, PinnedSpace>;
// The stream API of stream_fence.h.
struct HipStreams {
    using Stream = hipStream_t;
    using Event = hipEvent_t;
    using DeviceScope = DeviceGuard;      // (declared above: the device set, then restored)
    static int create_event(Event* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
    static void destroy_event(Event e) { (void)hipEventDestroy(e); }
    static int record(Event e, Stream s) { return hipEventRecord(e, s); }
    static int wait(Stream s, Event e) { return hipStreamWaitEvent(s, e, 0); }
    static int sync_stream(Stream s) { return hipStreamSynchronize(s); }
    static int sync_device() { return hipDeviceSynchronize(); }
    static void clear_error() { (void)hipGetLastError(); }
    static int fail(int e, const char* call) { return hip_result((hipError_t)e, call); }
};

}  // namespace imgrec

using imgrec::DevBuf;
using imgrec::PinBuf;

// (IndexShape, knn_plan.h: d, dp, dpb, nblk8, cus, metric, mode, ntotal, ... — what choose_route reads)
struct knn_index : imgrec::IndexShape {
    int device = 0;
    // launch knob read from the environment at creation (A/B and tests): the merge's second level
    // inside the rerank (IMGREC_MERGE_FUSE=0: off)
    bool merge_fuse = true;
    bool chance_skip = true;    // IMGREC_CHANCE_SKIP=0: every query takes the first rerank
    // int8 batches of at most this many queries skip the merge and the first rerank: the
    // certificate tail's second chance answers every query (RerankArgs::direct);
    // IMGREC_CHANCE_DIRECT=N sets it, 0 = off.  4: two queries 10 / 5.5 us faster at config 2 / 3,
    // four queries 9-18 us faster at config 2 and the same at config 3
    // (profiles/r05/nq1/direct_nq24/)
    int chance_direct_max = 4;
    // ... over the scan's lane lists unfolded: 1 = while <= 4096 per query, 2 = always, 0 = never
    // (IMGREC_DIRECT_RAW)
    int direct_raw = 1;
    // int8 scan at two workgroups per CU: every K-th round the second-dispatched half's groups go
    // to the first half (I8Args::half_k; IMGREC_I8_HALF_K=K, 0 = even split).  12: config 2 one
    // query 0.1517 -> 0.1503 ms; 6-8 and 24-32 measured worse (profiles/r05/nq1/half_k/)
    int i8_half_k = 12;
    // int8 scan: the last i8_pool64 / 64 of the row groups handed out at run time in chunks of
    // 4 i8_pool_ch groups (I8Args::pool).  Default: one query on one workgroup per CU (rows of
    // >= 24 blocks), where 4/64 in chunks of 8 groups took the config-3 search from 0.3258 to
    // 0.3210 ms; config 2's two workgroups per CU lost 4-30 us with any pool (profiles/r06/i8_pool/).
    // IMGREC_I8_POOL=<64ths> (0 = off) applies it to every one- or two-query scan with lists of 16.
    int i8_pool64 = 4;
    int i8_pool_ch = 2;
    bool i8_pool_forced = false;
    DevBuf<int> i8_dyn;      // the pool's two counters (zeroed once; the scan leaves them at 0)
    bool stream_lists = true;   // exact lists of <= 4 queries from one fp32 stream (IMGREC_STREAM_LISTS=0: tiles)
    bool merge_single = false;  // IMGREC_MERGE_SINGLE=1: the single-level merge in the rerank
    // IMGREC_B16W_SHARED_BOUND=0: the 256 x 256 bf16 kernel's lists screen each on their own (no
    // shared per-query bound, TileArgs::sbound)
    bool shared_bound = true;
    bool rerank_nw4 = false;    // IMGREC_RERANK_NW4=1: large batches rerank on 4-wave workgroups
    bool rerank_p1k = true;     // large batches rerank k rows first (IMGREC_RERANK_P1=0: 16)
    bool i8_fused_prep = true;  // int8 query prep inside the scan (IMGREC_I8_FUSED_PREP=0: own launch)
    bool merge_fuse1 = true;    // IMGREC_MERGE_FUSE=1: only level 2 in the rerank (0: neither)
    int64_t cap = 0, id_offset = 0;
    bool trained = true;
    DevBuf<float> xb;     // cap x dp
    DevBuf<float> xn;     // cap
    DevBuf<uint32_t> xs;  // cap x dp split-bf16 copy (built by the first split search)
    DevBuf<uint16_t> xh;  // cap x dpb bf16 copy (b16_ok only)
    DevBuf<float> xr;     // cap: |x - bf16(x)| per row (b16_ok only)
    DevBuf<int8_t> x8;    // cap x nblk8*64 block-scaled int8 copy (built by the first i8 search)
    DevBuf<float> x8s;    // cap x nblk8 block scales
    DevBuf<float> x8r;    // cap: |x - s c| per row
    DevBuf<float> x8r_max;   // device scalar, max of x8r
    // int8 tail copy of the 256 x 256 kernel (built by the first search that takes the route,
    // ensure_i8tail; DESIGN.md "int8 tail"): joint rows — columns xt_head .. dpb - 1 of every row as
    // codes, then its first xt_head columns as bf16 (the values of xh), so the kernel reads one array
    DevBuf<int8_t> xt;       // cap x xt_row bytes: xt_dpt codes (natural column order, pad 0) | xt_head bf16
    DevBuf<float> xts;       // cap: scale max|x_tail| / 127
    DevBuf<float4> xtm;      // cap: (|x_tail - s c|, |x_head - bf16(x_head)|, |x_tail|, |x_head|), rounded up
    DevBuf<float> xt_max;    // device: the four maxima of xtm (R_t, R_h, X_t, X_h)
    int xt_head = 0, xt_dpt = 0;     // (its state: IndexShape::xt_state)
    int xt_row = 0;                  // i8t_joint_row_bytes(xt_head, xt_dpt)
    // the copy's first search is a trial: its certificate counts decide whether the index keeps the
    // route (search_locked); false again after reset
    bool xt_tried = false;
    bool xt_no_trial = false;   // IMGREC_B16W_I8TAIL=2: no trial (measurement builds whose lists are wrong)
    bool xt_alloc_fail = false; // IMGREC_I8TAIL_ALLOC_FAIL=1 (tests): the copy's allocation counts as failed
    DevBuf<int8_t> qt;       // a search's query joint rows (nq_pad x xt_row), scales and inner-product bounds
    DevBuf<float> qts;
    DevBuf<float> q_eip;
    DevBuf<int8_t> q8;        // a search's two-level query codes
    DevBuf<float> q8s;       //   their scales
    DevBuf<float> q8r;       //   |q - q~| per query
    DevBuf<float> xn_max; // device scalar, max |x|^2 (refreshed when rows change)
    DevBuf<float> xr_max; // device scalar, max |x - bf16(x)|
    bool xn_max_stale = true;
    int last_path = 0;       // knn_last_path
    int64_t last_split_queries = 0;   // queries of the last search on a candidate path
    hipStream_t stream = nullptr;     // the index's own stream (host-pointer entry points)
    std::mutex mu;
    // cross-stream ordering of the index's operations (stream_fence.h; entry points run in an IndexOp)
    imgrec::Fence<imgrec::HipStreams> fence;
    // search workspace
    DevBuf<float> qpad;
    DevBuf<float> qnorm;
    DevBuf<float> cand_d;
    DevBuf<int64_t> cand_i;
    DevBuf<uint32_t> qsplit;
    DevBuf<float> cand2_d;
    DevBuf<int64_t> cand2_i;
    DevBuf<int> fail;          // the uncertified queries of a chunk
    DevBuf<int> chance;      // the second-chance queue of a chunk
    DevBuf<float> sc_key;    // sliced second chance (RerankArgs::sc_*)
    DevBuf<int64_t> sc_lab;
    DevBuf<unsigned> sc_meta;
    DevBuf<int> sc_done;
    DevBuf<int> stat;                               // 12 ints: two chunk parities + totals
    int stat_seq = 0;                                  // chunks run (parity = seq & 1)
    bool stat_valid = false;                           // the last search ran a candidate path
    DevBuf<uint16_t> qb16;
    DevBuf<float> q_resid;
    DevBuf<float> floor;
    DevBuf<float> heads;       // int8 lists' first keys (direct route)
    DevBuf<float> mws_d;          // two-level candidate merge workspace
    DevBuf<int64_t> mws_i;
    DevBuf<float> mws_f;
    DevBuf<uint32_t> sbound;       // shared screen bound records (kSBWords per query)
    // exact re-run workspace (device-planned: queries, candidate lists, plan)
    DevBuf<float> fb_q;
    DevBuf<float> fb_qn;
    DevBuf<float> fb_cd;
    DevBuf<int64_t> fb_ci;
    DevBuf<int> tail_ctl;   // tail claim counters + block tickets
    // host-path staging (device side), and page-locked host buffers for small searches
    PinBuf<float> pq;
    PinBuf<float> pd;
    PinBuf<int64_t> pi;
    DevBuf<float> hq;
    DevBuf<float> hd;
    DevBuf<int64_t> hi;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;   // pairs
    size_t ev_used = 0;
    // one index over several devices (knn_multi.cpp); NULL for a single-device index
    struct knn_multi* multi = nullptr;
    // k > KNN_MAX_K (knn_largek.hip): the fallback's stripe lists, the uncertified queries (+ count)
    DevBuf<uint64_t> lk_run;
    // a chunk's failed queries, then their count and the last large-k search's total (device)
    DevBuf<int> lk_fail;
    // k > KNN_MAX_K_LARGE (knn_hugek.hip): a query chunk's keys, sorted keys, segment offsets, and
    // the sort's temporary storage (bytes)
    DevBuf<uint64_t> hk_a;
    DevBuf<uint64_t> hk_b;
    DevBuf<unsigned> hk_off;
    DevBuf<char> hk_tmp;
    // range search (knn_range.hip): the append buffer (entries + their queries; starts at
    // range_cap0 entries, IMGREC_RANGE_CAP, and grows to a chunk's total when that overflows it),
    // the entries scattered into query segments, per-query counts, segment offsets, scatter
    // cursors, and the chunk's total on the device and in page-locked host memory
    size_t range_cap0 = size_t(1) << 20;
    DevBuf<uint64_t> rg_ent;
    DevBuf<uint32_t> rg_entq;
    DevBuf<uint64_t> rg_seg;
    DevBuf<uint32_t> rg_cnt;
    DevBuf<uint32_t> rg_off;
    DevBuf<uint32_t> rg_cur;
    DevBuf<unsigned long long> rg_total;
    PinBuf<unsigned long long> rg_total_h;
    // filtered search (knn_filter.hip): the compacted list of the selected rows (padded to a whole
    // tile), the compaction's per-block counts / offsets, the selected count on the device and in
    // page-locked host memory (read by the k > KNN_MAX_K route only), and the host form's device
    // copy of the bitmap
    DevBuf<uint32_t> ft_list;
    DevBuf<uint32_t> ft_blk;
    DevBuf<uint32_t> ft_m;
    PinBuf<uint32_t> ft_m_h;
    DevBuf<uint8_t> ft_bits;
    // remove_ids (knn_remove.hip): rows per bounce chunk when > 0 (IMGREC_REMOVE_CHUNK, tests), the
    // survivor count and first moved row in page-locked host memory, and a shard's copy of the
    // bitmap's per-word popcount prefix (multi-device renumbering)
    int64_t remove_chunk = 0;
    PinBuf<uint32_t> rm_h;
    DevBuf<uint32_t> rm_pref;
};

// One range search's result (knn_range_search): buffers on `device`, complete once `done` fires.
struct knn_range_result {
    int device = 0;
    int64_t nq = 0, size = 0;
    DevBuf<int64_t> lims;        // nq + 1
    DevBuf<float> D;             // size (one unused element when empty)
    DevBuf<int64_t> I;
    hipEvent_t done = nullptr;
};

namespace imgrec {

// knn_capi.cpp
const char* last_error();
int set_metric(knn_index* ix, int metric);
int set_trained(knn_index* ix, bool trained);
// One operation on an index: its lock, its device and its fence (stream_fence.h OpScope).
struct IndexOp : OpScope<HipStreams> {
    explicit IndexOp(knn_index* ix) : OpScope(ix->mu, ix->device, ix->fence, ix->stream) {}
};
// The host forms' staging on the index's own stream: nq queries up into hq (through the page-locked
// pq when `pinned`, which also reserves pd / pi) with room for nq x k results in hd / hi when k > 0;
// the bitmap's bytes that can matter (*nbits is lowered to ntotal) up into ft_bits; results down.
int stage_queries(knn_index* ix, const float* q, int64_t nq, int k, bool pinned = false);
int stage_bitmap(knn_index* ix, const uint8_t* bitmap, int64_t* nbits);
int fetch_results(knn_index* ix, int64_t nq, int k, float* D, int64_t* I);
// The per-row corpus arrays with their row strides in bytes, in allocation order: the only place
// that lists them.  Fills cols with the live ones (the split and int8 copies once materialised, the
// bf16 copy where enabled: what follows every add, regrowth and removal) and returns their number;
// all = true: with every column, at its kCol index.
enum { kColXb, kColXn, kColXs, kColXh, kColXr, kColX8, kColX8s, kColX8r, kColXt, kColXts, kColXtm, kCorpusColumns };
int corpus_columns(knn_index* ix, Column<DeviceSpace>* cols, bool all = false);
int reserve_rows(knn_index* ix, int64_t need, hipStream_t st);
int add_device_locked(knn_index* ix, const float* x, int64_t n, hipStream_t st);
int ensure_split(knn_index* ix, hipStream_t st);
int ensure_i8(knn_index* ix, hipStream_t st);
// the int8 tail copy: decides the index's eligibility and split column once (a host wait for the
// corpus statistics), builds the copy; xt_state says which.  drop_i8tail: the copy's only teardown,
// leaving xt_state = next (the caller has drained the streams that read it)
int ensure_i8tail(knn_index* ix, hipStream_t st);
void drop_i8tail(knn_index* ix, imgrec::TailCopy next);
int create_single(int d, int metric, int device, knn_index** out);
void free_single(knn_index* ix);
// knn_search.cpp
int search_locked(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                  hipStream_t st);
// knn_set_timing: records the first event of a pair on st and returns the second in *e1 (to be
// recorded after the timed launch); *e1 = NULL while timing is off
int timed_begin(knn_index* ix, hipStream_t st, hipEvent_t* e1);
int read_search_stats(knn_index* ix, int64_t* split_q, int64_t* fallback_q, int64_t* first_fail,
                      float* ratio);
// knn_largek.hip
int largek_search(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                  hipStream_t st);
// Exact per-(query, row split) top-32 lists of <= 4 queries from one fp32 stream of the corpus
// (csrc/knn_largek.hip largek_stream_kernel): the large-k route's lists and the exact route for
// small batches; lists at cd / ci + q * sp * 32 + s * 32 (labels with id_offset, -1 = empty).
bool stream_lists_ok(const knn_index* ix, int64_t nq);
int stream_splits(const knn_index* ix);
hipError_t launch_stream_lists(const knn_index* ix, const float* qpad, const float* qnorm, int64_t nq,
                               int metric, int sp, float* cd, int64_t* ci, hipStream_t st);
// queries the last large-k search sent to the exact scan (a device count: read on the index's own
// stream, which it synchronises; the caller holds a begun host scope when lk_fail exists)
int largek_fallbacks(knn_index* ix, int64_t* n);
// merge of nlists sorted per-shard lists for KNN_MAX_K < k (nlists * kin <= 8192; labels < 2^32)
hipError_t launch_merge_large(const float* cD, const int64_t* cI, int nlists, int64_t nq, int kin,
                              int64_t sd, int64_t si, int k, int metric, float* D, int64_t* I,
                              hipStream_t st);
// knn_hugek.hip: k > KNN_MAX_K_LARGE — every (query, row) key, a segmented sort per query
int hugek_search(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                 hipStream_t st);
// its segmented sort (knn_kernels.h) on an index's own temporary storage, which grows to what the
// sort asks for; and the same for nseg equal segments of `seg` keys, whose offsets it writes into
// `off` (nseg + 1 entries) first
hipError_t sort_u64_segments(uint64_t* in, uint64_t* out, int64_t total, int nseg, const unsigned* off,
                             unsigned end_bit, DevBuf<char>& tmp, hipStream_t st);
hipError_t sort_equal_segments(uint64_t* in, uint64_t* out, int nseg, int64_t seg, unsigned end_bit,
                               unsigned* off, DevBuf<char>& tmp, hipStream_t st);
// merge of nlists sorted lists of kin entries per query for any k (labels < 2^32)
hipError_t launch_merge_huge(const float* cD, const int64_t* cI, int nlists, int64_t nq, int kin,
                             int64_t sd, int64_t si, int k, int metric, float* D, int64_t* I,
                             hipStream_t st);
// the large-k list merge when it fits the in-LDS select (nlists * kin <= 8192), else the sort
hipError_t launch_merge_any(const float* cD, const int64_t* cI, int nlists, int64_t nq, int kin,
                            int64_t sd, int64_t si, int k, int metric, float* D, int64_t* I,
                            hipStream_t st);
// knn_range.hip: every row within `radius` of each of the nq device queries on `st` (waits once
// per query chunk for the chunk's size); labels are row + id_offset
int range_search_locked(knn_index* ix, const float* q, int64_t nq, float radius, hipStream_t st,
                        knn_range_result** out);
// a result on `device` from host arrays (the multi-device merge); waits for the upload
int range_result_from_host(int device, int64_t nq, const int64_t* lims, const float* D, const int64_t* I,
                           hipStream_t st, knn_range_result** out);
void range_result_free(knn_range_result* r);
// knn_filter.hip: the k best rows among those the bitmap selects (device bitmap, IDSelectorBitmap
// layout; bit lmap[r] for local row r when lmap is given, a shard's local -> global map), for the
// nq device queries on `st`; labels are row + id_offset.  Waits once only when k > KNN_MAX_K.
int filtered_search_locked(knn_index* ix, const float* q, int64_t nq, int k, const uint8_t* bits,
                           int64_t nbits, const int64_t* lmap, float* D, int64_t* I, hipStream_t st);
// its compaction alone: ft_list = the ascending local rows whose bit is set (invert: the stored rows
// whose bit is clear), padded with row 0 to 256 entries, and ft_m[0] = their count
int compact_rows(knn_index* ix, const uint8_t* bits, int64_t nbits, const int64_t* lmap, bool invert,
                 hipStream_t st);
// knn_remove.hip: the rows the device bitmap selects (bit lmap[r] for local row r when lmap is
// given) leave the index in place; `extra` (or NULL) is one more array of 8-byte rows compacted with
// them.  Waits once on `st` for the count; the moves may still run when it returns.
int remove_rows_locked(knn_index* ix, const uint8_t* bits, int64_t nbits, const int64_t* lmap,
                       int64_t* extra, hipStream_t st, int64_t* nremoved);
// lab[i] -= the set bits below lab[i] (words: the bitmap as 32-bit words, 0 at and past nbits; pref:
// their exclusive popcount prefix; removed: every set bit)
hipError_t launch_renumber_labels(int64_t* lab, int64_t n, const uint32_t* words, const uint32_t* pref,
                                  int64_t nbits, int64_t removed, hipStream_t st);

}  // namespace imgrec
