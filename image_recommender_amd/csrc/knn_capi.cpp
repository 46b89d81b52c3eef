// knn_capi.cpp — the C ABI of include/imgrec_knn.h: index lifetime, the HBM corpus buffer, adds,
// searches, merges, timing and stats.  The search paths live in knn_search.cpp, the route choice
// and launch geometry in knn_plan.h / knn_plan.cpp (HIP-free), the file layout in knn_io.cpp, the
// multi-device index in knn_multi.cpp.  The index's memory is owned by its DevBuf / PinBuf members
// (knn_index.h): free_single only quiesces the device and deletes the index; the corpus's per-row
// arrays are listed once, in corpus_columns.
//
// Reference call sites each entry point replaces are listed in include/imgrec_knn.h.
//
// Stream semantics: *_device entry points enqueue on the caller's stream and return without
// waiting for the GPU; host-pointer entry points run on the index's own stream and synchronise.
// Every entry point that touches the GPU runs inside an IndexOp (knn_index.h; stream_fence.h), so
// mixing streams (or host and device calls) is always ordered, also after an error exit.

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "knn_index.h"
#include "knn_multi.h"

namespace imgrec {

namespace {
thread_local std::string g_err;
}  // namespace

// The A/B and test knobs read at index creation (IMGREC_CUS, IMGREC_I8_WGPCU, IMGREC_MERGE_FUSE,
// IMGREC_CHANCE_SKIP, IMGREC_B16W_SHARED_BOUND; INTEGRATION.md "A/B switches"): not product
// settings.
// An inherited one silently re-plans every launch, so the first read of each that is set says so
// once on stderr.
const char* test_knob(const char* name) {
    const char* e = std::getenv(name);
    if (e && *e) {
        static std::mutex mu;
        static std::string seen;
        std::lock_guard<std::mutex> lk(mu);
        const std::string tag = std::string("|") + name + "|";
        if (seen.find(tag) == std::string::npos) {
            seen += tag;
            std::fprintf(stderr, "[imgrec] %s=%s overrides a launch default (test / A-B knob, "
                                 "INTEGRATION.md)\n", name, e);
        }
    }
    return e && *e ? e : nullptr;
}

void set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

const char* last_error() { return g_err.c_str(); }

// The corpus column table: every per-row array of the index with its row stride in bytes.
// reserve_rows, remove_rows_locked, add_device_locked, ensure_split and ensure_i8 all go through
// it, so a new column is added here (and its ingest launch to add_device_locked) and nowhere else.
int corpus_columns(knn_index* ix, Column<DeviceSpace>* cols, bool all) {
    int n = 0;
    cols[n++] = {&ix->xb, (size_t)ix->dp * sizeof(float)};
    cols[n++] = {&ix->xn, sizeof(float)};
    // the split copy exists only once a split-mode search has materialised it (ensure_split)
    if (all || ix->xs) cols[n++] = {&ix->xs, (size_t)ix->dp * sizeof(uint32_t)};
    if (all || ix->b16_ok) cols[n++] = {&ix->xh, (size_t)ix->dpb * sizeof(uint16_t)};
    if (all || ix->b16_ok) cols[n++] = {&ix->xr, sizeof(float)};
    // the int8 copy exists only once a small-batch search has materialised it (ensure_i8)
    if (all || ix->x8) cols[n++] = {&ix->x8, (size_t)i8_row_bytes(ix->nblk8)};
    if (all || ix->x8) cols[n++] = {&ix->x8s, (size_t)ix->nblk8 * sizeof(float)};
    if (all || ix->x8) cols[n++] = {&ix->x8r, sizeof(float)};
    // the int8 tail copy exists only once a large-batch search has materialised it (ensure_i8tail)
    if (all || ix->xt) cols[n++] = {&ix->xt, (size_t)ix->xt_row};
    if (all || ix->xt) cols[n++] = {&ix->xts, sizeof(float)};
    if (all || ix->xt) cols[n++] = {&ix->xtm, sizeof(float4)};
    return n;
}

// Grow the corpus buffers (every live column) to hold `need` rows; the copies of the existing rows
// run on `st` (ordered after the adds that wrote them), which is synchronised before the columns
// take their new blocks and the old ones are released (regrow_columns: all columns or none).
int reserve_rows(knn_index* ix, int64_t need, hipStream_t st) {
    if (need <= ix->cap) return KNN_OK;
    const int64_t ncap = round_up(std::max(need, ix->cap + ix->cap / 2), kTileRowsMax);
    Column<DeviceSpace> live[kCorpusColumns];
    const int n_all = corpus_columns(ix, live);
    // regrow_columns takes at most 8 columns: the int8 tail copy's three (the table's last) regrow
    // as a group of their own after the others.  Should that second group fail, the copy — which
    // can be rebuilt from the fp32 rows — is dropped instead of the whole regrowth.
    const int n_tail = ix->xt ? 3 : 0, n = n_all - n_tail;
    const size_t old = (size_t)ix->ntotal;
    hipError_t e = hipSuccess;
    const Column<DeviceSpace>* grp = live;
    auto fill_rows = [&](int i, void* dst, const void* src) {
        const size_t row = grp[i].stride;
        if (old && src) e = hipMemcpyAsync(dst, src, old * row, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync((char*)dst + old * row, 0, ((size_t)ncap - old) * row, st);
        return e == hipSuccess ? KNN_OK : KNN_EHIP;
    };
    auto wait_rows = [&]() {
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess) e = es;
        return e == hipSuccess ? KNN_OK : KNN_EHIP;
    };
    const int rc = regrow_columns(live, n, (size_t)ncap, fill_rows, wait_rows);
    if (rc != KNN_OK && e == hipSuccess) {   // no fill or wait failed: an allocation did
        (void)hipGetLastError();
        KNN_FAIL(KNN_ENOMEM, "hipMalloc of the %lld-row corpus buffers failed", (long long)ncap);
    }
    if (rc != KNN_OK) KNN_FAIL(KNN_EHIP, "corpus regrowth failed: %s", hipGetErrorString(e));
    ix->cap = ncap;
    if (n_tail > 0) {
        grp = live + n;
        if (regrow_columns(grp, n_tail, (size_t)ncap, fill_rows, wait_rows) != KNN_OK) {
            (void)hipGetLastError();
            drop_i8tail(ix, TailCopy::Undecided);      // the next large-batch search builds it again
        }
    }
    return KNN_OK;
}

// A lazily built copy's columns (table entries c0 .. c0 + n - 1) at the index's capacity, all or
// none; the caller fills them from the fp32 rows.
static int materialise_columns(knn_index* ix, int c0, int n) {
    Column<DeviceSpace> all[kCorpusColumns];
    corpus_columns(ix, all, true);
    const int rc = regrow_columns(all + c0, n, (size_t)std::max<int64_t>(ix->cap, 1),
                                  [](int, void*, const void*) { return KNN_OK; }, []() { return KNN_OK; });
    if (rc != KNN_OK) (void)hipGetLastError();
    return rc;
}

int add_device_locked(knn_index* ix, const float* x, int64_t n, hipStream_t st) {
    if ((int64_t)(ix->ntotal + n) > (int64_t)INT32_MAX)
        KNN_FAIL(KNN_EINVAL, "a single index shard holds at most 2^31-1 rows");
    int rc = reserve_rows(ix, ix->ntotal + n, st);
    if (rc != KNN_OK) return rc;
    // the new rows' place in every column (the ingest launches stay explicit: different kernels)
    Column<DeviceSpace> c[kCorpusColumns];
    corpus_columns(ix, c, true);
    auto at = [&](int col) { return (char*)c[col].buf->data() + (size_t)ix->ntotal * c[col].stride; };
    float* const xb = (float*)at(kColXb);
    KNN_HIP(launch_rows_ingest(x, n, ix->d, ix->dp, n, ix->metric == KNN_METRIC_COSINE ? 1 : 0, xb,
                               (float*)at(kColXn), st));
    if (ix->xs) KNN_HIP(launch_split_rows(xb, n, ix->dp, kSplitBK, (uint32_t*)at(kColXs), st));
    if (ix->b16_ok)
        KNN_HIP(launch_bf16_rows(xb, n, ix->dp, ix->dpb, (uint16_t*)at(kColXh), (float*)at(kColXr), st));
    if (ix->x8)
        KNN_HIP(launch_i8_rows(xb, n, ix->dp, ix->nblk8, (int8_t*)at(kColX8), (float*)at(kColX8s),
                               (float*)at(kColX8r), st));
    if (ix->xt) {
        KNN_HIP(launch_i8tail_rows(xb, n, ix->dp, ix->dpb, ix->xt_head, ix->xt_dpt, ix->xt_row, (int8_t*)at(kColXt),
                                   (float*)at(kColXts), (float4*)at(kColXtm), st));
        ix->xt_tried = false;        // new rows can move the copy's maxima: the next search is a trial again
    }
    ix->ntotal += n;
    ix->xn_max_stale = true;
    return KNN_OK;
}

// The split-bf16 copy (cap x dp words, as many bytes as the fp32 rows) is built on the first
// search that runs the split path, from the stored fp32 rows, and kept up to date by later adds.
// AUTO never takes the split path while the bf16 copy exists (every d >= 64), so a default index
// holds only the fp32 rows, norms and the bf16 copy: 12 GB instead of 20 GB per 1M x 1968 rows.
int ensure_split(knn_index* ix, hipStream_t st) {
    if (ix->xs) return KNN_OK;
    if (!ix->split_ok) KNN_FAIL(KNN_EINVAL, "split search needs d >= 256; d = %d", ix->d);
    if (materialise_columns(ix, kColXs, 1) != KNN_OK)
        KNN_FAIL(KNN_ENOMEM, "hipMalloc of the %lld-row split copy failed", (long long)ix->cap);
    if (ix->ntotal > 0)
        KNN_HIP(launch_split_rows(ix->xb, ix->ntotal, ix->dp, kSplitBK, ix->xs, st));
    return KNN_OK;
}

// The block-scaled int8 copy (i8_row_bytes(nblk8) + nblk8 scales + one residual per row, about half
// the bf16 copy) is built on the first search that runs the int8 small-batch path, from the stored
// fp32 rows, and kept up to date by later adds (the split copy's pattern).
int ensure_i8(knn_index* ix, hipStream_t st) {
    if (ix->x8) return KNN_OK;
    if (ix->nblk8 <= 0) KNN_FAIL(KNN_EINVAL, "int8 search needs 64 <= d <= 4096; d = %d", ix->d);
    if (materialise_columns(ix, kColX8, 3) != KNN_OK)
        KNN_FAIL(KNN_ENOMEM, "hipMalloc of the %lld-row int8 copy failed", (long long)ix->cap);
    ix->xn_max_stale = true;             // refresh_maxima computes the int8 residual maximum
    if (ix->ntotal > 0)
        KNN_HIP(launch_i8_rows(ix->xb, ix->ntotal, ix->dp, ix->nblk8, ix->x8, ix->x8s, ix->x8r, st));
    return KNN_OK;
}

// The int8 tail copy of the 256 x 256 kernel (a joint row of dpt code bytes and 2 H bytes of bf16
// head + a scale + four statistics per row: 2.2 GB per 1M x 1968 rows) is built on the first search that takes the route, from the stored fp32
// rows, and kept up to date by later adds (the int8 scan copy's pattern).  The split column comes
// from the corpus as it stands then (i8t_pick_head), which costs one host wait for the block
// maxima; the decision — eligible or not — then holds until knn_reset.
int ensure_i8tail(knn_index* ix, hipStream_t st) {
    if (ix->xt_state != TailCopy::Undecided) return KNN_OK;
    if (ix->ntotal <= 0 || !ix->b16_ok || ix->dpb > 4096) { ix->xt_state = TailCopy::Ineligible; return KNN_OK; }
    const int nblk = ix->dpb / kB16Pad;
    DevBuf<float> dmax;
    int rc;
    if ((rc = dmax.reserve((size_t)nblk)) != KNN_OK) return rc;
    std::vector<float> hmax((size_t)nblk);
    KNN_HIP(launch_block_absmax(ix->xb, ix->ntotal, ix->dp, nblk, dmax, st));
    KNN_HIP(hipMemcpyAsync(hmax.data(), dmax, (size_t)nblk * sizeof(float), hipMemcpyDeviceToHost, st));
    KNN_HIP(hipStreamSynchronize(st));
    const int head = i8t_pick_head(hmax.data(), nblk);
    if (head < 0) { ix->xt_state = TailCopy::Ineligible; return KNN_OK; }
    ix->xt_head = head;
    ix->xt_dpt = (int)round_up(ix->dpb - head, 128);
    ix->xt_row = i8t_joint_row_bytes(head, ix->xt_dpt);
    // no room for the copy: the index searched on the bf16 pass before and goes on doing so
    if (ix->xt_alloc_fail || materialise_columns(ix, kColXt, 3) != KNN_OK) {
        drop_i8tail(ix, TailCopy::Ineligible);
        return KNN_OK;
    }
    // (pad rows of the joint rows and scales are read by the kernel's partial tiles: zero)
    KNN_HIP(hipMemsetAsync(ix->xt, 0, (size_t)ix->cap * ix->xt_row, st));
    KNN_HIP(hipMemsetAsync(ix->xts, 0, (size_t)ix->cap * sizeof(float), st));
    KNN_HIP(hipMemsetAsync(ix->xtm, 0, (size_t)ix->cap * sizeof(float4), st));
    ix->xn_max_stale = true;             // refresh_maxima computes the copy's maxima
    KNN_HIP(launch_i8tail_rows(ix->xb, ix->ntotal, ix->dp, ix->dpb, head, ix->xt_dpt, ix->xt_row, ix->xt, ix->xts,
                               ix->xtm, st));
    ix->xt_state = TailCopy::Built;
    return KNN_OK;
}

// The copy's only teardown.  The caller has drained every stream that may still read the blocks.
// Every caller gets the whole reset, where each used to clear its own subset of xt_head, xt_dpt and
// xt_tried: the difference cannot be observed, since they (and xt_row) are read only while the copy is
// Built (searches, adds, corpus_columns' live columns, knn_debug_i8tail) or after the next
// ensure_i8tail wrote them on its way from Undecided.
void drop_i8tail(knn_index* ix, TailCopy next) {
    ix->xt.reset(); ix->xts.reset(); ix->xtm.reset();
    ix->xt_head = ix->xt_dpt = ix->xt_row = 0;
    ix->xt_tried = false; ix->xt_state = next;
}

int create_single(int d, int metric, int device, knn_index** out) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        KNN_FAIL(KNN_ENOSYS, "no HIP device visible");
    if (device < 0) KNN_HIP(hipGetDevice(&device));
    if (device >= ndev) KNN_FAIL(KNN_EINVAL, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    knn_index* ix = new knn_index();
    ix->d = d;
    // rows padded to 16 floats; from d >= 256 to 32, so the 32-deep staging path and the split
    // copy (32-float stages) serve every d the split path takes
    ix->dp = (int)round_up(d, d >= 256 ? 2 * kDepthPad : kDepthPad);
    ix->metric = metric;
    ix->device = device;
    ix->split_ok = ix->dp % 32 == 0 && d >= 256;
    ix->b16_ok = d >= 64;
    ix->dpb = (int)round_up(d, kB16Pad);
    ix->nblk8 = d >= 64 && d <= 4096 ? (d + 63) / 64 : 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        cus > 0)
        ix->cus = cus;
    // IMGREC_CUS=n (tests): plan launches for n CUs, as on a partitioned device (CPX mode)
    if (const char* e = test_knob("IMGREC_CUS")) {
        const int v = std::atoi(e);
        if (v > 0 && v < ix->cus) ix->cus = v;
    }
    if (const char* e = test_knob("IMGREC_I8_WGPCU")) {
        const int v = std::atoi(e);
        if (v > 0 && v <= 16) ix->i8_wgpcu = v;
    }
    if (const char* e = test_knob("IMGREC_MERGE_FUSE")) {
        ix->merge_fuse = *e != '0';
        ix->merge_fuse1 = *e != '0' && *e != '1';
    }
    if (const char* e = test_knob("IMGREC_CHANCE_SKIP")) ix->chance_skip = *e != '0';
    if (const char* e = test_knob("IMGREC_CHANCE_DIRECT")) ix->chance_direct_max = std::max(0, std::atoi(e));
    if (const char* e = test_knob("IMGREC_I8_HALF_K")) {
        const int v = std::atoi(e);
        ix->i8_half_k = v >= 2 ? v : 0;
    }
    if (const char* e = test_knob("IMGREC_I8_POOL")) {
        ix->i8_pool64 = std::min(64, std::max(0, std::atoi(e)));
        ix->i8_pool_forced = true;
    }
    if (const char* e = test_knob("IMGREC_I8_POOL_CH")) ix->i8_pool_ch = std::min(64, std::max(1, std::atoi(e)));
    if (const char* e = test_knob("IMGREC_DIRECT_RAW")) ix->direct_raw = std::min(2, std::max(0, std::atoi(e)));
    if (const char* e = test_knob("IMGREC_I8_FUSED_PREP")) ix->i8_fused_prep = *e != '0';
    if (const char* e = test_knob("IMGREC_RERANK_P1")) ix->rerank_p1k = *e != '0';
    if (const char* e = test_knob("IMGREC_RERANK_NW4")) ix->rerank_nw4 = *e != '0';
    if (const char* e = test_knob("IMGREC_MERGE_SINGLE")) ix->merge_single = *e != '0';
    if (const char* e = test_knob("IMGREC_STREAM_LISTS")) ix->stream_lists = *e != '0';
    if (const char* e = test_knob("IMGREC_B16W_SHARED_BOUND")) ix->shared_bound = *e != '0';
    if (const char* e = test_knob("IMGREC_B16W_I8TAIL")) {
        ix->i8tail = *e != '0';
        ix->xt_no_trial = *e == '2';
    }
    // IMGREC_I8TAIL_ALLOC_FAIL=1 (tests): the int8 tail copy's allocation fails, as on a full device
    if (const char* e = test_knob("IMGREC_I8TAIL_ALLOC_FAIL")) ix->xt_alloc_fail = *e != '0';
    // IMGREC_RANGE_CAP=<entries> (tests): the range search's initial append capacity, so small
    // shapes reach the overflow re-run
    if (const char* e = test_knob("IMGREC_RANGE_CAP")) {
        const long long v = std::atoll(e);
        if (v > 0) ix->range_cap0 = (size_t)v;
    }
    // IMGREC_REMOVE_CHUNK=<rows> (tests): rows per bounce chunk of remove_ids, so small shapes run
    // several chunks
    if (const char* e = test_knob("IMGREC_REMOVE_CHUNK")) {
        const long long v = std::atoll(e);
        if (v > 0) ix->remove_chunk = (int64_t)v;
    }
    if (hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking) != hipSuccess ||
        ix->fence.create() != KNN_OK) {
        if (ix->stream) (void)hipStreamDestroy(ix->stream);
        delete ix;
        KNN_FAIL(KNN_EHIP, "hipStreamCreate / hipEventCreate failed");
    }
    *out = ix;
    return KNN_OK;
}

void free_single(knn_index* ix) {
    DeviceGuard g(ix->device);
    (void)hipDeviceSynchronize();       // searches on other streams may still use the buffers
    for (hipEvent_t e : ix->ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ix->stream);
    delete ix;                          // (every buffer and the fence's event, while the guard holds)
}

// Batches whose query rows fit this many bytes go through page-locked staging: a pageable copy
// is a driver-staged, host-synchronous transfer on each side of a one-query search (round 1
// measured 47 us of PCIe-side overhead per one-query search), while a memcpy of a few KB into a
// pinned buffer and one DMA each way are a few us.  Larger batches copy pageable memory directly.
constexpr size_t kPinnedSearchBytes = 1 << 20;

int stage_queries(knn_index* ix, const float* q, int64_t nq, int k, bool pinned) {
    int rc;
    const size_t nqd = (size_t)nq * ix->d, nk = (size_t)nq * k;
    if ((rc = ix->hq.reserve(nqd)) != KNN_OK) return rc;
    if (k > 0 && (rc = ix->hd.reserve(nk)) != KNN_OK) return rc;
    if (k > 0 && (rc = ix->hi.reserve(nk)) != KNN_OK) return rc;
    if (pinned) {
        if ((rc = ix->pq.reserve(nqd)) != KNN_OK) return rc;
        if ((rc = ix->pd.reserve(nk)) != KNN_OK) return rc;
        if ((rc = ix->pi.reserve(nk)) != KNN_OK) return rc;
        // (the previous host-pointer search synchronised before returning: the buffers are free)
        std::memcpy(ix->pq, q, nqd * sizeof(float));
    }
    KNN_HIP(hipMemcpyAsync(ix->hq, pinned ? ix->pq : q, nqd * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    return KNN_OK;
}

int stage_bitmap(knn_index* ix, const uint8_t* bitmap, int64_t* nbits) {
    *nbits = std::min(*nbits, ix->ntotal);
    const size_t nbytes = (size_t)((*nbits + 7) / 8);
    const int rc = ix->ft_bits.reserve(std::max<size_t>(nbytes, 1));
    if (rc != KNN_OK) return rc;
    if (nbytes) KNN_HIP(hipMemcpyAsync(ix->ft_bits, bitmap, nbytes, hipMemcpyHostToDevice, ix->stream));
    return KNN_OK;
}

int fetch_results(knn_index* ix, int64_t nq, int k, float* D, int64_t* I) {
    const size_t nk = (size_t)nq * k;
    KNN_HIP(hipMemcpyAsync(D, ix->hd, nk * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    KNN_HIP(hipMemcpyAsync(I, ix->hi, nk * sizeof(int64_t), hipMemcpyDeviceToHost, ix->stream));
    return KNN_OK;
}

int set_metric(knn_index* ix, int metric) {
    if (ix->multi) return multi_set_metric(ix, metric);
    ix->metric = metric;
    return KNN_OK;
}

int set_trained(knn_index* ix, bool trained) {
    ix->trained = trained;
    if (ix->multi) return multi_set_trained(ix, trained);
    return KNN_OK;
}

}  // namespace imgrec

using namespace imgrec;

extern "C" {

const char* knn_last_error(void) { return imgrec::last_error(); }
const char* knn_version(void) {
    return "imgrec-knn 0.2 (gfx950: bf16 / split-bf16 / f32 MFMA candidates, fused top-k, "
           "device-side certificate)";
}

int knn_create(int d, int metric, int device, knn_index_t** out) {
    if (!out) KNN_FAIL(KNN_EINVAL, "out is NULL");
    *out = nullptr;
    if (d <= 0) KNN_FAIL(KNN_EINVAL, "d must be positive (got %d)", d);
    if (metric != KNN_METRIC_L2 && metric != KNN_METRIC_IP && metric != KNN_METRIC_COSINE)
        KNN_FAIL(KNN_EINVAL, "unknown metric %d", metric);
    return create_single(d, metric, device, out);
}

int knn_free(knn_index_t* ix) {
    if (!ix) return KNN_OK;
    if (ix->multi) return multi_free(ix);
    free_single(ix);
    return KNN_OK;
}

int knn_dim(const knn_index_t* ix) { return ix ? ix->d : KNN_EINVAL; }
int knn_metric(const knn_index_t* ix) { return ix ? ix->metric : KNN_EINVAL; }
int64_t knn_ntotal(const knn_index_t* ix) { return ix ? ix->ntotal : KNN_EINVAL; }
int knn_is_trained(const knn_index_t* ix) { return ix ? (ix->trained ? 1 : 0) : KNN_EINVAL; }

int knn_set_id_offset(knn_index_t* ix, int64_t off) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->id_offset = off;
    return KNN_OK;
}

int knn_train(knn_index_t* ix, const float* x, int64_t n) {
    (void)x;
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (n < 0) KNN_FAIL(KNN_EINVAL, "n must be >= 0");
    return set_trained(ix, true);
}

int knn_reserve(knn_index_t* ix, int64_t n) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (ix->multi) return multi_reserve(ix, n);
    IndexOp op(ix);
    int rc = op.begin(ix->stream);
    if (rc == KNN_OK) rc = reserve_rows(ix, n, ix->stream);
    return op.finish(rc);
}

static int add_args_ok(knn_index_t* ix, const float* x, int64_t n) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (n < 0 || (n > 0 && !x)) KNN_FAIL(KNN_EINVAL, "bad rows (n=%lld)", (long long)n);
    return KNN_OK;
}

int knn_add_device(knn_index_t* ix, const float* x, int64_t n, void* stream) {
    int rc;
    if ((rc = add_args_ok(ix, x, n)) != KNN_OK || n == 0) return rc;
    if (ix->multi) return multi_add_device(ix, x, n, (hipStream_t)stream);
    IndexOp op(ix);
    if ((rc = op.begin((hipStream_t)stream)) == KNN_OK) rc = add_device_locked(ix, x, n, op.stream());
    return op.finish(rc);
}

int knn_add(knn_index_t* ix, const float* x, int64_t n) {
    int rc;
    if ((rc = add_args_ok(ix, x, n)) != KNN_OK || n == 0) return rc;
    if (ix->multi) return multi_add(ix, x, n);
    IndexOp op(ix);
    if ((rc = op.begin_host()) != KNN_OK) return rc;
    if ((rc = reserve_rows(ix, ix->ntotal + n, ix->stream)) != KNN_OK) return rc;
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(64 << 20) / ((int64_t)ix->d * 4));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t cn = std::min(chunk, n - r0);
        if ((rc = stage_queries(ix, x + r0 * ix->d, cn, 0)) != KNN_OK) return rc;
        if ((rc = add_device_locked(ix, ix->hq, cn, ix->stream)) != KNN_OK) return rc;
        KNN_HIP(hipStreamSynchronize(ix->stream));
    }
    return op.finish_synced(KNN_OK);
}

int knn_reset(knn_index_t* ix) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (ix->multi) return multi_reset(ix);
    IndexOp op(ix);
    // the int8 tail copy goes with the rows its split column was chosen from (it is read by searches
    // that may still run: wait for them before the blocks are released)
    if (ix->xt_state != TailCopy::Undecided) {
        int rc = ix->xt ? op.begin_host() : KNN_OK;
        if (rc == KNN_OK && ix->xt) rc = HipStreams::fail(hipStreamSynchronize(ix->stream), "hipStreamSynchronize");
        if (rc != KNN_OK) return op.finish(rc);
        drop_i8tail(ix, TailCopy::Undecided);
        ix->ntotal = 0;
        ix->xn_max_stale = true;
        return op.finish_synced(KNN_OK);
    }
    ix->ntotal = 0;
    ix->xn_max_stale = true;
    return KNN_OK;
}

int knn_remove_ids(knn_index_t* ix, const uint8_t* bitmap, int64_t nbits, int64_t* nremoved) {
    if (nremoved) *nremoved = 0;
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (nbits < 0) KNN_FAIL(KNN_EINVAL, "nbits must be >= 0 (got %lld)", (long long)nbits);
    if (nbits > 0 && !bitmap) KNN_FAIL(KNN_EINVAL, "bitmap is NULL with nbits = %lld", (long long)nbits);
    int64_t n = 0;
    if (ix->multi) {
        const int rc = multi_remove_ids(ix, bitmap, nbits, &n);
        if (rc == KNN_OK && nremoved) *nremoved = n;
        return rc;
    }
    IndexOp op(ix);
    int rc = op.begin_host();
    nbits = std::min(nbits, ix->ntotal);             // bits at or past ntotal are ignored
    if (rc == KNN_OK && nbits > 0) rc = stage_bitmap(ix, bitmap, &nbits);
    if (rc == KNN_OK && nbits > 0) rc = remove_rows_locked(ix, ix->ft_bits, nbits, nullptr, nullptr, ix->stream, &n);
    if ((rc = op.finish(rc)) == KNN_OK && nremoved) *nremoved = n;
    return rc;
}

int knn_reconstruct_n(const knn_index_t* cix, int64_t i0, int64_t n, float* x) {
    knn_index* ix = const_cast<knn_index*>(cix);
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (i0 < 0 || n < 0 || i0 + n > ix->ntotal || (n > 0 && !x))
        KNN_FAIL(KNN_EINVAL, "reconstruct range [%lld, %lld) outside [0, %lld)", (long long)i0,
                 (long long)(i0 + n), (long long)ix->ntotal);
    if (n == 0) return KNN_OK;
    if (ix->multi) return multi_reconstruct_n(ix, i0, n, x);
    IndexOp op(ix);
    if (const int rc = op.begin_host()) return rc;
    KNN_HIP(hipMemcpy2DAsync(x, (size_t)ix->d * 4, ix->xb + (size_t)i0 * ix->dp, (size_t)ix->dp * 4,
                             (size_t)ix->d * 4, (size_t)n, hipMemcpyDeviceToHost, ix->stream));
    return op.finish(KNN_OK);
}

static int search_args_ok(knn_index_t* ix, const float* q, int64_t nq, int k, const float* D, const int64_t* I) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (k <= 0) KNN_FAIL(KNN_EINVAL, "k must be >= 1 (got %d)", k);
    if (nq < 0 || (nq > 0 && (!q || !D || !I))) KNN_FAIL(KNN_EINVAL, "bad query/output pointers");
    return KNN_OK;
}

int knn_search_device(knn_index_t* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                      void* stream) {
    int rc;
    if ((rc = search_args_ok(ix, q, nq, k, D, I)) != KNN_OK || nq == 0) return rc;
    if (ix->multi) return multi_search_device(ix, q, nq, k, D, I, (hipStream_t)stream);
    IndexOp op(ix);
    if ((rc = op.begin((hipStream_t)stream)) == KNN_OK) rc = search_locked(ix, q, nq, k, D, I, op.stream());
    return op.finish(rc);
}

int knn_search(knn_index_t* ix, const float* q, int64_t nq, int k, float* D, int64_t* I) {
    int rc;
    if ((rc = search_args_ok(ix, q, nq, k, D, I)) != KNN_OK || nq == 0) return rc;
    if (ix->multi) return multi_search(ix, q, nq, k, D, I);
    IndexOp op(ix);
    const bool pinned = (size_t)nq * ix->d * sizeof(float) <= kPinnedSearchBytes;
    if ((rc = op.begin_host()) == KNN_OK) rc = stage_queries(ix, q, nq, k, pinned);
    if (rc == KNN_OK) rc = search_locked(ix, ix->hq, nq, k, ix->hd, ix->hi, ix->stream);
    if (rc == KNN_OK) rc = fetch_results(ix, nq, k, pinned ? ix->pd.get() : D, pinned ? ix->pi.get() : I);
    if ((rc = op.finish(rc)) == KNN_OK && pinned) {
        std::memcpy(D, ix->pd, (size_t)nq * k * sizeof(float));
        std::memcpy(I, ix->pi, (size_t)nq * k * sizeof(int64_t));
    }
    return rc;
}

static int range_args_ok(knn_index_t* ix, const float* q, int64_t nq, float radius,
                         knn_range_result_t** out) {
    if (out) *out = nullptr;
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (!out) KNN_FAIL(KNN_EINVAL, "out is NULL");
    if (nq < 0 || (nq > 0 && !q)) KNN_FAIL(KNN_EINVAL, "bad query pointer (nq=%lld)", (long long)nq);
    if (radius != radius) KNN_FAIL(KNN_EINVAL, "radius is NaN");
    return KNN_OK;
}

int knn_range_search_device(knn_index_t* ix, const float* q, int64_t nq, float radius, void* stream,
                            knn_range_result_t** out) {
    int rc;
    if ((rc = range_args_ok(ix, q, nq, radius, out)) != KNN_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (ix->multi) return multi_range_search(ix, q, false, nq, radius, st, out);
    IndexOp op(ix);
    if ((rc = op.begin(st)) == KNN_OK) rc = range_search_locked(ix, q, nq, radius, st, out);
    return op.finish(rc);
}

int knn_range_search(knn_index_t* ix, const float* q, int64_t nq, float radius,
                     knn_range_result_t** out) {
    int rc;
    if ((rc = range_args_ok(ix, q, nq, radius, out)) != KNN_OK) return rc;
    if (ix->multi) return multi_range_search(ix, q, true, nq, radius, nullptr, out);
    IndexOp op(ix);
    if ((rc = op.begin_host()) == KNN_OK && nq > 0) rc = stage_queries(ix, q, nq, 0);
    if (rc == KNN_OK) rc = range_search_locked(ix, ix->hq, nq, radius, ix->stream, out);
    return op.finish(rc);
}

int64_t knn_range_nq(const knn_range_result_t* r) { return r ? r->nq : KNN_EINVAL; }
int64_t knn_range_size(const knn_range_result_t* r) { return r ? r->size : KNN_EINVAL; }

int knn_range_copy(const knn_range_result_t* r, int64_t* lims, float* D, int64_t* I) {
    if (!r) KNN_FAIL(KNN_EINVAL, "result is NULL");
    DeviceGuard g(r->device);
    KNN_HIP(hipEventSynchronize(r->done));
    if (lims) KNN_HIP(hipMemcpy(lims, r->lims, (size_t)(r->nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (D && r->size > 0) KNN_HIP(hipMemcpy(D, r->D, (size_t)r->size * sizeof(float), hipMemcpyDeviceToHost));
    if (I && r->size > 0) KNN_HIP(hipMemcpy(I, r->I, (size_t)r->size * sizeof(int64_t), hipMemcpyDeviceToHost));
    return KNN_OK;
}

int knn_range_device(const knn_range_result_t* r, const int64_t** lims, const float** D,
                     const int64_t** I) {
    if (!r) KNN_FAIL(KNN_EINVAL, "result is NULL");
    DeviceGuard g(r->device);
    KNN_HIP(hipEventSynchronize(r->done));
    if (lims) *lims = r->lims;
    if (D) *D = r->D;
    if (I) *I = r->I;
    return KNN_OK;
}

int knn_range_free(knn_range_result_t* r) {
    range_result_free(r);
    return KNN_OK;
}

static int filtered_args_ok(knn_index_t* ix, const float* q, int64_t nq, int k, const uint8_t* bitmap,
                            int64_t nbits, const float* D, const int64_t* I) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (k <= 0) KNN_FAIL(KNN_EINVAL, "k must be >= 1 (got %d)", k);
    if (nbits < 0) KNN_FAIL(KNN_EINVAL, "nbits must be >= 0 (got %lld)", (long long)nbits);
    if (nbits > 0 && !bitmap) KNN_FAIL(KNN_EINVAL, "bitmap is NULL with nbits = %lld", (long long)nbits);
    if (nq < 0 || (nq > 0 && (!q || !D || !I))) KNN_FAIL(KNN_EINVAL, "bad query/output pointers");
    return KNN_OK;
}

int knn_search_filtered_device(knn_index_t* ix, const float* q, int64_t nq, int k, const uint8_t* bitmap,
                               int64_t nbits, float* D, int64_t* I, void* stream) {
    int rc;
    if ((rc = filtered_args_ok(ix, q, nq, k, bitmap, nbits, D, I)) != KNN_OK || nq == 0) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (ix->multi) return multi_search_filtered(ix, q, false, nq, k, bitmap, nbits, D, I, st);
    IndexOp op(ix);
    if ((rc = op.begin(st)) == KNN_OK) rc = filtered_search_locked(ix, q, nq, k, bitmap, nbits, nullptr, D, I, st);
    return op.finish(rc);
}

int knn_search_filtered(knn_index_t* ix, const float* q, int64_t nq, int k, const uint8_t* bitmap,
                        int64_t nbits, float* D, int64_t* I) {
    int rc;
    if ((rc = filtered_args_ok(ix, q, nq, k, bitmap, nbits, D, I)) != KNN_OK || nq == 0) return rc;
    if (ix->multi) return multi_search_filtered(ix, q, true, nq, k, bitmap, nbits, D, I, nullptr);
    IndexOp op(ix);
    if ((rc = op.begin_host()) == KNN_OK) rc = stage_queries(ix, q, nq, k);
    if (rc == KNN_OK) rc = stage_bitmap(ix, bitmap, &nbits);
    if (rc == KNN_OK)
        rc = filtered_search_locked(ix, ix->hq, nq, k, ix->ft_bits, nbits, nullptr, ix->hd, ix->hi, ix->stream);
    if (rc == KNN_OK) rc = fetch_results(ix, nq, k, D, I);
    return op.finish(rc);
}

int knn_merge_device(const float* cD, const int64_t* cI, int nlists, int64_t nq, int kin, int k,
                     int metric, float* D, int64_t* I, void* stream) {
    if (nlists <= 0 || kin <= 0 || nq < 0) KNN_FAIL(KNN_EINVAL, "bad merge shape");
    if (k <= 0) KNN_FAIL(KNN_EINVAL, "k must be >= 1 (got %d)", k);
    if (nq == 0) return KNN_OK;
    if (!cD || !cI || !D || !I) KNN_FAIL(KNN_EINVAL, "NULL pointer");
    const int kmetric = metric == KNN_METRIC_L2 ? 1 : 0;
    if (k > KNN_MAX_K) {
        KNN_HIP(launch_merge_any(cD, cI, nlists, nq, kin, nq * (int64_t)kin, nq * (int64_t)kin, k,
                                 kmetric, D, I, (hipStream_t)stream));
        return KNN_OK;
    }
    KNN_HIP(launch_merge(cD, cI, nq, nlists, kin, kin, nq * (int64_t)kin, k, kmetric,
                         kmetric ? 0 : 1, D, I, (hipStream_t)stream));
    return KNN_OK;
}

int64_t knn_packed_bytes(int64_t nq, int k) {
    if (nq < 0 || k <= 0) return KNN_EINVAL;
    const int64_t n = nq * k;
    return (n + (n & 1)) * 4 + n * 8;
}

int knn_merge_packed_device(const void* packed, int nlists, int64_t nq, int kin, int k, int metric,
                            float* D, int64_t* I, void* stream) {
    if (nlists <= 0 || kin <= 0 || nq < 0) KNN_FAIL(KNN_EINVAL, "bad merge shape");
    if (k <= 0) KNN_FAIL(KNN_EINVAL, "k must be >= 1 (got %d)", k);
    if (nq == 0) return KNN_OK;
    if (!packed || !D || !I) KNN_FAIL(KNN_EINVAL, "NULL pointer");
    const int64_t n = nq * kin, nf = n + (n & 1);
    const float* cD = static_cast<const float*>(packed);
    const int64_t* cI = reinterpret_cast<const int64_t*>(static_cast<const char*>(packed) + nf * 4);
    const int kmetric = metric == KNN_METRIC_L2 ? 1 : 0;
    if (k > KNN_MAX_K) {
        KNN_HIP(launch_merge_any(cD, cI, nlists, nq, kin, nf + 2 * n, nf / 2 + n, k, kmetric, D, I,
                                 (hipStream_t)stream));
        return KNN_OK;
    }
    // chunk = nf floats + n int64: nf + 2n floats, nf / 2 + n int64
    KNN_HIP(launch_merge_strided(cD, cI, nq, nlists, kin, kin, nf + 2 * n, nf / 2 + n, k, kmetric,
                                 kmetric ? 0 : 1, D, I, (hipStream_t)stream));
    return KNN_OK;
}

int knn_set_timing(knn_index_t* ix, int enable) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (ix->multi) return multi_set_timing(ix, enable);
    IndexOp op(ix);
    ix->timing = enable != 0;
    ix->ev_used = 0;
    return KNN_OK;
}

int knn_set_fence_mode(knn_index_t* ix, int mode) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (mode != KNN_FENCE_EAGER && mode != KNN_FENCE_LAZY) KNN_FAIL(KNN_EINVAL, "unknown fence mode %d", mode);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->multi) {
        int rc = multi_set_fence_mode(ix, mode);
        if (rc != KNN_OK) return rc;
    }
    ix->fence.lazy = mode == KNN_FENCE_LAZY;
    return KNN_OK;
}

int knn_kernel_time(knn_index_t* ix, double* total_ms, int* launches) {
    if (!ix || !total_ms || !launches) KNN_FAIL(KNN_EINVAL, "NULL argument");
    if (ix->multi) return multi_kernel_time(ix, total_ms, launches);
    IndexOp op(ix);
    double tot = 0.0;
    for (size_t i = 0; i + 1 < ix->ev_used; i += 2) {
        KNN_HIP(hipEventSynchronize(ix->ev[i + 1]));
        float ms = 0.f;
        KNN_HIP(hipEventElapsedTime(&ms, ix->ev[i], ix->ev[i + 1]));
        tot += ms;
    }
    *total_ms = tot;
    *launches = (int)(ix->ev_used / 2);
    ix->ev_used = 0;
    return KNN_OK;
}

int knn_set_search_mode(knn_index_t* ix, int mode) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (mode != KNN_SEARCH_AUTO && mode != KNN_SEARCH_EXACT && mode != KNN_SEARCH_SPLIT &&
        mode != KNN_SEARCH_BF16 && mode != KNN_SEARCH_I8)
        KNN_FAIL(KNN_EINVAL, "unknown search mode %d", mode);
    if (ix->multi) return multi_set_search_mode(ix, mode);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (mode == KNN_SEARCH_SPLIT && !ix->split_ok)
        KNN_FAIL(KNN_EINVAL, "split search needs d >= 256; d = %d", ix->d);
    if (mode == KNN_SEARCH_BF16 && !ix->b16_ok)
        KNN_FAIL(KNN_EINVAL, "bf16 search needs d >= 64; d = %d", ix->d);
    if (mode == KNN_SEARCH_I8 && ix->nblk8 <= 0)
        KNN_FAIL(KNN_EINVAL, "int8 search needs 64 <= d <= 4096; d = %d", ix->d);
    ix->mode = mode;
    return KNN_OK;
}

int knn_search_stats(knn_index_t* ix, int64_t* split_queries, int64_t* fallback_queries,
                     float* max_err_ratio) {
    return knn_search_stats2(ix, split_queries, fallback_queries, nullptr, max_err_ratio);
}

int knn_search_stats2(knn_index_t* ix, int64_t* split_queries, int64_t* fallback_queries,
                      int64_t* second_chance_queries, float* max_err_ratio) {
    if (!ix || !split_queries || !fallback_queries) KNN_FAIL(KNN_EINVAL, "NULL argument");
    if (ix->multi)
        return multi_search_stats(ix, split_queries, fallback_queries, second_chance_queries,
                                  max_err_ratio);
    IndexOp op(ix);
    int64_t first_fail = 0;
    *fallback_queries = 0;
    int rc = ix->stat_valid ? op.begin_host() : KNN_OK;     // (no candidate search yet: the GPU is not touched)
    if (rc == KNN_OK) rc = read_search_stats(ix, split_queries, fallback_queries, &first_fail, max_err_ratio);
    if (second_chance_queries) *second_chance_queries = first_fail - *fallback_queries;
    return op.finish_synced(rc);
}

int knn_last_path(const knn_index_t* ix) {
    if (!ix) return KNN_EINVAL;
    return ix->multi ? multi_last_path(ix) : ix->last_path;
}

// The count lives on the device (the large-k search never waits for the GPU): reading it waits
// for the index's last operation.
static int large_k_fallbacks_one(knn_index* ix, int64_t* n) {
    IndexOp op(ix);
    int rc = ix->lk_fail ? op.begin_host() : KNN_OK;
    if (rc == KNN_OK) rc = largek_fallbacks(ix, n);
    return op.finish_synced(rc);
}

int knn_large_k_fallbacks(const knn_index_t* cix, int64_t* n) {
    if (!cix || !n) KNN_FAIL(KNN_EINVAL, "NULL argument");
    knn_index* ix = const_cast<knn_index*>(cix);     // (only the fence state changes)
    if (!ix->multi) return large_k_fallbacks_one(ix, n);
    *n = 0;
    for (int s = 0; s < multi_num_shards(ix); ++s) {
        int64_t v = 0;
        const int rc = large_k_fallbacks_one(const_cast<knn_index*>(multi_shard(ix, s)), &v);
        if (rc != KNN_OK) return rc;
        *n += v;
    }
    return KNN_OK;
}

// knn_plan and knn_plan_kernel format what search_locked decides for a search's first chunk.
static_assert((int)Route::Exact == kModeF32 && (int)Route::Split == kModeSplit && (int)Route::B16 == kModeBF16,
              "knn_plan_kernel prints a generic tile's route as its kMode");

int knn_plan(const knn_index_t* cix, int64_t nq, int k, int* tr, int* tq, int* splits, int* wgs) {
    if (!cix || !tr || !tq || !splits || !wgs) KNN_FAIL(KNN_EINVAL, "NULL argument");
    const knn_index* ix = cix->multi ? multi_shard(cix, 0) : cix;
    const Plan p = choose_route(*ix, std::min(nq, kQueryChunk), k).plan;
    *tr = p.bm; *tq = p.bq;
    *splits = p.nsplit; *wgs = p.wgs;
    return KNN_OK;
}

int knn_plan_kernel(const knn_index_t* cix, int64_t nq, int k, char* name, int cap) {
    if (!cix || !name || cap < 1) KNN_FAIL(KNN_EINVAL, "NULL argument");
    const knn_index* ix = cix->multi ? multi_shard(cix, 0) : cix;
    const int l2 = ix->metric == KNN_METRIC_L2 ? 1 : 0;
    const RoutePlan rp = choose_route(*ix, std::min(nq, kQueryChunk), k);
    const Plan& p = rp.plan;
    if (rp.route == Route::I8)
        std::snprintf(name, cap, "knn_i8_scan_kernel<%d, %d, %d>", rp.i8_inst, p.km, (ix->nblk8 + 15) / 16);
    else if (p.big)
        std::snprintf(name, cap, "knn_b16w_tile_kernel%s<%d, %d, %s>",
                      ix->xt_state == TailCopy::Built && rp.tail_ok ? "_i8t" : "", p.km, l2,
                      p.ib > 0 ? "true" : "false");
    else       // (Route's values are the generic tile's kMode* arithmetic: Exact, Split, B16)
        std::snprintf(name, cap, "knn_tile_topk_kernel<%d, %d, ..., %d, ...>", p.wr, p.wq, (int)rp.route);
    return KNN_OK;
}

/* Read-only view of the int8 tail copy for tests (NULL outputs are skipped): the split column and
 * codes per row, and rows [i0, i0 + n) of the codes (n x dpt), scales (n) and statistics (n x 4).
 * KNN_EINVAL while the copy does not exist. */
int knn_debug_i8tail(knn_index_t* ix, int* head, int* dpt, int64_t i0, int64_t n, int8_t* codes,
                     float* scales, float* stats) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (ix->multi) KNN_FAIL(KNN_EINVAL, "knn_debug_i8tail: single-device indexes only");
    IndexOp op(ix);
    if (ix->xt_state != TailCopy::Built || !ix->xt) KNN_FAIL(KNN_EINVAL, "the index has no int8 tail copy");
    if (i0 < 0 || n < 0 || i0 + n > ix->ntotal) KNN_FAIL(KNN_EINVAL, "rows outside [0, ntotal)");
    if (head) *head = ix->xt_head;
    if (dpt) *dpt = ix->xt_dpt;
    int rc = op.begin_host();
    auto down = [&](void* dst, const void* src, size_t row) {
        if (rc == KNN_OK && dst && n > 0)
            rc = HipStreams::fail(hipMemcpyAsync(dst, (const char*)src + (size_t)i0 * row, (size_t)n * row,
                                                 hipMemcpyDeviceToHost, ix->stream), "hipMemcpyAsync");
    };
    // the codes are the first xt_dpt bytes of every joint row: a strided copy packs them
    if (rc == KNN_OK && codes && n > 0)
        rc = HipStreams::fail(hipMemcpy2DAsync(codes, (size_t)ix->xt_dpt,
                                               (const char*)ix->xt.get() + (size_t)i0 * ix->xt_row,
                                               (size_t)ix->xt_row, (size_t)ix->xt_dpt, (size_t)n,
                                               hipMemcpyDeviceToHost, ix->stream), "hipMemcpy2DAsync");
    down(scales, ix->xts.get(), sizeof(float));
    down(stats, ix->xtm.get(), sizeof(float4));
    return op.finish(rc);
}

/* Read-only view of the copy's raw joint rows for tests: *row_bytes = dpt + 2 head (a row is its dpt
 * tail codes, then its first head columns as bf16), and rows [i0, i0 + n) of them at `rows` (n x
 * row_bytes; NULL outputs are skipped).  KNN_EINVAL while the copy does not exist. */
int knn_debug_i8tail_rows(knn_index_t* ix, int64_t i0, int64_t n, int* row_bytes, uint8_t* rows) {
    if (!ix) KNN_FAIL(KNN_EINVAL, "index is NULL");
    if (ix->multi) KNN_FAIL(KNN_EINVAL, "knn_debug_i8tail_rows: single-device indexes only");
    IndexOp op(ix);
    if (ix->xt_state != TailCopy::Built || !ix->xt) KNN_FAIL(KNN_EINVAL, "the index has no int8 tail copy");
    if (i0 < 0 || n < 0 || i0 + n > ix->ntotal) KNN_FAIL(KNN_EINVAL, "rows outside [0, ntotal)");
    if (row_bytes) *row_bytes = ix->xt_row;
    int rc = op.begin_host();
    if (rc == KNN_OK && rows && n > 0)
        rc = HipStreams::fail(hipMemcpyAsync(rows, (const char*)ix->xt.get() + (size_t)i0 * ix->xt_row,
                                             (size_t)n * ix->xt_row, hipMemcpyDeviceToHost, ix->stream),
                              "hipMemcpyAsync");
    return op.finish(rc);
}

}  // extern "C"
