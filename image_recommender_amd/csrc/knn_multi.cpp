// knn_multi.cpp — one k-NN index over several HIP devices of one process (include/imgrec_knn.h
// knn_create_multi).  The reference's CLI is single-process (/root/reference/main/
// search_from_image.py:430-441, main/create_index.py:327-341), so this is how its own entry
// points use every GPU of a node without torchrun: the faiss-compatible index object is the same,
// its corpus lives in per-device row shards.
//
// Layout: every add of n rows is cut into ndev contiguous pieces, piece s appended to shard s;
// a shard keeps, per local row, its global label (device array `lmap`), so labels stay the
// reference's dense offsets whatever the add sizes.  Within a shard global labels grow with local
// rows, so a shard's (key, local row) order is the (key, label) order of the whole index.
//
// Search: the query batch reaches every shard's device (peer copy; none when the shard shares the
// first device), each shard runs the single-device search on its own stream concurrently, maps
// its labels, and its (nq, k) result lands in a [ndev][nq][k] gather buffer on the first device
// (peer copy over xGMI), where knn_merge's kernel produces the final rows.  The same shard merge as
// the torchrun path (sharded.py), with device-to-device copies instead of an RCCL all-gather.
#include <cstdlib>
#include <cstring>
#include <thread>
#include <utility>

#include "knn_multi.h"

struct knn_multi {
    std::vector<knn_index*> shards;
    std::vector<int> devices;
    struct Run { int64_t g0; int shard; int64_t l0; int64_t n; };
    std::vector<Run> runs;                       // global row ranges in increasing order
    struct Shard {                               // per shard, on its device
        DevBuf<int64_t> lmap;                    // local row -> label
        DevBuf<float> sq;                        // query copy (other devices only)
        DevBuf<float> sd;                        // results (other devices only)
        DevBuf<int64_t> si;
        DevBuf<uint8_t> sb;                      // bitmap copy (other devices only)
        DevBuf<float> sx;                        // row staging for add_device
        hipEvent_t done = nullptr;
    };
    std::vector<Shard> per;
    hipEvent_t ready = nullptr;                  // inputs ready on the first device
    // IMGREC_MULTI_FORCE_REMOTE=1 (tests): shards on the first device take the other devices'
    // staging + peer-copy path too, so one GPU exercises it
    bool force_remote = false;
    DevBuf<float> gD;                            // [ndev][nq][k] on the first device
    DevBuf<int64_t> gI;
};

namespace imgrec {

namespace {

knn_multi* M(const knn_index* ix) { return ix->multi; }

// shard s's piece of an add of n rows
inline int64_t piece0(int64_t n, int s, int ndev) { return n * s / ndev; }

// a label map that keeps its entries when it grows
int grow_keep(DevBuf<int64_t>& b, size_t need, hipStream_t st) {
    if (b.cap() >= need) return KNN_OK;
    DevBuf<int64_t> nb;
    const int rc = nb.reserve(std::max(need, b.cap() * 3 / 2));
    if (rc != KNN_OK) return rc;
    if (b) {
        const hipError_t e = hipMemcpyAsync(nb, b, b.cap() * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
        if (e2 != hipSuccess) KNN_FAIL(KNN_EHIP, "label map regrowth failed: %s", hipGetErrorString(e2));
    }
    b.swap(nb);                                  // (the old map goes with nb)
    return KNN_OK;
}

int append_runs(knn_index* ix, const std::vector<int64_t>& before, int64_t n) {
    knn_multi* m = M(ix);
    const int ndev = (int)m->shards.size();
    for (int s = 0; s < ndev; ++s) {
        const int64_t r0 = piece0(n, s, ndev), r1 = piece0(n, s + 1, ndev);
        if (r1 <= r0) continue;
        m->runs.push_back({ix->ntotal + r0, s, before[s], r1 - r0});
        knn_index* sh = m->shards[s];
        DeviceGuard g(sh->device);
        int rc;
        // lmap grows with the shard's capacity; rows already mapped keep their labels
        if ((rc = grow_keep(m->per[s].lmap, (size_t)sh->cap, sh->stream)) != KNN_OK)
            return rc;
        KNN_HIP(launch_iota64(m->per[s].lmap + before[s], r1 - r0, ix->ntotal + r0, sh->stream));
        KNN_HIP(hipStreamSynchronize(sh->stream));
    }
    ix->ntotal += n;
    return KNN_OK;
}

}  // namespace

int multi_create(int d, int metric, const int* devices, int ndev, knn_index** out) {
    *out = nullptr;
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0)
        KNN_FAIL(KNN_ENOSYS, "no HIP device visible");
    for (int s = 0; s < ndev; ++s)
        if (devices[s] < 0 || devices[s] >= visible)
            KNN_FAIL(KNN_EINVAL, "device %d out of range (%d visible)", devices[s], visible);
    knn_index* ix = nullptr;
    int rc = create_single(d, metric, devices[0], &ix);
    if (rc != KNN_OK) return rc;
    knn_multi* m = new knn_multi();
    ix->multi = m;
    m->devices.assign(devices, devices + ndev);
    if (const char* e = std::getenv("IMGREC_MULTI_FORCE_REMOTE")) m->force_remote = std::atoi(e) != 0;
    m->per.resize(ndev);
    {
        DeviceGuard g(ix->device);
        if (hipEventCreateWithFlags(&m->ready, hipEventDisableTiming) != hipSuccess) {
            multi_free(ix);
            KNN_FAIL(KNN_EHIP, "hipEventCreate failed");
        }
    }
    for (int s = 0; s < ndev; ++s) {
        knn_index* sh = nullptr;
        if ((rc = create_single(d, metric, devices[s], &sh)) != KNN_OK) {
            multi_free(ix);
            return rc;
        }
        m->shards.push_back(sh);
        DeviceGuard g(devices[s]);
        if (hipEventCreateWithFlags(&m->per[s].done, hipEventDisableTiming) != hipSuccess) {
            multi_free(ix);
            KNN_FAIL(KNN_EHIP, "hipEventCreate failed");
        }
        // peer access between the first device and every other (xGMI); already enabled or
        // unsupported is not an error here: peer copies then stage through the runtime
        if (devices[s] != devices[0]) {
            (void)hipDeviceEnablePeerAccess(devices[0], 0);
            DeviceGuard g0(devices[0]);
            (void)hipDeviceEnablePeerAccess(devices[s], 0);
            (void)hipGetLastError();
        }
    }
    *out = ix;
    return KNN_OK;
}

int multi_free(knn_index* ix) {
    knn_multi* m = M(ix);
    for (size_t s = 0; s < m->devices.size(); ++s) {
        DeviceGuard g(m->devices[s]);
        (void)hipDeviceSynchronize();
        if (m->per[s].done) (void)hipEventDestroy(m->per[s].done);
        m->per[s] = knn_multi::Shard();          // (its buffers, while the guard holds)
    }
    for (knn_index* sh : m->shards) free_single(sh);
    {
        DeviceGuard g(ix->device);
        if (m->ready) (void)hipEventDestroy(m->ready);
        delete m;                                // (the gather buffers, while the guard holds)
    }
    ix->multi = nullptr;
    free_single(ix);
    return KNN_OK;
}

int multi_reserve(knn_index* ix, int64_t n) {
    knn_multi* m = M(ix);
    std::lock_guard<std::mutex> lk(ix->mu);
    const int ndev = (int)m->shards.size();
    for (int s = 0; s < ndev; ++s) {
        // later adds are cut evenly: shard s ends up with about n / ndev rows
        int rc = knn_reserve(m->shards[s], (n + ndev - 1) / ndev + 1);
        if (rc != KNN_OK) return rc;
    }
    return KNN_OK;
}

int multi_add(knn_index* ix, const float* x, int64_t n) {
    knn_multi* m = M(ix);
    std::lock_guard<std::mutex> lk(ix->mu);
    const int ndev = (int)m->shards.size();
    std::vector<int64_t> before(ndev);
    for (int s = 0; s < ndev; ++s) {
        before[s] = m->shards[s]->ntotal;
        const int64_t r0 = piece0(n, s, ndev), r1 = piece0(n, s + 1, ndev);
        if (r1 <= r0) continue;
        int rc = knn_add(m->shards[s], x + r0 * ix->d, r1 - r0);
        if (rc != KNN_OK) return rc;
    }
    return append_runs(ix, before, n);
}

int multi_add_device(knn_index* ix, const float* x, int64_t n, hipStream_t st) {
    knn_multi* m = M(ix);
    std::lock_guard<std::mutex> lk(ix->mu);
    const int ndev = (int)m->shards.size();
    int rc;
    {
        DeviceGuard g(ix->device);
        KNN_HIP(hipEventRecord(m->ready, st));       // the rows are written on the caller's stream
    }
    std::vector<int64_t> before(ndev);
    for (int s = 0; s < ndev; ++s) {
        knn_index* sh = m->shards[s];
        before[s] = sh->ntotal;
        const int64_t r0 = piece0(n, s, ndev), r1 = piece0(n, s + 1, ndev);
        if (r1 <= r0) continue;
        const float* src = x + r0 * ix->d;
        if (sh->device == ix->device && !m->force_remote) {
            if ((rc = knn_add_device(sh, src, r1 - r0, st)) != KNN_OK) return rc;
            continue;
        }
        DeviceGuard g(sh->device);
        const size_t bytes = (size_t)(r1 - r0) * ix->d * sizeof(float);
        if ((rc = m->per[s].sx.reserve((size_t)(r1 - r0) * ix->d)) != KNN_OK) return rc;
        KNN_HIP(hipStreamWaitEvent(sh->stream, m->ready, 0));
        KNN_HIP(hipMemcpyPeerAsync(m->per[s].sx, sh->device, src, ix->device, bytes, sh->stream));
        if ((rc = knn_add_device(sh, m->per[s].sx, r1 - r0, sh->stream)) != KNN_OK) return rc;
        // the caller may reuse x once its stream passes this point
        KNN_HIP(hipEventRecord(m->per[s].done, sh->stream));
        KNN_HIP(hipStreamWaitEvent(st, m->per[s].done, 0));
    }
    return append_runs(ix, before, n);
}

int multi_reset(knn_index* ix) {
    knn_multi* m = M(ix);
    std::lock_guard<std::mutex> lk(ix->mu);
    for (knn_index* sh : m->shards) {
        int rc = knn_reset(sh);
        if (rc != KNN_OK) return rc;
    }
    m->runs.clear();
    ix->ntotal = 0;
    return KNN_OK;
}

// Removal.  The host has the bitmap, so everything a shard cannot derive from its own rows is
// computed here: the bitmap as 32-bit words (bits at and past nbits cleared) and the words'
// exclusive popcount prefix.  Every shard gets both, compacts its rows and its label map with the
// bit of each row's label (remove_rows_locked through lmap), and renumbers the surviving labels:
// new = old - (set bits below old).  A run's survivors stay contiguous in labels and in local rows
// (labels become dense again), so every old run maps to at most one new run.
int multi_remove_ids(knn_index* ix, const uint8_t* bitmap, int64_t nbits, int64_t* nremoved) {
    knn_multi* m = M(ix);
    std::lock_guard<std::mutex> lk(ix->mu);
    *nremoved = 0;
    nbits = std::min(nbits, ix->ntotal);
    if (nbits <= 0) return KNN_OK;
    const size_t nw = (size_t)((nbits + 31) / 32), nbytes = (size_t)((nbits + 7) / 8);
    std::vector<uint32_t> words(nw, 0u), pref(nw + 1, 0u);
    std::memcpy(words.data(), bitmap, nbytes);
    if (nbits & 31) words[nw - 1] &= (1u << (int)(nbits & 31)) - 1u;
    for (size_t w = 0; w < nw; ++w) pref[w + 1] = pref[w] + (uint32_t)__builtin_popcount(words[w]);
    const int64_t removed = (int64_t)pref[nw];
    if (removed == 0) return KNN_OK;
    // set bits below label g
    auto below = [&](int64_t g) -> int64_t {
        if (g >= nbits) return removed;
        return (int64_t)pref[(size_t)(g >> 5)] +
               __builtin_popcount(words[(size_t)(g >> 5)] & ((1u << (int)(g & 31)) - 1u));
    };
    int rc;
    for (size_t s = 0; s < m->shards.size(); ++s) {
        knn_index* sh = m->shards[s];
        if (sh->ntotal == 0) continue;
        IndexOp ops(sh);
        const hipStream_t ss = sh->stream;
        if ((rc = ops.begin_host()) != KNN_OK) return rc;
        if ((rc = sh->ft_bits.reserve(nw * 4)) != KNN_OK) return rc;
        if ((rc = sh->rm_pref.reserve(nw)) != KNN_OK) return rc;
        KNN_HIP(hipMemcpyAsync(sh->ft_bits, words.data(), nw * 4, hipMemcpyHostToDevice, ss));
        KNN_HIP(hipMemcpyAsync(sh->rm_pref, pref.data(), nw * 4, hipMemcpyHostToDevice, ss));
        int64_t gone = 0;
        if ((rc = remove_rows_locked(sh, sh->ft_bits, nbits, m->per[s].lmap, m->per[s].lmap, ss, &gone)) != KNN_OK)
            return rc;
        KNN_HIP(launch_renumber_labels(m->per[s].lmap, sh->ntotal,
                                       reinterpret_cast<const uint32_t*>(sh->ft_bits.get()),
                                       sh->rm_pref, nbits, removed, ss));
        if ((rc = ops.finish(KNN_OK)) != KNN_OK) return rc;
    }
    std::vector<knn_multi::Run> runs;
    std::vector<int64_t> local(m->shards.size(), 0);
    for (const auto& r : m->runs) {
        const int64_t b0 = below(r.g0), keep = r.n - (below(r.g0 + r.n) - b0);
        if (keep > 0) runs.push_back({r.g0 - b0, r.shard, local[r.shard], keep});
        local[r.shard] += keep;
    }
    m->runs.swap(runs);
    ix->ntotal -= removed;
    *nremoved = removed;
    return KNN_OK;
}

int multi_reconstruct_n(knn_index* ix, int64_t i0, int64_t n, float* x) {
    knn_multi* m = M(ix);
    std::lock_guard<std::mutex> lk(ix->mu);
    const int64_t i1 = i0 + n;
    for (const auto& r : m->runs) {
        const int64_t a = std::max(i0, r.g0), b = std::min(i1, r.g0 + r.n);
        if (a >= b) continue;
        int rc = knn_reconstruct_n(m->shards[r.shard], r.l0 + (a - r.g0), b - a, x + (a - i0) * ix->d);
        if (rc != KNN_OK) return rc;
    }
    return KNN_OK;
}

namespace {

// Every shard searches q (device pointer on the first device, ready when m->ready fires) into the
// gather buffer; the first device's stream `st` then merges into D, I.  With `filtered`, the
// search among the rows the bitmap `bits` (first device, global rows; nbits <= ntotal) selects.
int fan_out_search(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                   hipStream_t st, bool filtered = false, const uint8_t* bits = nullptr,
                   int64_t nbits = 0) {
    knn_multi* m = M(ix);
    const int ndev = (int)m->shards.size();
    const size_t nk = (size_t)nq * k;
    if (ix->ntotal == 0 || (filtered && nbits == 0)) {       // no row to search: the empty rows
        KNN_HIP(launch_fill_empty(D, I, nq * (int64_t)k, ix->metric == KNN_METRIC_L2 ? 1 : 0, st));
        return KNN_OK;
    }
    // the k > KNN_MAX_K merges pack a label into 32 bits (include/imgrec_knn.h knn_merge_device)
    if (k > KNN_MAX_K && ix->ntotal + ix->id_offset > (int64_t(1) << 32))
        KNN_FAIL(KNN_EINVAL, "k = %d > %d over shards: labels must stay below 2^32, ntotal + id_offset = %lld",
                 k, KNN_MAX_K, (long long)(ix->ntotal + ix->id_offset));
    int rc;                                      // (the caller's scope has set the first device)
    if ((rc = m->gD.reserve(nk * ndev)) != KNN_OK) return rc;
    if ((rc = m->gI.reserve(nk * ndev)) != KNN_OK) return rc;
    KNN_HIP(hipEventRecord(m->ready, st));
    for (int s = 0; s < ndev; ++s) {
        knn_index* sh = m->shards[s];
        const bool local = sh->device == ix->device && !m->force_remote;
        IndexOp ops(sh);
        const hipStream_t ss = sh->stream;
        KNN_HIP(hipStreamWaitEvent(ss, m->ready, 0));
        if ((rc = ops.begin(ss)) != KNN_OK) return rc;
        const float* qs = q;
        float* ds = m->gD + s * nk;
        int64_t* is = m->gI + s * nk;
        if (!local) {
            if ((rc = m->per[s].sq.reserve((size_t)nq * ix->d)) != KNN_OK) return rc;
            if ((rc = m->per[s].sd.reserve(nk)) != KNN_OK) return rc;
            if ((rc = m->per[s].si.reserve(nk)) != KNN_OK) return rc;
            KNN_HIP(hipMemcpyPeerAsync(m->per[s].sq, sh->device, q, ix->device,
                                       (size_t)nq * ix->d * sizeof(float), ss));
            qs = m->per[s].sq;
            ds = m->per[s].sd;
            is = m->per[s].si;
        }
        if (filtered) {
            const uint8_t* bs = bits;
            const size_t nbytes = (size_t)((nbits + 7) / 8);
            if (!local && nbytes) {
                if ((rc = m->per[s].sb.reserve(nbytes)) != KNN_OK) return rc;
                KNN_HIP(hipMemcpyPeerAsync(m->per[s].sb, sh->device, bits, ix->device, nbytes, ss));
                bs = m->per[s].sb;
            }
            rc = filtered_search_locked(sh, qs, nq, k, bs, nbits, m->per[s].lmap, ds, is, ss);
        } else {
            rc = search_locked(sh, qs, nq, k, ds, is, ss);
        }
        if (rc != KNN_OK) return rc;
        KNN_HIP(launch_map_labels(is, (int64_t)nk, m->per[s].lmap, ix->id_offset, ss));
        if (!local) {
            KNN_HIP(hipMemcpyPeerAsync(m->gD + s * nk, ix->device, ds, sh->device,
                                       nk * sizeof(float), ss));
            KNN_HIP(hipMemcpyPeerAsync(m->gI + s * nk, ix->device, is, sh->device,
                                       nk * sizeof(int64_t), ss));
        }
        if ((rc = ops.finish(KNN_OK)) != KNN_OK) return rc;
        KNN_HIP(hipEventRecord(m->per[s].done, ss));
    }
    for (int s = 0; s < ndev; ++s) KNN_HIP(hipStreamWaitEvent(st, m->per[s].done, 0));
    const int kmetric = ix->metric == KNN_METRIC_L2 ? 1 : 0;
    if (k > KNN_MAX_K) {
        KNN_HIP(launch_merge_any(m->gD, m->gI, ndev, nq, k, (int64_t)nk, (int64_t)nk, k, kmetric, D, I, st));
        return KNN_OK;
    }
    KNN_HIP(launch_merge(m->gD, m->gI, nq, ndev, k, k, (int64_t)nk, k, kmetric, kmetric ? 0 : 1, D, I,
                         st));
    return KNN_OK;
}

}  // namespace

int multi_search_device(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                        hipStream_t st) {
    IndexOp op(ix);
    int rc = op.begin(st);
    if (rc == KNN_OK) rc = fan_out_search(ix, q, nq, k, D, I, st);
    return op.finish(rc);
}

int multi_search(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I) {
    IndexOp op(ix);
    int rc = op.begin_host();
    if (rc == KNN_OK) rc = stage_queries(ix, q, nq, k);        // (pageable copies: knn_search's pinned path is not taken)
    if (rc == KNN_OK) rc = fan_out_search(ix, ix->hq, nq, k, ix->hd, ix->hi, ix->stream);
    if (rc == KNN_OK) rc = fetch_results(ix, nq, k, D, I);
    return op.finish(rc);
}

int multi_search_filtered(knn_index* ix, const float* q, bool q_on_host, int64_t nq, int k,
                          const uint8_t* bitmap, int64_t nbits, float* D, int64_t* I, hipStream_t st) {
    IndexOp op(ix);
    int rc = q_on_host ? op.begin_host() : op.begin(st);
    if (rc == KNN_OK && q_on_host) rc = stage_queries(ix, q, nq, k);
    if (rc == KNN_OK && q_on_host) rc = stage_bitmap(ix, bitmap, &nbits);
    if (rc != KNN_OK) return rc;
    nbits = std::min(nbits, ix->ntotal);         // bits at or past ntotal are ignored
    rc = q_on_host ? fan_out_search(ix, ix->hq, nq, k, ix->hd, ix->hi, op.stream(), true, ix->ft_bits, nbits)
                   : fan_out_search(ix, q, nq, k, D, I, st, true, bitmap, nbits);
    if (rc == KNN_OK && q_on_host) rc = fetch_results(ix, nq, k, D, I);
    return op.finish(rc);
}

// Range search: every shard runs the single-device range search on its own device and stream, one
// host thread each (a shard's search waits for its own result size), maps its labels and copies
// its result to the host; the segments of a query (each already in (key, label) order, labels
// disjoint) are merged there and the merged result is uploaded to the first device.  A pair's key
// does not depend on the shard it sits in, so the result equals the single-device one bit for bit.
int multi_range_search(knn_index* ix, const float* q, bool q_on_host, int64_t nq, float radius,
                       hipStream_t st, knn_range_result** out) {
    knn_multi* m = M(ix);
    IndexOp op(ix);
    const int ndev = (int)m->shards.size();
    int rc = q_on_host ? op.begin_host() : op.begin(st);
    if (rc != KNN_OK) return rc;
    st = op.stream();
    if (q_on_host && nq > 0) {
        if ((rc = stage_queries(ix, q, nq, 0)) != KNN_OK) return rc;
        q = ix->hq;
    }
    KNN_HIP(hipEventRecord(m->ready, st));
    struct ShardHits {
        std::vector<int64_t> lims;
        std::vector<float> D;
        std::vector<int64_t> I;
        int rc = KNN_OK;
        std::string err;
    };
    std::vector<ShardHits> hits(ndev);
    auto run_shard = [&](int s) -> int {
        knn_index* sh = m->shards[s];
        ShardHits& h = hits[s];
        const bool local = sh->device == ix->device && !m->force_remote;
        IndexOp ops(sh);
        const hipStream_t ss = sh->stream;
        int r;
        KNN_HIP(hipStreamWaitEvent(ss, m->ready, 0));
        if ((r = ops.begin_host()) != KNN_OK) return r;
        const float* qs = q;
        if (!local && nq > 0) {
            if ((r = m->per[s].sq.reserve((size_t)nq * ix->d)) != KNN_OK) return r;
            KNN_HIP(hipMemcpyPeerAsync(m->per[s].sq, sh->device, q, ix->device,
                                       (size_t)nq * ix->d * sizeof(float), ss));
            qs = m->per[s].sq;
        }
        knn_range_result* res = nullptr;
        if ((r = range_search_locked(sh, qs, nq, radius, ss, &res)) != KNN_OK) return r;
        const int64_t n = res->size;
        h.lims.resize((size_t)nq + 1);
        h.D.resize((size_t)n);
        h.I.resize((size_t)n);
        hipError_t e = hipSuccess;
        if (n > 0) e = launch_map_labels(res->I, n, m->per[s].lmap, ix->id_offset, ss);
        if (e == hipSuccess)
            e = hipMemcpyAsync(h.lims.data(), res->lims, ((size_t)nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ss);
        if (e == hipSuccess && n > 0)
            e = hipMemcpyAsync(h.D.data(), res->D, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ss);
        if (e == hipSuccess && n > 0)
            e = hipMemcpyAsync(h.I.data(), res->I, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, ss);
        const hipError_t e2 = hipStreamSynchronize(ss);
        range_result_free(res);
        if (e != hipSuccess || e2 != hipSuccess)
            KNN_FAIL(KNN_EHIP, "range search shard %d: %s", s, hipGetErrorString(e != hipSuccess ? e : e2));
        return ops.finish_synced(KNN_OK);
    };
    {
        std::vector<std::thread> th;
        for (int s = 0; s < ndev; ++s)
            th.emplace_back([&, s]() {
                hits[s].rc = run_shard(s);
                if (hits[s].rc != KNN_OK) hits[s].err = last_error();   // the message is per thread
            });
        for (std::thread& t : th) t.join();
    }
    for (int s = 0; s < ndev; ++s)
        if (hits[s].rc != KNN_OK) KNN_FAIL(hits[s].rc, "%s", hits[s].err.c_str());
    // per query: the shards' sorted segments into one (key, label) order
    const bool l2 = ix->metric == KNN_METRIC_L2;
    std::vector<int64_t> lims((size_t)nq + 1, 0);
    for (int64_t i = 0; i < nq; ++i) {
        int64_t c = 0;
        for (int s = 0; s < ndev; ++s) c += hits[s].lims[i + 1] - hits[s].lims[i];
        lims[i + 1] = lims[i] + c;
    }
    std::vector<float> D((size_t)lims[nq]);
    std::vector<int64_t> I((size_t)lims[nq]);
    // the device sort's key: the order-preserving bits of the key (wave_ops.h key_bits_ordered)
    auto key_bits = [](float k) {
        uint32_t u;
        std::memcpy(&u, &k, sizeof u);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    };
    std::vector<std::pair<std::pair<uint32_t, int64_t>, float>> seg;
    for (int64_t i = 0; i < nq; ++i) {
        seg.clear();
        for (int s = 0; s < ndev; ++s)
            for (int64_t e = hits[s].lims[i]; e < hits[s].lims[i + 1]; ++e) {
                const float d = hits[s].D[e];
                seg.push_back({{key_bits(l2 ? d : -d), hits[s].I[e]}, d});
            }
        std::sort(seg.begin(), seg.end());
        for (size_t e = 0; e < seg.size(); ++e) {
            D[(size_t)lims[i] + e] = seg[e].second;
            I[(size_t)lims[i] + e] = seg[e].first.second;
        }
    }
    // (the upload synchronises st: the host form has nothing left to wait for)
    return op.finish_synced(range_result_from_host(ix->device, nq, lims.data(), D.data(), I.data(), st, out));
}

int multi_set_metric(knn_index* ix, int metric) {
    ix->metric = metric;
    for (knn_index* sh : M(ix)->shards) sh->metric = metric;
    return KNN_OK;
}

int multi_set_trained(knn_index* ix, bool trained) {
    for (knn_index* sh : M(ix)->shards) sh->trained = trained;
    ix->trained = trained;
    return KNN_OK;
}

int multi_set_timing(knn_index* ix, int enable) {
    for (knn_index* sh : M(ix)->shards) {
        int rc = knn_set_timing(sh, enable);
        if (rc != KNN_OK) return rc;
    }
    return KNN_OK;
}

int multi_kernel_time(knn_index* ix, double* total_ms, int* launches) {
    double tot = 0.0;
    int n = 0;
    for (knn_index* sh : M(ix)->shards) {
        double t = 0.0;
        int l = 0;
        int rc = knn_kernel_time(sh, &t, &l);
        if (rc != KNN_OK) return rc;
        tot += t;
        n += l;
    }
    *total_ms = tot;
    *launches = n;
    return KNN_OK;
}

int multi_set_fence_mode(knn_index* ix, int mode) {
    for (knn_index* sh : M(ix)->shards) {
        std::lock_guard<std::mutex> lk(sh->mu);
        sh->fence.lazy = mode == KNN_FENCE_LAZY;
    }
    return KNN_OK;
}

int multi_set_search_mode(knn_index* ix, int mode) {
    for (knn_index* sh : M(ix)->shards) {
        int rc = knn_set_search_mode(sh, mode);
        if (rc != KNN_OK) return rc;
    }
    ix->mode = mode;
    return KNN_OK;
}

// queries on a candidate path: every query runs on every shard, so the largest shard count;
// re-runs and second chances: summed over shards (one query can count once per shard)
int multi_search_stats(knn_index* ix, int64_t* split_q, int64_t* fallback_q, int64_t* second_q,
                       float* ratio) {
    *split_q = 0;
    *fallback_q = 0;
    if (second_q) *second_q = 0;
    if (ratio) *ratio = 0.f;
    for (knn_index* sh : M(ix)->shards) {
        int64_t a = 0, b = 0, c = 0;
        float r = 0.f;
        int rc = knn_search_stats2(sh, &a, &b, &c, &r);
        if (rc != KNN_OK) return rc;
        *split_q = std::max(*split_q, a);
        *fallback_q += b;
        if (second_q) *second_q += c;
        if (ratio) *ratio = std::max(*ratio, r);
    }
    return KNN_OK;
}

int multi_last_path(const knn_index* ix) { return M(ix)->shards[0]->last_path; }

const knn_index* multi_shard(const knn_index* ix, int s) { return M(ix)->shards[s]; }

int multi_num_shards(const knn_index* ix) { return (int)M(ix)->shards.size(); }

}  // namespace imgrec

extern "C" {

int knn_create_multi(int d, int metric, const int* devices, int ndev, knn_index_t** out) {
    if (!out) KNN_FAIL(KNN_EINVAL, "out is NULL");
    *out = nullptr;
    if (d <= 0) KNN_FAIL(KNN_EINVAL, "d must be positive (got %d)", d);
    if (metric != KNN_METRIC_L2 && metric != KNN_METRIC_IP && metric != KNN_METRIC_COSINE)
        KNN_FAIL(KNN_EINVAL, "unknown metric %d", metric);
    if (!devices || ndev <= 0 || ndev > 64) KNN_FAIL(KNN_EINVAL, "need 1..64 devices (got %d)", ndev);
    return imgrec::multi_create(d, metric, devices, ndev, out);
}

int knn_num_shards(const knn_index_t* ix) {
    if (!ix) return KNN_EINVAL;
    return ix->multi ? imgrec::multi_num_shards(ix) : 1;
}

}  // extern "C"
