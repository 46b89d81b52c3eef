// knn_kmeans.hip — Lloyd k-means (faiss Clustering::train; include/imgrec_kmeans.h).
//
// One step (kmeans_step_device) is six launches on the caller's stream, none of which waits:
//   1. kmeans_norms_kernel      |c|^2 of the k centroids (rows_tile.h row_norms).
//   2. kmeans_assign_kernel     the row tile of rows_tile.h with the centroids as the rows: a lane
//                               keeps a running (key, id) minimum per point over the stream's keys,
//                               fmaf(-2, x.c, |c|^2) or -x.c.  Then the waves' minima meet in LDS,
//                               the distance to the chosen centroid is summed directly (four points
//                               at a time per wave), and the workgroup's 128 distances are added in
//                               float64 in point order into partial[block].
//   3. kmeans_obj_kernel        the partials, strided over 256 threads and then in thread order.
//   4. rocPRIM radix_sort_pairs (assign, point index) on ceil(log2 k) key bits: stable, so a
//                               cluster's members are in ascending point index.
//   5. kmeans_offsets_kernel    segment offsets by binary search (counts), kmeans_parts_kernel their
//                               exclusive scan in parts of P members.
//   6. kmeans_partsum_kernel    one part per thread group, a thread per column (gathered rows are
//                               read coalesced), members added in order; kmeans_combine_kernel adds
//                               a cluster's part sums in part order and divides.
//
// Determinism.  Keys: rows_tile.h's argument, so two bitwise-equal centroid rows give bitwise-equal
// keys and the smaller id wins: the (key, id) comparison is lexicographic at every level.
// The update's summation tree depends on P alone: not on the grid, not on dispatch order.
//
// kmeans_assign_kernel: the tile's 55 KB of LDS (the waves' minima and the workgroup's results reuse
// the stage buffer after the stream), 184 VGPRs: two waves per SIMD, one workgroup per CU.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <unordered_set>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "../../include/imgrec_kmeans.h"
#include "dev_workspace.h"
#include "rows_tile.h"

namespace imgrec {
namespace {

constexpr int kPartDefault = 256;       // members per part of the segmented sum
constexpr float kSplitEps = 1.0f / 1024.0f;

__device__ __forceinline__ void take_min(float& bk, int& bi, float k, int i) {
    if (key_less(k, i, bk, bi)) { bk = k; bi = i; }
}

__global__ void __launch_bounds__(256)
kmeans_norms_kernel(const float* __restrict__ c, int k, int d, float* __restrict__ out) {
    row_norms(c, k, d, out);
}

__global__ void __launch_bounds__(kNT)
kmeans_assign_kernel(const float* __restrict__ x, int64_t n, int d, const float* __restrict__ c,
                     const float* __restrict__ cn, int k, int spherical, int vec_x, int vec_c,
                     int* __restrict__ assign, float* __restrict__ dist, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float stage[kRows * kLDK];
    __shared__ float cns[kBN];
    // after the last stage the buffer holds the waves' minima and the workgroup's results
    float* const redk = stage;                                        // [4][kBM]
    int* const redi = reinterpret_cast<int*>(stage + 4 * kBM);         // [4][kBM]
    int* const s_as = reinterpret_cast<int*>(stage + 8 * kBM);         // [kBM]
    float* const s_d = stage + 9 * kBM;                                // [kBM]
    static_assert(10 * kBM <= kRows * kLDK, "results fit the stage buffer");

    const RowLanes t;
    const int tid = t.tid, lane = t.lane, wave = t.wave, lr = t.lr, lh = t.lh, wc = t.wc, wp = t.wp;
    const int64_t p0 = (int64_t)blockIdx.x * kBM;
    float bk[2] = {INFINITY, INFINITY};
    int bi[2] = {INT32_MAX, INT32_MAX};
    rows_stream(t, stage, cns, x, n, d, c, cn, k, vec_x, vec_c,
                [&](int b, float dot, float cnv, int cid) __attribute__((always_inline)) {
                    take_min(bk[b], bi[b], spherical ? -dot : fmaf(-2.f, dot, cnv), cid);
                });

    // the two halves of a wave, then the four waves that share the points
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float ok = __shfl_xor(bk[b], 32);
        const int oi = __shfl_xor(bi[b], 32);
        take_min(bk[b], bi[b], ok, oi);
        if (lh == 0) {
            redk[wc * kBM + wp * 64 + b * 32 + lr] = bk[b];
            redi[wc * kBM + wp * 64 + b * 32 + lr] = bi[b];
        }
    }
    __syncthreads();
    if (tid < kBM) {
        float fk = redk[tid];
        int fi = redi[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) take_min(fk, fi, redk[w * kBM + tid], redi[w * kBM + tid]);
        if (fi < 0 || fi >= k) fi = 0;       // every key NaN: cluster 0
        s_as[tid] = fi;
        if (p0 + tid < n) assign[p0 + tid] = fi;
    }
    __syncthreads();
    // the distance to the chosen centroid, summed directly: kBM / 8 points per wave, four at a time
    // (their loads are independent), lanes over columns, a fixed butterfly
    constexpr int PW = kBM / (kNT / 64);
#pragma unroll 1
    for (int pp = 0; pp < PW; pp += 4) {
        const float* xr[4];
        const float* cr[4];
        float sum[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pl = wave * PW + pp + q;
            const int64_t p = min(p0 + pl, n - 1);            // a clamped row is computed, not written
            xr[q] = x + p * (int64_t)d;
            cr[q] = c + (int64_t)s_as[pl] * d;
            sum[q] = 0.f;
        }
        for (int j = lane; j < d; j += 64) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float xv = xr[q][j], cv = cr[q][j];
                if (spherical) {
                    sum[q] = fmaf(xv, cv, sum[q]);
                } else {
                    const float t = xv - cv;
                    sum[q] = fmaf(t, t, sum[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sum[q] = wave_sum(sum[q]);
            const int pl = wave * PW + pp + q;
            const bool live = p0 + pl < n;
            if (lane == 0) {
                if (live) dist[p0 + pl] = sum[q];
                s_d[pl] = live ? sum[q] : 0.f;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < kBM; ++i) t += (double)s_d[i];
        partial[blockIdx.x] = t;
    }
}

// obj = the partials: thread t adds partial[t], partial[t + 256], ... and thread 0 adds the 256 sums
__global__ void __launch_bounds__(256)
kmeans_obj_kernel(const double* __restrict__ partial, int64_t nb, double* __restrict__ obj) {
    __shared__ double sh[256];
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < nb; i += 256) t += partial[i];
    sh[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += sh[i];
        *obj = s;
    }
}

// off[c] = the first sorted position with key >= c (c = 0 .. k), counts[c] = off[c + 1] - off[c]
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__global__ void __launch_bounds__(256)
kmeans_offsets_kernel(const uint32_t* __restrict__ keys, uint32_t n, int k, uint32_t* __restrict__ off,
                      int64_t* __restrict__ counts) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > k) return;
    const uint32_t lo = lower_bound_u32(keys, n, (uint32_t)c);
    off[c] = lo;
    if (c < k) counts[c] = (int64_t)lower_bound_u32(keys, n, (uint32_t)c + 1) - (int64_t)lo;
}

// pstart[c] = the parts of the clusters before c (c = 0 .. k): one workgroup, a contiguous span of
// clusters per thread
__global__ void __launch_bounds__(256)
kmeans_parts_kernel(const uint32_t* __restrict__ off, int k, uint32_t P, uint32_t* __restrict__ pstart) {
    __shared__ uint32_t tot[256];
    const int span = (k + 255) / 256, c0 = threadIdx.x * span, c1 = min(k, c0 + span);
    uint32_t s = 0;
    for (int c = c0; c < c1; ++c) s += (off[c + 1] - off[c] + P - 1) / P;
    tot[threadIdx.x] = s;
    __syncthreads();
    uint32_t base = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) base += tot[t];
    for (int c = c0; c < c1; ++c) {
        pstart[c] = base;
        base += (off[c + 1] - off[c] + P - 1) / P;
    }
    if (c1 == k) pstart[k] = base;            // every thread at or past the end holds the same total
}

// psum[q] = the sum of part q's member rows, members in sorted (ascending point) order.  A workgroup
// serves ppb parts, a thread one column of one part (columns dcols apart when d > 256).
__global__ void __launch_bounds__(256)
kmeans_partsum_kernel(const float* __restrict__ x, int d, const uint32_t* __restrict__ idx,
                      const uint32_t* __restrict__ off, const uint32_t* __restrict__ pstart, int k,
                      uint32_t P, int dcols, int ppb, float* __restrict__ psum) {
    const int pl = threadIdx.x / dcols, col0 = threadIdx.x - pl * dcols;
    if (pl >= ppb) return;
    const uint32_t q = blockIdx.x * (uint32_t)ppb + pl;
    if (q >= pstart[k]) return;
    // the cluster of part q: the last c with pstart[c] <= q (empty clusters share a start)
    uint32_t lo = 0, hi = (uint32_t)k;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pstart[mid] <= q) lo = mid;
        else hi = mid;
    }
    const uint32_t cl = lo;
    const uint32_t m0 = off[cl] + (q - pstart[cl]) * P, m1 = min(m0 + P, off[cl + 1]);
    for (int col = col0; col < d; col += dcols) {
        float s = x[(int64_t)idx[m0] * d + col];
        for (uint32_t m = m0 + 1; m < m1; ++m) s += x[(int64_t)idx[m] * d + col];
        psum[(int64_t)q * d + col] = s;
    }
}

// new centroid = (its part sums in part order) / count; an empty cluster keeps the old row
__global__ void __launch_bounds__(256)
kmeans_combine_kernel(const float* __restrict__ psum, const uint32_t* __restrict__ off,
                      const uint32_t* __restrict__ pstart, int d, const float* __restrict__ oldc,
                      float* __restrict__ newc) {
    const int cl = blockIdx.x;
    const uint32_t cnt = off[cl + 1] - off[cl], q0 = pstart[cl], q1 = pstart[cl + 1];
    for (int col = threadIdx.x; col < d; col += 256) {
        const int64_t o = (int64_t)cl * d + col;
        if (cnt == 0) {
            newc[o] = oldc[o];
            continue;
        }
        float s = psum[(int64_t)q0 * d + col];
        for (uint32_t q = q0 + 1; q < q1; ++q) s += psum[(int64_t)q * d + col];
        newc[o] = (float)((double)s / (double)cnt);
    }
}

// the (ci, cj) pairs of a repair, in order: a thread owns one column of every row, so later pairs
// see earlier ones
__global__ void __launch_bounds__(256)
kmeans_split_kernel(float* __restrict__ c, int d, const int* __restrict__ pairs, int npairs) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    const float up = 1.f + kSplitEps, dn = 1.f - kSplitEps;
    const float fi = (col & 1) ? dn : up, fj = (col & 1) ? up : dn;
    for (int p = 0; p < npairs; ++p) {
        const int64_t ci = pairs[2 * p], cj = pairs[2 * p + 1];
        const float v = c[cj * d + col];
        c[ci * d + col] = v * fi;
        c[cj * d + col] = v * fj;
    }
}

// rows L2-normalised in place (rows of norm 0 unchanged), one wave per row
__global__ void __launch_bounds__(256)
kmeans_normalize_kernel(float* __restrict__ c, int k, int d) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= k) return;
    float* p = c + (int64_t)row * d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) s = fmaf(p[j], p[j], s);
    s = wave_sum(s);
    if (s > 0.f) {
        const float inv = 1.f / sqrtf(s);
        for (int j = lane; j < d; j += 64) p[j] *= inv;
    }
}

// dst row r = src row rows[r]
__global__ void __launch_bounds__(256)
kmeans_gather_kernel(const float* __restrict__ src, int d, const int64_t* __restrict__ rows,
                     float* __restrict__ dst) {
    const int64_t r = rows[blockIdx.x];
    for (int col = threadIdx.x; col < d; col += 256) dst[(int64_t)blockIdx.x * d + col] = src[r * d + col];
}

// ---- host side ----------------------------------------------------------------------------------

// what a step's launches share (dev_workspace.h: one per device)
struct Workspace : StreamHandoff {
    DevBuf<float> cnorm;
    DevBuf<double> partial;
    DevBuf<uint32_t> skey;
    DevBuf<uint32_t> sidx;
    DevBuf<uint32_t> off;
    DevBuf<uint32_t> pstart;
    DevBuf<float> psum;
    DevBuf<int> pairs;
    DevBuf<char> tmp;
};

int check_step_args(const void* x, int64_t n, int d, const void* c, int k, const char* who) {
    if (d <= 0) KNN_FAIL(KNN_EINVAL, "%s: d must be positive (got %d)", who, d);
    if (k <= 0) KNN_FAIL(KNN_EINVAL, "%s: k must be positive (got %d)", who, k);
    if (n < k)
        KNN_FAIL(KNN_EINVAL, "%s: Number of training points (%lld) should be at least as large as number "
                             "of clusters (%d)", who, (long long)n, k);
    if (n >= (int64_t(1) << 31)) KNN_FAIL(KNN_EINVAL, "%s: n = %lld rows (limit 2^31 - 1)", who, (long long)n);
    if (!x || !c) KNN_FAIL(KNN_EINVAL, "%s: NULL points or centroids", who);
    if (!row_stages_fit(k, d)) KNN_FAIL(KNN_EINVAL, "%s: k x d too large (%d x %d)", who, k, d);
    return KNN_OK;
}

uint32_t part_size() {
    if (const char* e = test_knob("IMGREC_KMEANS_PART")) {
        const long long v = std::atoll(e);
        if (v > 0 && v < (1ll << 31)) return (uint32_t)v;
    }
    return (uint32_t)kPartDefault;
}

// The step on `st` (w->mu held).  ev (or NULL): four events recorded before the assignment, after
// it, after the sort and after the update.
int step_locked(Workspace* w, const float* x, int64_t n, int d, const float* c, int k, int flags,
                int32_t* assign, float* dist, float* newc, int64_t* counts, double* obj, hipStream_t st,
                hipEvent_t* ev) {
    const uint32_t P = part_size();
    const int64_t nblk = (n + kBM - 1) / kBM;
    const int64_t maxparts = (n + P - 1) / P + k;
    if (maxparts >= (int64_t(1) << 31)) KNN_FAIL(KNN_EINVAL, "kmeans_step_device: too many parts (%lld)", (long long)maxparts);
    int rc;
    if ((rc = w->cnorm.reserve((size_t)k)) != KNN_OK) return rc;
    if ((rc = w->partial.reserve((size_t)nblk)) != KNN_OK) return rc;
    if ((rc = w->skey.reserve((size_t)n)) != KNN_OK) return rc;
    if ((rc = w->sidx.reserve((size_t)n)) != KNN_OK) return rc;
    if ((rc = w->off.reserve((size_t)k + 1)) != KNN_OK) return rc;
    if ((rc = w->pstart.reserve((size_t)k + 1)) != KNN_OK) return rc;
    if ((rc = w->psum.reserve((size_t)maxparts * d)) != KNN_OK) return rc;
    unsigned end_bit = 1;
    while (end_bit < 31 && (1u << end_bit) < (unsigned)k) ++end_bit;
    const uint32_t* keys_in = reinterpret_cast<const uint32_t*>(assign);
    rocprim::counting_iterator<uint32_t> iota(0u);
    size_t need = 0;
    KNN_HIP(rocprim::radix_sort_pairs(nullptr, need, keys_in, w->skey.get(), iota, w->sidx.get(),
                                      (unsigned)n, 0u, end_bit, st));
    if ((rc = w->tmp.reserve(std::max(need, size_t(16)))) != KNN_OK) return rc;

    if (ev) KNN_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, c, k, d, w->cnorm);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)nblk), dim3(kNT), 0, st, x, n, d, c, w->cnorm, k,
                       (flags & KMEANS_SPHERICAL) ? 1 : 0, row4_vec(x, d), row4_vec(c, d), assign, dist, w->partial);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(kmeans_obj_kernel, dim3(1), dim3(256), 0, st, w->partial, nblk, obj);
    KNN_HIP(hipGetLastError());
    if (ev) KNN_HIP(hipEventRecord(ev[1], st));

    size_t have = w->tmp.cap();
    KNN_HIP(rocprim::radix_sort_pairs(w->tmp.get(), have, keys_in, w->skey.get(), iota, w->sidx.get(),
                                      (unsigned)n, 0u, end_bit, st));
    hipLaunchKernelGGL(kmeans_offsets_kernel, dim3((unsigned)((k + 1 + 255) / 256)), dim3(256), 0, st,
                       w->skey, (uint32_t)n, k, w->off, counts);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(kmeans_parts_kernel, dim3(1), dim3(256), 0, st, w->off, k, P, w->pstart);
    KNN_HIP(hipGetLastError());
    if (ev) KNN_HIP(hipEventRecord(ev[2], st));

    const int dcols = std::min(d, 256), ppb = 256 / dcols;
    hipLaunchKernelGGL(kmeans_partsum_kernel, dim3((unsigned)((maxparts + ppb - 1) / ppb)), dim3(256), 0, st, x,
                       d, w->sidx, w->off, w->pstart, k, P, dcols, ppb, w->psum);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(kmeans_combine_kernel, dim3((unsigned)k), dim3(256), 0, st, w->psum, w->off, w->pstart,
                       d, c, newc);
    KNN_HIP(hipGetLastError());
    if (ev) KNN_HIP(hipEventRecord(ev[3], st));
    return KNN_OK;
}

// faiss split_clusters' donor draw on the host counts; pairs = (ci, cj) in order
int draw_splits(int64_t* cnt, int k, std::vector<int>* pairs) {
    pairs->clear();
    int64_t n = 0;
    bool donor = false, empty = false;
    for (int c = 0; c < k; ++c) {
        if (cnt[c] < 0) KNN_FAIL(KNN_EINVAL, "kmeans_split_device: negative count of cluster %d", c);
        n += cnt[c];
        donor = donor || cnt[c] > 1;
        empty = empty || cnt[c] == 0;
    }
    if (!empty) return KNN_OK;
    if (!donor || n <= k)
        KNN_FAIL(KNN_EINVAL, "kmeans_split_device: an empty cluster and no cluster with more than one member");
    std::mt19937 mt(1234);
    for (int ci = 0; ci < k; ++ci) {
        if (cnt[ci] != 0) continue;
        int cj = 0;
        for (;; cj = (cj + 1) % k) {
            const float p = (float)(((double)cnt[cj] - 1.0) / (double)(n - k));
            const float r = mt() / float(mt.max());
            if (r < p) break;
        }
        pairs->push_back(ci);
        pairs->push_back(cj);
        cnt[ci] = cnt[cj] / 2;
        cnt[cj] -= cnt[ci];
    }
    return KNN_OK;
}

int split_locked(Workspace* w, float* c, int k, int d, int64_t* cnt, int* nsplit, hipStream_t st) {
    std::vector<int> pairs;
    int rc = draw_splits(cnt, k, &pairs);
    if (rc != KNN_OK) return rc;
    const int np = (int)(pairs.size() / 2);
    if (nsplit) *nsplit = np;
    if (np == 0) return KNN_OK;
    if ((rc = w->pairs.reserve(pairs.size())) != KNN_OK) return rc;
    // the list must have left `pairs` before it goes out of scope: the one wait of a repair
    KNN_HIP(hipMemcpyAsync(w->pairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, st));
    KNN_HIP(hipStreamSynchronize(st));
    hipLaunchKernelGGL(kmeans_split_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, c, d, w->pairs, np);
    KNN_HIP(hipGetLastError());
    return KNN_OK;
}

int check_train_args(const void* x, int64_t n, int d, int k, const kmeans_params_t* p, const void* out,
                     const void* obj, const char* who) {
    int rc = check_step_args(x, n, d, x, k, who);
    if (rc != KNN_OK) return rc;
    if (!p || !out || !obj) KNN_FAIL(KNN_EINVAL, "%s: NULL params, centroids_out or obj_out", who);
    if (p->niter <= 0 || p->nredo <= 0)
        KNN_FAIL(KNN_EINVAL, "%s: niter and nredo must be positive (got %d, %d)", who, p->niter, p->nredo);
    return KNN_OK;
}

struct Events {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
};

int train_device_impl(const float* x, int64_t n, int d, int k, const kmeans_params_t* prm, const float* init,
                      float* cout_, double* obj_out, double* stats_out, hipStream_t st) {
    using clk = std::chrono::steady_clock;
    const size_t kd = (size_t)k * d;
    DevBuf<float> ca, cb, di;
    DevBuf<int32_t> as;
    DevBuf<int64_t> cn, rows;
    int rc;
    if ((rc = ca.reserve(kd)) != KNN_OK) return rc;
    if ((rc = cb.reserve(kd)) != KNN_OK) return rc;
    if ((rc = as.reserve((size_t)n)) != KNN_OK) return rc;
    if ((rc = di.reserve((size_t)n)) != KNN_OK) return rc;
    if ((rc = cn.reserve((size_t)k + 1)) != KNN_OK) return rc;      // counts, then the objective
    if (!init && (rc = rows.reserve((size_t)k)) != KNN_OK) return rc;
    Events evs;
    for (hipEvent_t& e : evs.e) KNN_HIP(hipEventCreate(&e));
    int64_t* cnt_d = cn;
    double* obj_d = (double*)(cnt_d + k);
    std::vector<int64_t> host((size_t)k + 1);
    std::vector<double> stats((size_t)prm->niter * KMEANS_STATS_PER_ITER), best_stats;
    std::vector<float> best_c;
    double best_obj = 0.0;
    const int flags = prm->spherical ? KMEANS_SPHERICAL : 0;

    for (int redo = 0; redo < prm->nredo; ++redo) {
        float* cur = ca;
        float* nxt = cb;
        rc = on_workspace<Workspace>(st, [&](Workspace*) -> int {
            if (init) {
                KNN_HIP(hipMemcpyAsync(cur, init, kd * sizeof(float), hipMemcpyHostToDevice, st));
            } else {
                // k distinct rows, Floyd's sampling, in draw order
                std::mt19937_64 rng((uint64_t)prm->seed + (uint64_t)redo);
                std::unordered_set<int64_t> seen;
                std::vector<int64_t> pick;
                for (int64_t j = n - k; j < n; ++j) {
                    const int64_t t = (int64_t)(rng() % (uint64_t)(j + 1));
                    const int64_t v = seen.insert(t).second ? t : j;
                    if (v == j) seen.insert(j);
                    pick.push_back(v);
                }
                KNN_HIP(hipMemcpyAsync(rows, pick.data(), (size_t)k * sizeof(int64_t), hipMemcpyHostToDevice, st));
                KNN_HIP(hipStreamSynchronize(st));
                hipLaunchKernelGGL(kmeans_gather_kernel, dim3((unsigned)k), dim3(256), 0, st, x, d,
                                   rows, cur);
                KNN_HIP(hipGetLastError());
            }
            if (prm->spherical) {
                hipLaunchKernelGGL(kmeans_normalize_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, cur, k, d);
                KNN_HIP(hipGetLastError());
            }
            return KNN_OK;
        });
        if (rc != KNN_OK) return rc;
        const clk::time_point t0 = clk::now();
        double t_search = 0.0, obj = 0.0;
        for (int it = 0; it < prm->niter; ++it) {
            const clk::time_point ts = clk::now();
            int nsplit = 0;
            double s1 = 0.0, s2 = 0.0;
            rc = on_workspace<Workspace>(st, [&](Workspace* w) -> int {
                int rc = step_locked(w, x, n, d, cur, k, flags, as, di, nxt, cnt_d, obj_d, st, evs.e);
                if (rc != KNN_OK) return rc;
                KNN_HIP(hipMemcpyAsync(host.data(), cnt_d, ((size_t)k + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
                KNN_HIP(hipStreamSynchronize(st));
                t_search += std::chrono::duration<double>(clk::now() - ts).count();
                std::memcpy(&obj, &host[k], sizeof(double));
                for (int c = 0; c < k; ++c) {
                    s1 += (double)host[c];
                    s2 += (double)host[c] * (double)host[c];
                }
                if ((rc = split_locked(w, nxt, k, d, host.data(), &nsplit, st)) != KNN_OK) return rc;
                if (prm->spherical) {
                    hipLaunchKernelGGL(kmeans_normalize_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, nxt, k, d);
                    KNN_HIP(hipGetLastError());
                }
                return KNN_OK;
            });
            if (rc != KNN_OK) return rc;
            float ms[3] = {0.f, 0.f, 0.f};
            for (int e = 0; e < 3; ++e) KNN_HIP(hipEventElapsedTime(&ms[e], evs.e[e], evs.e[e + 1]));
            double* s = &stats[(size_t)it * KMEANS_STATS_PER_ITER];
            s[0] = obj;
            s[1] = std::chrono::duration<double>(clk::now() - t0).count();
            s[2] = t_search;
            s[3] = s1 > 0.0 ? (double)k * s2 / (s1 * s1) : 0.0;
            s[4] = (double)nsplit;
            s[5] = ms[0]; s[6] = ms[1]; s[7] = ms[2];
            if (prm->verbose)
                std::fprintf(stderr, "  Iteration %d (%.2f s, search %.2f s): objective=%g imbalance=%.3f nsplit=%d\n",
                             it, stats[(size_t)it * KMEANS_STATS_PER_ITER + 1], t_search, obj,
                             stats[(size_t)it * KMEANS_STATS_PER_ITER + 3], nsplit);
            std::swap(cur, nxt);
        }
        const bool better = redo == 0 || (prm->spherical ? obj > best_obj : obj < best_obj);
        if (better) {
            best_obj = obj;
            best_stats = stats;
            best_c.resize(kd);
            KNN_HIP(hipMemcpyAsync(best_c.data(), cur, kd * sizeof(float), hipMemcpyDeviceToHost, st));
            KNN_HIP(hipStreamSynchronize(st));
        }
        if (prm->verbose && prm->nredo > 1)
            std::fprintf(stderr, "Outer iteration %d / %d: objective %g%s\n", redo, prm->nredo, obj,
                         better ? " (kept)" : "");
    }
    KNN_HIP(hipStreamSynchronize(st));
    std::memcpy(cout_, best_c.data(), kd * sizeof(float));
    *obj_out = best_obj;
    if (stats_out) std::memcpy(stats_out, best_stats.data(), best_stats.size() * sizeof(double));
    return KNN_OK;
}

}  // namespace
}  // namespace imgrec

using namespace imgrec;

extern "C" {

int kmeans_step_device(const float* x, int64_t n, int d, const float* centroids, int k, int flags,
                       int32_t* assign, float* dist, float* new_centroids, int64_t* counts,
                       double* obj, void* stream) {
    int rc = check_step_args(x, n, d, centroids, k, "kmeans_step_device");
    if (rc != KNN_OK) return rc;
    if (!assign || !dist || !new_centroids || !counts || !obj)
        KNN_FAIL(KNN_EINVAL, "kmeans_step_device: NULL output");
    if (new_centroids == centroids) KNN_FAIL(KNN_EINVAL, "kmeans_step_device: new_centroids aliases centroids");
    if (flags & ~KMEANS_SPHERICAL) KNN_FAIL(KNN_EINVAL, "kmeans_step_device: unknown flags 0x%x", flags);
    if ((rc = have_device()) != KNN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return on_workspace<Workspace>(st, [&](Workspace* w) {
        return step_locked(w, x, n, d, centroids, k, flags, assign, dist, new_centroids, counts, obj, st, nullptr);
    });
}

int kmeans_split_device(float* centroids, int k, int d, int64_t* counts_host, int* nsplit, void* stream) {
    if (nsplit) *nsplit = 0;
    if (d <= 0) KNN_FAIL(KNN_EINVAL, "kmeans_split_device: d must be positive (got %d)", d);
    if (k <= 0) KNN_FAIL(KNN_EINVAL, "kmeans_split_device: k must be positive (got %d)", k);
    if (!centroids || !counts_host) KNN_FAIL(KNN_EINVAL, "kmeans_split_device: NULL centroids or counts");
    int rc;
    {
        // a dry run of the draw on a copy: bad counts are reported before any GPU call
        std::vector<int64_t> tmp(counts_host, counts_host + k);
        std::vector<int> pairs;
        if ((rc = draw_splits(tmp.data(), k, &pairs)) != KNN_OK) return rc;
        if (pairs.empty()) return KNN_OK;
    }
    if ((rc = have_device()) != KNN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return on_workspace<Workspace>(
        st, [&](Workspace* w) { return split_locked(w, centroids, k, d, counts_host, nsplit, st); });
}

int kmeans_train_device(const float* x_dev, int64_t n, int d, int k, const kmeans_params_t* params,
                        const float* init_centroids, float* centroids_out, double* obj_out,
                        double* stats_out, void* stream) {
    int rc = check_train_args(x_dev, n, d, k, params, centroids_out, obj_out, "kmeans_train_device");
    if (rc != KNN_OK) return rc;
    if ((rc = have_device()) != KNN_OK) return rc;
    return train_device_impl(x_dev, n, d, k, params, init_centroids, centroids_out, obj_out, stats_out,
                             (hipStream_t)stream);
}

int kmeans_train(const float* x_host, int64_t n, int d, int k, const kmeans_params_t* params,
                 const float* init_centroids, float* centroids_out, double* obj_out, double* stats_out) {
    int rc = check_train_args(x_host, n, d, k, params, centroids_out, obj_out, "kmeans_train");
    if (rc != KNN_OK) return rc;
    if ((rc = have_device()) != KNN_OK) return rc;
    int ndev = 0;
    KNN_HIP(hipGetDeviceCount(&ndev));
    if (params->device >= ndev) KNN_FAIL(KNN_EINVAL, "kmeans_train: device %d out of range (%d visible)", params->device, ndev);
    DeviceGuard g(params->device);
    DevBuf<float> xd;
    if ((rc = xd.reserve((size_t)n * d)) != KNN_OK) return rc;
    StreamGuard sg;       // declared after xd: the stream is drained before the rows are freed
    KNN_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    KNN_HIP(hipMemcpyAsync(xd, x_host, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, sg.s));
    return train_device_impl(xd, n, d, k, params, init_centroids, centroids_out, obj_out,
                             stats_out, sg.s);
}

}  // extern "C"
