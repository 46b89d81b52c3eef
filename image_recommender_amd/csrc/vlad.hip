// vlad.hip — soft-assignment VLAD of local descriptors (include/imgrec_vlad.h; the reference's
// _compute_sift_vlad_worker, vector_scripts/create_sift_vector.py:448-475).
//
// One call (vlad_encode_device) is four launches on the caller's stream, none of which waits:
//   1. vlad_norms_kernel      |c|^2 of the k codebook rows (rows_tile.h row_norms).
//   2. vlad_nn_kernel<L>      the nn nearest rows of every descriptor, over the concatenated
//                             descriptors (images play no part here): the row tile of rows_tile.h
//                             with the codebook as the rows and kmeans_assign_kernel's key,
//                             fmaf(-2, x.c, |c|^2).  Where that kernel keeps one running (key, id)
//                             minimum, a lane here keeps a sorted list of L = 1, 2, 4 or 8 >= nn
//                             entries per descriptor in registers (a compare against the list's
//                             tail, then an unrolled bubble towards the head).  The two half waves'
//                             lists meet by a cross-lane exchange, the four codebook waves' lists in
//                             LDS; one thread per descriptor merges them.  Then |x - c|^2 of the nn
//                             listed rows is summed directly, 16 (descriptor, row) pairs at a time
//                             per wave.
//   3. vlad_aggregate_kernel  a workgroup per (image, tile of ct codebook rows); the accumulator,
//                             ct x d sums, lives in LDS (ct = k = 256 at d = 128: 128 KiB of the
//                             CU's 160).  A wave owns the rows with
//                             (row - tile start) mod 8 == its number and a lane the columns lane,
//                             lane + 64, ...: every accumulator element has one owner, so the kernel
//                             needs no atomics, and no barrier between its zeroing and its sums.
//                             Every wave scans the image's N_i x nn list entries 64 at a time (a lane
//                             per entry), keeps its own by ballot, and serves them in ascending
//                             entry order, eight at a time: the loads of the eight descriptor rows
//                             and of their codebook rows (from L2) are issued together, the eight
//                             fmaf(w, x - C, acc) into LDS follow in order.
//   4. vlad_epilogue_kernel   (not with VLAD_RAW) a workgroup per image: the row norms and the
//                             global norm in float64 in the fixed order the header documents, then
//                             sign(v) sqrt(|v| / r) / g in float64, rounded once.  The global norm
//                             needs no pass of its own: |sign(v) sqrt(|v| / r)|^2 = |v| / r, so
//                             g^2 = sum_rows (sum |v|) / r comes out of the pass that finds r.
//                             It is a launch of its own because the norm spans the cluster tiles.
//
// Determinism.  Keys: rows_tile.h's argument; lexicographic (key, id) at every level; ids are
// distinct, so the sorted list is unique whatever the insertion order.  Aggregation: an element's
// members are added by its one owner in ascending descriptor order, whatever ct, the grid or the
// image's place in the batch.
//
// Registers and LDS.  vlad_nn_kernel: the tile's 55 KB; after the stream the stage buffer holds the
// waves' lists (4 x 128 x L keys and ids) and the merged ids (128 x L): 36 KB at L = 8.  204 VGPRs
// (232 at L = 8) against kmeans_assign_kernel's 184: the lists, and 16 distance pairs in flight;
// two waves per SIMD either way.  The
// aggregation takes 51 VGPRs and ct x d floats of dynamic LDS.  Figures per kernel: profiles/vlad/.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../include/imgrec_vlad.h"
#include "dev_workspace.h"
#include "rows_tile.h"
#include "vlad_args.h"

namespace imgrec {
namespace {

constexpr int kDP = 16;                 // (descriptor, row) pairs whose direct distances a wave sums at a time
constexpr int kAG = 8;                  // list entries whose descriptor loads an aggregation wave issues together
constexpr int kAggNT = 512;             // aggregation: 8 waves, a wave per residue of the row mod 8
constexpr int kAggWaves = kAggNT / 64;
static_assert(9 * kBM * VLAD_MAX_NN <= kRows * kLDK, "the lists fit the stage buffer");
static_assert((kAggWaves & (kAggWaves - 1)) == 0, "row ownership is a mask");

// (key, id) into a list sorted ascending: dropped unless it beats the tail
template <int L>
__device__ __forceinline__ void list_insert(float (&lk)[L], int (&li)[L], float key, int id) {
    if (key_less(key, id, lk[L - 1], li[L - 1])) {
        lk[L - 1] = key;
        li[L - 1] = id;
#pragma unroll
        for (int s = L - 1; s > 0; --s) {
            const float ak = lk[s - 1], bk = lk[s];
            const int ai = li[s - 1], bi = li[s];
            const bool sw = key_less(bk, bi, ak, ai);
            lk[s - 1] = sw ? bk : ak;
            li[s - 1] = sw ? bi : ai;
            lk[s] = sw ? ak : bk;
            li[s] = sw ? ai : bi;
        }
    }
}

__global__ void __launch_bounds__(256)
vlad_norms_kernel(const float* __restrict__ c, int k, int d, float* __restrict__ out) {
    row_norms(c, k, d, out);
}

template <int L>
__global__ void __launch_bounds__(kNT)
vlad_nn_kernel(const float* __restrict__ x, int64_t n, int d, const float* __restrict__ c,
               const float* __restrict__ cn, int k, int nn, int vec_x, int vec_c,
               int* __restrict__ nn_idx, float* __restrict__ nn_dist) {
    __shared__ __attribute__((aligned(16))) float stage[kRows * kLDK];
    __shared__ float cns[kBN];
    // after the last stage the buffer holds the waves' lists and the merged ids
    float* const redk = stage;                                             // [4][kBM][L]
    int* const redi = reinterpret_cast<int*>(stage + 4 * kBM * L);          // [4][kBM][L]
    int* const s_id = reinterpret_cast<int*>(stage + 8 * kBM * L);          // [kBM][L]

    const RowLanes t;
    const int tid = t.tid, lane = t.lane, wave = t.wave, lr = t.lr, lh = t.lh, wc = t.wc, wp = t.wp;
    const int64_t p0 = (int64_t)blockIdx.x * kBM;
    float lk[2][L];
    int li[2][L];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int s = 0; s < L; ++s) {
            lk[b][s] = INFINITY;
            li[b][s] = INT32_MAX;
        }
    rows_stream(t, stage, cns, x, n, d, c, cn, k, vec_x, vec_c,
                [&](int b, float dot, float cnv, int cid) __attribute__((always_inline)) {
                    list_insert<L>(lk[b], li[b], fmaf(-2.f, dot, cnv), cid);
                });

    // the two halves of a wave (each takes the other's list), then the four waves that share the
    // descriptors
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        float ok[L];
        int oi[L];
#pragma unroll
        for (int s = 0; s < L; ++s) {
            ok[s] = __shfl_xor(lk[b][s], 32);
            oi[s] = __shfl_xor(li[b][s], 32);
        }
#pragma unroll
        for (int s = 0; s < L; ++s) list_insert<L>(lk[b], li[b], ok[s], oi[s]);
        if (lh == 0) {
            const int o = (wc * kBM + wp * 64 + b * 32 + lr) * L;
#pragma unroll
            for (int s = 0; s < L; ++s) {
                redk[o + s] = lk[b][s];
                redi[o + s] = li[b][s];
            }
        }
    }
    __syncthreads();
    if (tid < kBM) {
        float fk[L];
        int fi[L];
#pragma unroll
        for (int s = 0; s < L; ++s) {
            fk[s] = redk[tid * L + s];
            fi[s] = redi[tid * L + s];
        }
#pragma unroll
        for (int w = 1; w < 4; ++w)
#pragma unroll
            for (int s = 0; s < L; ++s)
                list_insert<L>(fk, fi, redk[(w * kBM + tid) * L + s], redi[(w * kBM + tid) * L + s]);
#pragma unroll
        for (int s = 0; s < L; ++s)          // NaN keys leave a slot unfilled: row 0, never out of range
            s_id[tid * L + s] = (fi[s] < 0 || fi[s] >= k) ? 0 : fi[s];
    }
    __syncthreads();
    // the distances to the listed rows, summed directly: kBM / 8 descriptors x nn pairs per wave,
    // kDP at a time (their loads are independent), lanes over columns, a fixed butterfly
    constexpr int PW = kBM / (kNT / 64);
    static_assert(PW % kDP == 0, "a wave's pairs divide evenly for every nn");
    const int npair = PW * nn;               // a multiple of kDP
#pragma unroll 1
    for (int pp = 0; pp < npair; pp += kDP) {
        const float* xr[kDP];
        const float* cr[kDP];
        float sum[kDP];
        int pl[kDP], sl[kDP], id[kDP];
#pragma unroll
        for (int q = 0; q < kDP; ++q) {
            pl[q] = wave * PW + (pp + q) / nn;
            sl[q] = (pp + q) % nn;
            id[q] = s_id[pl[q] * L + sl[q]];
            const int64_t p = min(p0 + pl[q], n - 1);            // a clamped row is computed, not written
            xr[q] = x + p * (int64_t)d;
            cr[q] = c + (int64_t)id[q] * d;
            sum[q] = 0.f;
        }
        for (int j = lane; j < d; j += 64) {
#pragma unroll
            for (int q = 0; q < kDP; ++q) {
                const float t = xr[q][j] - cr[q][j];
                sum[q] = fmaf(t, t, sum[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < kDP; ++q) {
            sum[q] = wave_sum(sum[q]);
            if (lane == 0 && p0 + pl[q] < n) {
                const int64_t o = (p0 + pl[q]) * nn + sl[q];
                nn_idx[o] = id[q];
                nn_dist[o] = sum[q];
            }
        }
    }
}

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__global__ void __launch_bounds__(kAggNT)
vlad_aggregate_kernel(const float* __restrict__ x, int64_t n, int d, const int64_t* __restrict__ offsets,
                      const float* __restrict__ c, int k, int nn, float two_s2,
                      const int* __restrict__ nn_idx, const float* __restrict__ nn_dist, int ct, int ntiles,
                      float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const acc = lds;                          // [ct][d]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t img = blockIdx.x / (unsigned)ntiles;
    const int c0 = (int)(blockIdx.x % (unsigned)ntiles) * ct, cn = min(ct, k - c0);
    const int64_t o0 = min(max(offsets[img], (int64_t)0), n), o1 = min(max(offsets[img + 1], o0), n);
    float* const dst = out + (img * k + c0) * (int64_t)d;
    const int total = cn * d;                        // <= the accumulator's floats
    if (o0 == o1) {                                  // no descriptors: the zero vector
        for (int e = tid; e < total; e += kAggNT) dst[e] = 0.f;
        return;
    }
    // a wave zeroes what it owns and is the only one to touch it until the final barrier
    for (int li = wave; li < cn; li += kAggWaves)
        for (int col = lane; col < d; col += 64) acc[li * d + col] = 0.f;
    const int64_t e0 = o0 * nn, e1 = o1 * nn;
    for (int64_t base = e0; base < e1; base += 64) {
        const int64_t e = base + lane;
        bool mine = false;
        int li = 0, row = 0;
        float w = 0.f;
        if (e < e1) {
            li = nn_idx[e] - c0;
            mine = li >= 0 && li < cn && (li & (kAggWaves - 1)) == wave;
            if (mine) {
                w = expf(-nn_dist[e] / two_s2);
                row = (int)((uint64_t)e / (unsigned)nn);
            }
        }
        uint64_t mask = __ballot(mine);
        while (mask) {                               // wave-uniform: ascending entries, kAG at a time
            int lq[kAG], rq[kAG];
            float wq[kAG];
            bool on[kAG];
#pragma unroll
            for (int q = 0; q < kAG; ++q) {
                on[q] = mask != 0;
                const int b = on[q] ? __builtin_ctzll(mask) : 0;
                mask &= mask - 1;                    // (0 stays 0)
                lq[q] = lane_i(li, b);
                rq[q] = lane_i(row, b);
                wq[q] = lane_f(w, b);
            }
            for (int col = lane; col < d; col += 64) {
                float v[kAG], cv[kAG];
#pragma unroll
                for (int q = 0; q < kAG; ++q) {
                    v[q] = on[q] ? x[(int64_t)rq[q] * d + col] : 0.f;
                    cv[q] = on[q] ? c[(int64_t)(c0 + lq[q]) * d + col] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < kAG; ++q)
                    if (on[q]) {
                        float* a = acc + lq[q] * d + col;
                        *a = fmaf(wq[q], v[q] - cv[q], *a);
                    }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < total; e += kAggNT) dst[e] = acc[e];
}

// In place on an image's k x d raw rows; rn, ga: k doubles each per image (workspace).
__global__ void __launch_bounds__(256)
vlad_epilogue_kernel(float* __restrict__ out, int k, int d, double* __restrict__ rnorm, double* __restrict__ gpart) {
    __shared__ double sh[256];
    __shared__ double s_g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const v = out + (int64_t)blockIdx.x * k * d;
    double* const rn = rnorm + (int64_t)blockIdx.x * k;
    double* const ga = gpart + (int64_t)blockIdx.x * k;
    for (int row = wave; row < k; row += 4) {
        const float* p = v + (int64_t)row * d;
        double s = 0.0, a = 0.0;
        for (int col = lane; col < d; col += 64) {
            const double t = (double)p[col];
            s = fma(t, t, s);
            a += fabs(t);
        }
        s = wave_sum(s);
        a = wave_sum(a);
        if (lane == 0) {
            const double r = sqrt(s);
            rn[row] = r;
            ga[row] = r > 0.0 ? a / r : 0.0;
        }
    }
    __syncthreads();
    double t = 0.0;
    for (int row = tid; row < k; row += 256) t += ga[row];
    sh[tid] = t;
    __syncthreads();
    if (tid == 0) {
        double g2 = 0.0;
        for (int i = 0; i < 256; ++i) g2 += sh[i];
        s_g = sqrt(g2);
    }
    __syncthreads();
    const double g = s_g;
    for (int row = wave; row < k; row += 4) {
        float* p = v + (int64_t)row * d;
        const double r = rn[row];
        for (int col = lane; col < d; col += 64) {
            const double t = (double)p[col];
            double o = 0.0;
            if (r > 0.0 && g > 0.0) o = copysign(sqrt(fabs(t) / r) / g, t);
            p[col] = (float)o;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------

// what a call's launches share (dev_workspace.h: one per device)
struct Workspace : StreamHandoff {
    DevBuf<float> cnorm;
    DevBuf<int32_t> idx;
    DevBuf<float> dist;
    DevBuf<double> rnorm;
    DevBuf<double> gpart;
};

int check_args(const VladArgs& a, const char* who) {
    char msg[256];
    if (vlad_check_args(a, who, msg, sizeof msg) != 0) KNN_FAIL(KNN_EINVAL, "%s", msg);
    return KNN_OK;
}

int64_t acc_floats() {
    if (const char* e = test_knob("IMGREC_VLAD_LDS_FLOATS")) {
        const long long v = std::atoll(e);
        if (v > 0 && v <= kVladAccFloats) return v;
    }
    return kVladAccFloats;
}

template <int L>
int launch_nn(const float* x, int64_t n, int d, const float* c, const float* cn, int k, int nn, int32_t* idx,
              float* dist, hipStream_t st) {
    hipLaunchKernelGGL(vlad_nn_kernel<L>, dim3((unsigned)((n + kBM - 1) / kBM)), dim3(kNT), 0, st, x, n, d, c, cn,
                       k, nn, row4_vec(x, d), row4_vec(c, d), idx, dist);
    KNN_HIP(hipGetLastError());
    return KNN_OK;
}

// the launches on `st` (w->mu held); `ct`, `ntiles` from vlad_cluster_tile
int encode_locked(Workspace* w, const VladArgs& a, int ct, int64_t ntiles, int32_t* nn_idx, float* nn_dist,
                  hipStream_t st) {
    const float* x = (const float*)a.x;
    const float* c = (const float*)a.codebook;
    float* out = (float*)a.vlad;
    const size_t lists = (size_t)a.N * a.nn;
    int rc;
    if ((rc = w->cnorm.reserve((size_t)a.k)) != KNN_OK) return rc;
    if (!nn_idx && (rc = w->idx.reserve(std::max(lists, size_t(1)))) != KNN_OK) return rc;
    if (!nn_dist && (rc = w->dist.reserve(std::max(lists, size_t(1)))) != KNN_OK) return rc;
    const bool raw = (a.flags & VLAD_RAW) != 0;
    if (!raw) {
        if ((rc = w->rnorm.reserve((size_t)a.nimg * a.k)) != KNN_OK) return rc;
        if ((rc = w->gpart.reserve((size_t)a.nimg * a.k)) != KNN_OK) return rc;
    }
    int32_t* idx = nn_idx ? nn_idx : w->idx.get();
    float* dist = nn_dist ? nn_dist : w->dist.get();
    if (a.N > 0) {
        hipLaunchKernelGGL(vlad_norms_kernel, dim3((unsigned)((a.k + 3) / 4)), dim3(256), 0, st, c, a.k, a.d,
                           w->cnorm.get());
        KNN_HIP(hipGetLastError());
        if (a.nn == 1) rc = launch_nn<1>(x, a.N, a.d, c, w->cnorm, a.k, a.nn, idx, dist, st);
        else if (a.nn == 2) rc = launch_nn<2>(x, a.N, a.d, c, w->cnorm, a.k, a.nn, idx, dist, st);
        else if (a.nn <= 4) rc = launch_nn<4>(x, a.N, a.d, c, w->cnorm, a.k, a.nn, idx, dist, st);
        else rc = launch_nn<8>(x, a.N, a.d, c, w->cnorm, a.k, a.nn, idx, dist, st);
        if (rc != KNN_OK) return rc;
    }
    const size_t lds = (size_t)ct * a.d * sizeof(float);
    KNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(vlad_aggregate_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const float two_s2 = (float)(2.0 * (double)a.sigma * (double)a.sigma);
    hipLaunchKernelGGL(vlad_aggregate_kernel, dim3((unsigned)(a.nimg * ntiles)), dim3(kAggNT), lds, st, x, a.N,
                       a.d, (const int64_t*)a.offsets, c, a.k, a.nn, two_s2, idx, dist, ct, (int)ntiles, out);
    KNN_HIP(hipGetLastError());
    if (!raw) {
        hipLaunchKernelGGL(vlad_epilogue_kernel, dim3((unsigned)a.nimg), dim3(256), 0, st, out, a.k, a.d,
                           w->rnorm.get(), w->gpart.get());
        KNN_HIP(hipGetLastError());
    }
    return KNN_OK;
}

int encode_device_impl(const VladArgs& a, int32_t* nn_idx, float* nn_dist, hipStream_t st) {
    if (a.nimg == 0) return KNN_OK;
    int ct = 0;
    int64_t ntiles = 0;
    char msg[256];
    if (vlad_cluster_tile(a.k, a.d, acc_floats(), a.nimg, &ct, &ntiles, "vlad_encode_device", msg, sizeof msg) != 0)
        KNN_FAIL(KNN_EINVAL, "%s", msg);
    int rc = have_device();
    if (rc != KNN_OK) return rc;
    return on_workspace<Workspace>(
        st, [&](Workspace* w) { return encode_locked(w, a, ct, ntiles, nn_idx, nn_dist, st); });
}

}  // namespace
}  // namespace imgrec

using namespace imgrec;

extern "C" {

int vlad_encode_device(const float* x, int64_t N, const int64_t* offsets, int64_t nimg, int d,
                       const float* codebook, int k, int nn, float sigma, int flags, float* vlad,
                       int32_t* nn_idx, float* nn_dist, void* stream) {
    const VladArgs a{x, N, offsets, nimg, d, codebook, k, nn, sigma, flags, vlad};
    const int rc = check_args(a, "vlad_encode_device");
    if (rc != KNN_OK) return rc;
    return encode_device_impl(a, nn_idx, nn_dist, (hipStream_t)stream);
}

int vlad_encode(const float* x, int64_t N, const int64_t* offsets, int64_t nimg, int d,
                const float* codebook, int k, int nn, float sigma, int flags, float* vlad,
                int32_t* nn_idx, float* nn_dist, int device) {
    const VladArgs a{x, N, offsets, nimg, d, codebook, k, nn, sigma, flags, vlad};
    int rc = check_args(a, "vlad_encode");
    if (rc != KNN_OK) return rc;
    char msg[256];
    if (vlad_check_offsets(offsets, nimg, N, "vlad_encode", msg, sizeof msg) != 0) KNN_FAIL(KNN_EINVAL, "%s", msg);
    if (nimg == 0) return KNN_OK;
    if ((rc = have_device()) != KNN_OK) return rc;
    int ndev = 0;
    KNN_HIP(hipGetDeviceCount(&ndev));
    if (device >= ndev) KNN_FAIL(KNN_EINVAL, "vlad_encode: device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    const size_t nx = (size_t)N * d, nc = (size_t)k * d, no = (size_t)nimg * k * d, nl = (size_t)N * nn;
    DevBuf<float> xd, cd, od, dd;
    DevBuf<int64_t> offd;
    DevBuf<int32_t> idd;
    if ((rc = xd.reserve(std::max(nx, size_t(1)))) != KNN_OK) return rc;
    if ((rc = cd.reserve(nc)) != KNN_OK) return rc;
    if ((rc = od.reserve(no)) != KNN_OK) return rc;
    if ((rc = offd.reserve((size_t)nimg + 1)) != KNN_OK) return rc;
    if (nn_idx && (rc = idd.reserve(std::max(nl, size_t(1)))) != KNN_OK) return rc;
    if (nn_dist && (rc = dd.reserve(std::max(nl, size_t(1)))) != KNN_OK) return rc;
    StreamGuard sg;       // declared after the buffers: the stream is drained before they are freed
    KNN_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    if (nx) KNN_HIP(hipMemcpyAsync(xd, x, nx * sizeof(float), hipMemcpyHostToDevice, sg.s));
    KNN_HIP(hipMemcpyAsync(cd, codebook, nc * sizeof(float), hipMemcpyHostToDevice, sg.s));
    KNN_HIP(hipMemcpyAsync(offd, offsets, ((size_t)nimg + 1) * sizeof(int64_t), hipMemcpyHostToDevice, sg.s));
    const VladArgs da{xd.get(), N, offd.get(), nimg, d, cd.get(), k, nn, sigma, flags, od.get()};
    if ((rc = encode_device_impl(da, nn_idx ? idd.get() : nullptr, nn_dist ? dd.get() : nullptr, sg.s)) != KNN_OK)
        return rc;
    KNN_HIP(hipMemcpyAsync(vlad, od, no * sizeof(float), hipMemcpyDeviceToHost, sg.s));
    if (nn_idx && nl) KNN_HIP(hipMemcpyAsync(nn_idx, idd, nl * sizeof(int32_t), hipMemcpyDeviceToHost, sg.s));
    if (nn_dist && nl) KNN_HIP(hipMemcpyAsync(nn_dist, dd, nl * sizeof(float), hipMemcpyDeviceToHost, sg.s));
    KNN_HIP(hipStreamSynchronize(sg.s));
    return KNN_OK;
}

}  // extern "C"
