// rows_tile.h — the fp32 row tile shared by the kernels that hold a few hundred rows against
// millions: kmeans_assign_kernel (knn_kmeans.hip: centroids against points) and vlad_nn_kernel<L>
// (vlad.hip: codebook rows against descriptors).  One definition of the tile geometry, the guarded
// row load, the stage stream and the row norms, so the depth order and the dot product behind every
// key — what makes the two kernels' results bitwise equal — cannot drift apart.  A sibling of
// knn_tile.h, whose ring is DMA-fed; this one is register-staged.  Included by .hip translation
// units only.
//
// A workgroup of 8 waves owns kBM = 128 points and streams the rows in tiles of kBN = 256 through
// LDS, kBK = 32 columns (one 128-byte line of every row) per stage.  One stage buffer: the next
// stage's global loads are issued before the MFMAs, wait in registers and are stored between two
// barriers.  Four waves split a tile's rows (64 each), two the points (64 each): a wave holds 2 x 2
// accumulators of v_mfma_f32_32x32x2_f32 with the rows as A and the points as B (columns), so a lane
// owns one point per column block and its 16 accumulator registers are 16 rows of that point: what
// a kernel keeps per point (a minimum, a list) needs no cross-lane step until the stream ends.  With
// k <= 256 every point is loaded once; with more tiles the workgroup's 128 points are re-read once
// per tile (from L2).
//
// Determinism.  A dot product is an fmaf chain over the depth in one order for every (row, point)
// pair: which tile, wave, lane or register a row falls in changes nothing, so two bitwise-equal rows
// give a point bitwise-equal dot products.  Zero padding of the depth adds +0 products to every pair
// alike.
//
// LDS: 384 rows x 36 floats (32 + 4 pad: the 16 rows a quarter wave reads as float4 fall in distinct
// banks) = 55,296 B plus 256 norms: 55 KB, declared by the kernel, which reuses the stage buffer
// after the stream.  (A 64-point, 16-column, double-buffered form of the tile ran 49 / 67 TF where
// this one runs 57 / 80 TF at d = 128, k = 256 / d = 768, k = 1024: it fetched half a line per row
// and stage and re-read the rows twice as often; profiles/kmeans/.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace imgrec {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBM = 128;                // points per workgroup
constexpr int kBN = 256;                // rows per tile
constexpr int kBK = 32;                 // depth per stage: a row's 128-byte line
constexpr int kLDK = kBK + 4;           // LDS row stride (floats)
constexpr int kNT = 512;                // threads: 4 waves over the rows x 2 over the points
constexpr int kQ = kBK / 4;             // float4 per row and stage
constexpr int kRows = kBN + kBM;        // rows per stage: the row tile, then the points
constexpr int kLd4 = kRows * kQ / kNT;  // float4 loads per thread and stage
static_assert(kRows * kQ % kNT == 0 && kBM == 2 * 64 && kBN == 4 * 64, "stage loads divide evenly");

// a thread's place: its wave's 64 rows of the tile (wc) and 64 points (wp); its column of the two
// 32-point blocks (lr) and its half wave (lh)
struct RowLanes {
    int tid, lane, wave, lr, lh, wc, wp;
    __device__ __forceinline__ RowLanes()
        : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), lr(lane & 31), lh(lane >> 5), wc(wave & 3),
          wp(wave >> 2) {}
};

// columns [col, col + 4) of row `row` (zeros outside the matrix)
__device__ __forceinline__ float4 load_row4(const float* __restrict__ base, int64_t row, int64_t nrows,
                                            int d, int col, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nrows && col < d) {
        const float* p = base + row * (int64_t)d + col;
        if (vec && col + 4 <= d) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = p[0];
            if (col + 1 < d) v.y = p[1];
            if (col + 2 < d) v.z = p[2];
            if (col + 3 < d) v.w = p[3];
        }
    }
    return v;
}

// (key a, id a) before (key b, id b): the order of every minimum and list over the stream's keys
__device__ __forceinline__ bool key_less(float ka, int ia, float kb, int ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// out[r] = |row r|^2 on 256 threads, one wave per row: lanes stride the columns, then a fixed
// butterfly
__device__ __forceinline__ void row_norms(const float* __restrict__ c, int k, int d, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= k) return;
    const float* p = c + (int64_t)row * d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) s = fmaf(p[j], p[j], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[row] = s;
}

// The stage stream of workgroup blockIdx.x: every row tile against its kBM points.  stage
// (kRows * kLDK floats, 16-byte aligned) and cns (kBN floats) are the kernel's LDS.  From a tile's
// last stage, on_key(b, dot, cnv, cid) is called once per live row cid < k and point block b = 0, 1
// of the lane (point p0 + wp * 64 + b * 32 + lr): dot = x . c and cnv = cn[cid].  A lane sees its
// point's rows in ascending tile order; all threads have passed a barrier when the stream returns.
template <class OnKey>
__device__ __forceinline__ void rows_stream(const RowLanes& t, float* __restrict__ stage, float* __restrict__ cns,
                                            const float* __restrict__ x, int64_t n, int d,
                                            const float* __restrict__ c, const float* __restrict__ cn, int k,
                                            int vec_x, int vec_c, OnKey on_key) {
    const int tid = t.tid, lr = t.lr, lh = t.lh, wc = t.wc, wp = t.wp;
    const int64_t p0 = (int64_t)blockIdx.x * kBM;
    const int nkc = (d + kBK - 1) / kBK, nct = (k + kBN - 1) / kBN;
    const int total = nct * nkc;            // < 2^31: checked on the host

    float4 pre[kLd4];
    auto fetch = [&](int s) __attribute__((always_inline)) {
        const int ct = s / nkc, kc = s - ct * nkc;
#pragma unroll
        for (int it = 0; it < kLd4; ++it) {
            const int idx = tid + it * kNT, row = idx / kQ, col = kc * kBK + 4 * (idx % kQ);
            pre[it] = row < kBN ? load_row4(c, (int64_t)ct * kBN + row, k, d, col, vec_c)
                                : load_row4(x, p0 + (row - kBN), n, d, col, vec_x);
        }
    };
    auto store = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < kLd4; ++it) {
            const int idx = tid + it * kNT;
            *reinterpret_cast<float4*>(stage + (idx / kQ) * kLDK + 4 * (idx % kQ)) = pre[it];
        }
        const int ct = s / nkc;
        if (s - ct * nkc == 0 && tid < kBN) {    // a tile's first stage brings its norms
            const int64_t cid = (int64_t)ct * kBN + tid;
            cns[tid] = cid < k ? cn[cid] : 0.f;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    fetch(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < total; ++s) {
        if (s + 1 < total) fetch(s + 1);     // in flight during the MFMAs
        // a half wave takes columns 8 g + 4 lh .. + 3 of each group g of 8: the depth order is a
        // permutation of the columns, the same for every pair
#pragma unroll
        for (int g = 0; g < kBK / 8; ++g) {
            float av[2][4], bv[2][4];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float4 v = *reinterpret_cast<const float4*>(
                    stage + (wc * 64 + a * 32 + lr) * kLDK + 8 * g + 4 * lh);
                av[a][0] = v.x; av[a][1] = v.y; av[a][2] = v.z; av[a][3] = v.w;
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float4 v = *reinterpret_cast<const float4*>(
                    stage + (kBN + wp * 64 + b * 32 + lr) * kLDK + 8 * g + 4 * lh);
                bv[b][0] = v.x; bv[b][1] = v.y; bv[b][2] = v.z; bv[b][3] = v.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][e], bv[b][e], acc[a][b], 0, 0, 0);
        }
        const int ct = s / nkc;
        if (s - ct * nkc == nkc - 1) {       // the tile's last stage: its dot products leave
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = wc * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const int64_t cid = (int64_t)ct * kBN + i;
                    if (cid < k) {
                        const float cnv = cns[i];
#pragma unroll
                        for (int b = 0; b < 2; ++b) on_key(b, acc[a][b][r], cnv, (int)cid);
                    }
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b][r] = 0.f;
                }
        }
        __syncthreads();                     // every wave has read the stage (and the norms)
        if (s + 1 < total) store(s + 1);
        __syncthreads();
    }
}

}  // namespace imgrec
