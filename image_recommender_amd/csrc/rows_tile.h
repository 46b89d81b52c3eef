// rows_tile.h — the fp32 row tile shared by the kernels that hold a few hundred rows against
// millions: kmeans_assign_kernel (knn_kmeans.hip: centroids against points), vlad_nn_kernel<L>
// (vlad.hip: codebook rows against descriptors) and vladenc_linear_kernel<..> (vladenc.hip: weight
// rows against batch rows, a plain GEMM).  One definition of the tile geometry (its numbers:
// rows_geom.h), the guarded row load, the stage stream, the accumulator map, the row norms and the
// wave sum, so the depth order and the dot product behind every key and every partial sum — what
// makes the kernels' results bitwise reproducible, and the first two kernels' bitwise equal —
// cannot drift apart.  A sibling of knn_tile.h, whose ring is DMA-fed; this one is register-staged.
// Included by .hip translation units only.
//
// stage_stream<G> is the one stage loop: FW x PW waves over the rows and the points, FA x PB
// accumulators of v_mfma_f32_32x32x2_f32 per wave with the rows as A and the points as B (columns),
// kBK = 32 columns (one 128-byte line of every row) per stage through one LDS stage buffer: the next
// stage's global loads are issued before the MFMAs, wait in registers and are stored between two
// barriers.  A lane owns one point per column block and its 16 accumulator registers are 16 rows of
// that point: what a kernel keeps per point (a minimum, a list) needs no cross-lane step until the
// stream ends.  What a stage holds, and what happens when it is stored and when its MFMAs are done,
// is the caller's: rows_stream walks row tiles against a workgroup's points and hands out keys at a
// tile's end; the encoder streams a depth split of one feature tile and keeps the accumulators.
//
// rows_stream.  A workgroup owns kBM = 128 points and streams the rows in tiles of kBN = 256: four
// waves split a tile's rows (64 each), two the points (64 each), 2 x 2 accumulators per wave.  With
// k <= 256 every point is loaded once; with more tiles the workgroup's 128 points are re-read once
// per tile (from L2).
//
// Determinism.  A dot product is an fmaf chain over the depth in one order for every (row, point)
// pair: which tile, wave, lane, register or geometry a row falls in changes nothing, so two
// bitwise-equal rows give a point bitwise-equal dot products.  Zero padding of the depth adds +0
// products to every pair alike.
//
// LDS: 384 rows x 36 floats (32 + 4 pad: the 16 rows a quarter wave reads as float4 fall in distinct
// banks) = 55,296 B plus 256 norms: 55 KB, declared by the kernel, which reuses the stage buffer
// after the stream.  (A 64-point, 16-column, double-buffered form of the tile ran 49 / 67 TF where
// this one runs 57 / 80 TF at d = 128, k = 256 / d = 768, k = 1024: it fetched half a line per row
// and stage and re-read the rows twice as often; profiles/kmeans/.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rows_geom.h"

namespace imgrec {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// FW x PW waves over the rows and the points, FA x PB accumulators of 32 x 32 per wave
template <int FW_, int PW_, int FA_, int PB_>
struct StageGeom {
    static constexpr int FW = FW_, PW = PW_, FA = FA_, PB = PB_;
    static constexpr int BN = FW * FA * 32;               // rows per stage
    static constexpr int BM = PW * PB * 32;               // points per stage
    static constexpr int R = BN + BM;                     // a stage: the rows, then the points
    static constexpr int LD4 = (R * kQ + kNT - 1) / kNT;  // float4 loads per thread and stage
    static_assert(FW * PW * 64 == kNT, "eight waves");
};
using RowGeom = StageGeom<4, 2, 2, 2>;
constexpr int kRows = RowGeom::R;
static_assert(RowGeom::BN == kBN && RowGeom::BM == kBM && kRows * kQ % kNT == 0, "stage loads divide evenly");

// a thread's place: its wave's rows (wc) and points (wp); its column of the 32-point blocks (lr)
// and its half wave (lh)
template <class G>
struct StageLanes {
    int tid, lane, wave, lr, lh, wc, wp;
    __device__ __forceinline__ StageLanes()
        : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), lr(lane & 31), lh(lane >> 5), wc(wave % G::FW),
          wp(wave / G::FW) {}
    // the stage row of register r of accumulator [a][.], and the stage's point of accumulator [.][b]
    __device__ __forceinline__ int acc_row(int a, int r) const {
        return (wc * G::FA + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    }
    __device__ __forceinline__ int acc_point(int b) const { return (wp * G::PB + b) * 32 + lr; }
};
using RowLanes = StageLanes<RowGeom>;

// columns [col, col + 4) of row `row` (zeros outside the matrix); vec = row4_vec of the matrix
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
// whether every four columns of a matrix of d columns at p are one aligned float4 (host side)
inline int row4_vec(const float* p, int d) { return d % 4 == 0 && (uintptr_t)p % 16 == 0; }

// (key a, id a) before (key b, id b): the order of every minimum and list over the stream's keys
__device__ __forceinline__ bool key_less(float ka, int ia, float kb, int ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// the sum of v over the wave, in every lane: a fixed butterfly
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// out[r] = |row r|^2 on 256 threads, one wave per row: lanes stride the columns, then the wave sum
__device__ __forceinline__ void row_norms(const float* __restrict__ c, int k, int d, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= k) return;
    const float* p = c + (int64_t)row * d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) s = fmaf(p[j], p[j], s);
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

// Stages s0 .. s1 - 1 (s0 < s1) through `stage` (G::R * kLDK floats of LDS, 16-byte aligned), into
// acc, zeroed first.  load(s, row, c4) is the float4 at column offset c4 of row `row` of stage s;
// stored(s) runs with the store of stage s, done(s) after the MFMAs of stage s and before the
// barrier that ends its reads (it may use and reset acc).  All threads have passed a barrier when
// the stream returns.
template <class G, class Load, class Stored, class Done>
__device__ __forceinline__ void stage_stream(float* __restrict__ stage, int s0, int s1,
                                             f32x16 (&acc)[G::FA][G::PB], Load load, Stored stored, Done done) {
    const StageLanes<G> t;
    const int tid = t.tid, lr = t.lr, lh = t.lh;
    float4 pre[G::LD4];
    auto fetch = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < G::LD4; ++it) {
            const int idx = tid + it * kNT;
            if (G::R * kQ % kNT == 0 || idx < G::R * kQ) pre[it] = load(s, idx / kQ, 4 * (idx % kQ));
        }
    };
    auto store = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < G::LD4; ++it) {
            const int idx = tid + it * kNT;
            if (G::R * kQ % kNT == 0 || idx < G::R * kQ)
                *reinterpret_cast<float4*>(stage + (idx / kQ) * kLDK + 4 * (idx % kQ)) = pre[it];
        }
        stored(s);
    };

#pragma unroll
    for (int a = 0; a < G::FA; ++a)
#pragma unroll
        for (int b = 0; b < G::PB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    fetch(s0);
    store(s0);
    __syncthreads();
    for (int s = s0; s < s1; ++s) {
        if (s + 1 < s1) fetch(s + 1);        // in flight during the MFMAs
        // a half wave takes columns 8 g + 4 lh .. + 3 of each group g of 8: the depth order is a
        // permutation of the columns, the same for every pair
#pragma unroll
        for (int g = 0; g < kBK / 8; ++g) {
            float av[G::FA][4], bv[G::PB][4];
#pragma unroll
            for (int a = 0; a < G::FA; ++a) {
                const float4 v = *reinterpret_cast<const float4*>(
                    stage + ((t.wc * G::FA + a) * 32 + lr) * kLDK + 8 * g + 4 * lh);
                av[a][0] = v.x; av[a][1] = v.y; av[a][2] = v.z; av[a][3] = v.w;
            }
#pragma unroll
            for (int b = 0; b < G::PB; ++b) {
                const float4 v = *reinterpret_cast<const float4*>(
                    stage + (G::BN + t.acc_point(b)) * kLDK + 8 * g + 4 * lh);
                bv[b][0] = v.x; bv[b][1] = v.y; bv[b][2] = v.z; bv[b][3] = v.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int a = 0; a < G::FA; ++a)
#pragma unroll
                    for (int b = 0; b < G::PB; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][e], bv[b][e], acc[a][b], 0, 0, 0);
        }
        done(s);
        __syncthreads();                     // every wave has read the stage (and what came with it)
        if (s + 1 < s1) store(s + 1);
        __syncthreads();
    }
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
    const int64_t p0 = (int64_t)blockIdx.x * kBM;
    const int nkc = (d + kBK - 1) / kBK, nct = (k + kBN - 1) / kBN;
    f32x16 acc[2][2];
    stage_stream<RowGeom>(                   // nct * nkc < 2^31: checked on the host
        stage, 0, nct * nkc, acc,
        [&](int s, int row, int c4) __attribute__((always_inline)) {
            const int ct = s / nkc, col = (s - ct * nkc) * kBK + c4;
            return row < kBN ? load_row4(c, (int64_t)ct * kBN + row, k, d, col, vec_c)
                             : load_row4(x, p0 + (row - kBN), n, d, col, vec_x);
        },
        [&](int s) __attribute__((always_inline)) {
            const int ct = s / nkc;
            if (s - ct * nkc == 0 && t.tid < kBN) {      // a tile's first stage brings its norms
                const int64_t cid = (int64_t)ct * kBN + t.tid;
                cns[t.tid] = cid < k ? cn[cid] : 0.f;
            }
        },
        [&](int s) __attribute__((always_inline)) {
            const int ct = s / nkc;
            if (s - ct * nkc != nkc - 1) return;
#pragma unroll
            for (int a = 0; a < 2; ++a)                   // the tile's last stage: its dot products leave
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = t.acc_row(a, r);
                    const int64_t cid = (int64_t)ct * kBN + i;
                    if (cid < k) {
                        const float cnv = cns[i];
#pragma unroll
                        for (int b = 0; b < 2; ++b) on_key(b, acc[a][b][r], cnv, (int)cid);
                    }
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b][r] = 0.f;
                }
        });
}

}  // namespace imgrec
