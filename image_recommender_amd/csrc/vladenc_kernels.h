// vladenc_kernels.h — the encoder's GEMM and the device helpers that the forward pass (vladenc.hip)
// and the training step (vladtrain.hip) share: vladenc_linear_kernel<..> on rows_tile.h's
// stage_stream, the split reduction (split_sum: one summation order for both files), Mish and the
// workgroup sum.  One definition, so the training forward's bytes are the forward's.  Included by those two .hip files inside
// `namespace imgrec { namespace {`: every translation unit gets kernels of its own.
#pragma once

// Waves per SIMD the 128-row shape is compiled for.  4 = two workgroups per CU: 128 VGPRs with 12
// of its 160 spilled to scratch, and still 6 % faster at B = 1024 than one workgroup per CU
// (-DVLADENC_WIDE_WAVES=1; profiles/vladenc/), because a neighbour's MFMAs cover a workgroup's
// first load, barriers and stores.
#ifndef VLADENC_WIDE_WAVES
#define VLADENC_WIDE_WAVES 4
#endif

// FW x PW waves over the features and the batch rows, FA x PB accumulators of 32 x 32 per wave
template <int FW, int PW, int FA, int PB>
__global__ void __launch_bounds__(kNT, FA * PB == 4 ? VLADENC_WIDE_WAVES : 1)
vladenc_linear_kernel(const float* __restrict__ x, int m, int K, const float* __restrict__ W, int N, int per,
                      int stages, int vec_x, int vec_w, float* __restrict__ part) {
    using G = StageGeom<FW, PW, FA, PB>;
    static_assert(G::BN == kBN, "one feature tile of the split rule");
    __shared__ __attribute__((aligned(16))) float stage[G::R * kLDK];
    const int f0 = blockIdx.x * G::BN, split = blockIdx.y, p0 = blockIdx.z * G::BM;
    const int s0 = split * per, s1 = min(s0 + per, stages);

    f32x16 acc[FA][PB];
    stage_stream<G>(
        stage, s0, s1, acc,
        [&](int s, int row, int c4) __attribute__((always_inline)) {
            return row < G::BN ? load_row4(W, (int64_t)f0 + row, N, K, s * kBK + c4, vec_w)
                               : load_row4(x, (int64_t)p0 + (row - G::BN), m, K, s * kBK + c4, vec_x);
        },
        [](int) {}, [](int) {});
    // part[split][feature][row]: a lane's batch row is the fastest index
    const StageLanes<G> t;
#pragma unroll
    for (int a = 0; a < FA; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = f0 + t.acc_row(a, r);
#pragma unroll
            for (int b = 0; b < PB; ++b) {
                const int p = p0 + t.acc_point(b);
                if (i < N && p < m) part[((int64_t)split * N + i) * m + p] = acc[a][b][r];
            }
        }
}

// softplus with torch's threshold, then x tanh(.)
__device__ __forceinline__ float mish(float x) {
    const float sp = x > 20.f ? x : log1pf(expf(x));
    return x * tanhf(sp);
}

// The sum of v over the workgroup's 256 threads: a wave's butterfly, then the four wave sums in
// wave order.  `red` is 4 doubles of LDS that no other sum uses.
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ((p[0] + p[total]) + p[2 total]) + ... over nsplit partial sums `total` floats apart, sequentially
// in ascending split order: the one summation order of every split product.  kRedUnroll loads are
// in flight before the additions take them (at B = 1 the 147 partial sums of a feature would
// otherwise be 147 round trips).
constexpr int kRedUnroll = 16;
__device__ __forceinline__ float split_sum(const float* __restrict__ p, int64_t total, int nsplit) {
    float t = p[0];
    int s = 1;
    for (; s + kRedUnroll <= nsplit; s += kRedUnroll) {
        float v[kRedUnroll];
#pragma unroll
        for (int q = 0; q < kRedUnroll; ++q) v[q] = p[(s + q) * total];
#pragma unroll
        for (int q = 0; q < kRedUnroll; ++q) t += v[q];
    }
    for (; s < nsplit; ++s) t += p[s * total];
    return t;
}

// part[split][feature][row] -> part[0][feature][row] = split_sum + bias, in place: a thread per
// (feature, row), whose S loads are contiguous across the wave.
__global__ void __launch_bounds__(256)
vladenc_reduce_kernel(float* __restrict__ part, int m, int N, int nsplit, const float* __restrict__ bias) {
    const int64_t total = (int64_t)N * m, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    part[e] = split_sum(part + e, total, nsplit) + bias[e / m];
}

// one launch of the GEMM: feature tiles x sp.nsplit splits x row tiles, partial sums to `part`
template <int FW, int PW, int FA, int PB>
int launch_linear(const float* x, int m, int K, const float* W, int N, const EncSplit& sp, float* part,
                  hipStream_t st) {
    constexpr int BM = PW * PB * 32;
    auto* kern = vladenc_linear_kernel<FW, PW, FA, PB>;
    hipLaunchKernelGGL(kern, dim3((unsigned)sp.tiles, (unsigned)sp.nsplit, (unsigned)((m + BM - 1) / BM)), dim3(kNT),
                       0, st, x, m, K, W, N, sp.per, sp.stages, row4_vec(x, K), row4_vec(W, K), part);
    KNN_HIP(hipGetLastError());
    return KNN_OK;
}
