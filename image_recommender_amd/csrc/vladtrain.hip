// vladtrain.hip — one training step of the SIFT-VLAD MLP encoder (include/imgrec_vladtrain.h; the
// reference's loop, vector_scripts/create_sift_vector.py:393-404, and its losses, :80-123).
//
// A step is a fixed sequence of launches on the caller's stream:
//   forward   per layer vladenc_linear_kernel<..> / vladenc_reduce_kernel (vladenc_kernels.h: the
//             forward pass's own, so its bytes) and vladtrain_finish_kernel, a workgroup per row:
//             LayerNorm, Mish and dropout, or F.normalize; it keeps y, the row statistics and the
//             post-dropout activation for the backward.
//   losses    G = X X^T as a product (below), vladtrain_diag_kernel, vladtrain_dist_kernel (a
//             workgroup per row: D_x in place over G, D_z by differences, the row's softmax sums, KL
//             term and Pearson moments), vladtrain_loss_kernel (one workgroup: the three losses
//             and the gradient's coefficients).
//   backward  vladtrain_dz_kernel (dL/du per row), vladtrain_normalize_bwd_kernel, then per layer
//             from the last: vladtrain_colsum_kernel (bias gradient), the weight gradient and the
//             data gradient as products over vladtrain_transpose_kernel's copies,
//             vladtrain_bwd_finish_kernel (a workgroup per row: dropout, Mish', LayerNorm backward)
//             and vladtrain_colsum_kernel again (gamma, beta).
//   update    vladtrain_adam_kernel over the flat parameter vector.
//
// A product C[i][j] = sum_k A[i][k] B[j][k] is vladenc_linear_kernel<4, 2, 2, 2> with A as the
// weights and B as the batch: its [feature][row] output is C row-major, so dW = dY^T A lands in
// nn.Linear's (out, in) layout in the gradient vector itself.  Both operands must have the depth
// contiguous, which load_row4 reads as whole 128-byte lines; where it is not (dY^T, A^T, W^T) a
// transposed copy is made first: a copy costs one pass over an operand that the product re-reads
// once per tile of the other, and keeps stage_stream's loader and LDS layout as they are.  The
// split rule (vladtrain_args.h) counts the tiles of both output axes, so the reference's dW_0
// (3 x 256 tiles) is one pass with no partial sums.
//
// Parameters, gradients and both Adam moments are four flat vectors in one layout
// (vladtrain_layout), so Adam is one elementwise launch.
//
// LDS: the GEMM's 55 KB; vladtrain_dist_kernel 48 KB (a row of u, D_x and D_z),
// vladtrain_dz_kernel 50 KB (a row of u, the row's float64 weights and 256 group sums), the finish kernels 16 / 32 KB.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "../../include/imgrec_vladtrain.h"
#include "dev_workspace.h"
#include "rows_tile.h"
#include "vladtrain_args.h"

struct vladtrain {
    int nlayers = 0;
    int widths[VLADENC_MAX_LAYERS + 1] = {};
    int hsum = 0;                // the hidden widths' sum: a row of `masks`
    vladtrain_config cfg = {};
    uint32_t thr = 0;            // floor(dropout * 2^24)
    float scale = 1.f;           // 1 / (1 - dropout)
    int device = 0;
    int64_t off[4 * VLADENC_MAX_LAYERS] = {};
    int64_t total = 0;
    imgrec::DevBuf<float> P, G, M, V;
    std::mutex mu;               // the step counter
    int64_t step = 0;
};

namespace imgrec {
namespace {

#include "vladenc_kernels.h"

struct SampleBits {
    uint64_t w[VLADTRAIN_MAX_BATCH / 64];
};
__device__ __forceinline__ bool sampled(const SampleBits& b, int i) { return (b.w[i >> 6] >> (i & 63)) & 1; }

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t v) {
    v ^= v >> 30;
    v *= 0xbf58476d1ce4e5b9ull;
    v ^= v >> 27;
    v *= 0x94d049bb133111ebull;
    v ^= v >> 31;
    return v;
}
// imgrec_vladtrain.h "mask": a = mix64(seed + golden * (step + 1)) comes from the host
__device__ __forceinline__ bool keep_at(uint64_t a, int layer, int row, int f, uint32_t thr) {
    const uint64_t b = mix64(a ^ ((uint64_t)(uint32_t)layer << 32 | (uint64_t)(uint32_t)row));
    return (uint32_t)(mix64(b + (uint64_t)f) >> 40) >= thr;
}

// Workgroup = row p of the launch's m (row r0 + p of the batch); ysum[feature][row] from the
// reduction.  The forward's vladenc_finish_kernel with what the backward needs kept: y, the row's
// (mean, sd) or (clamped norm, norm), and on a hidden layer dropout after Mish.
__global__ void __launch_bounds__(256)
vladtrain_finish_kernel(const float* __restrict__ ysum, int m, int N, const float* __restrict__ gamma,
                        const float* __restrict__ beta, float eps, int last, float* __restrict__ ykeep,
                        double* __restrict__ stats, float* __restrict__ dst, uint64_t a, int layer, int r0,
                        uint32_t thr, float scale) {
    __shared__ float y[VLADENC_MAX_WIDTH];
    __shared__ double red[2][4];
    const int tid = threadIdx.x, p = blockIdx.x;
    for (int f = tid; f < N; f += 256) {
        y[f] = ysum[(int64_t)f * m + p];
        ykeep[(int64_t)p * N + f] = y[f];
    }
    __syncthreads();
    float* const o = dst + (int64_t)p * N;
    if (!last) {
        double s = 0.0;
        for (int f = tid; f < N; f += 256) s += (double)y[f];
        const double mean = block_sum(s, red[0]) / N;
        s = 0.0;
        for (int f = tid; f < N; f += 256) {
            const double t = (double)y[f] - mean;
            s = fma(t, t, s);
        }
        const double sd = sqrt(block_sum(s, red[1]) / N + (double)eps);
        if (tid == 0) {
            stats[2 * p] = mean;
            stats[2 * p + 1] = sd;
        }
        for (int f = tid; f < N; f += 256) {
            const float v = (float)(((double)y[f] - mean) / sd);
            float h = mish(fmaf(v, gamma[f], beta[f]));
            if (thr) h = keep_at(a, layer, r0 + p, f, thr) ? h * scale : 0.f;
            o[f] = h;
        }
        return;
    }
    double s = 0.0;
    for (int f = tid; f < N; f += 256) s = fma((double)y[f], (double)y[f], s);
    const double raw = sqrt(block_sum(s, red[0])), nrm = fmax(raw, 1e-12);
    if (tid == 0) {
        stats[2 * p] = nrm;
        stats[2 * p + 1] = raw;
    }
    for (int f = tid; f < N; f += 256) o[f] = (float)((double)y[f] / nrm);
}

// out (C x R) = in (R x C) transposed, 32 x 32 tiles through LDS; block (32, 8)
__global__ void __launch_bounds__(256)
vladtrain_transpose_kernel(const float* __restrict__ in, int R, int C, float* __restrict__ out) {
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int q = threadIdx.y; q < 32; q += 8) {
        const int r = r0 + q, c = c0 + threadIdx.x;
        if (r < R && c < C) t[q][threadIdx.x] = in[(int64_t)r * C + c];
    }
    __syncthreads();
    for (int q = threadIdx.y; q < 32; q += 8) {
        const int c = c0 + q, r = r0 + threadIdx.x;
        if (r < R && c < C) out[(int64_t)c * R + r] = t[threadIdx.x][q];
    }
}

// masks[row][off + f] = keep of hidden layer `layer`
__global__ void __launch_bounds__(256)
vladtrain_mask_kernel(uint64_t a, int layer, int n, int N, uint32_t thr, uint8_t* __restrict__ masks, int stride,
                      int off) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * N) return;
    const int row = (int)(e / N), f = (int)(e % N);
    masks[(int64_t)row * stride + off + f] = keep_at(a, layer, row, f, thr) ? 1 : 0;
}

__global__ void __launch_bounds__(256) vladtrain_diag_kernel(const float* __restrict__ g, int n, float* __restrict__ diag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) diag[i] = g[(int64_t)i * n + i];
}

// |u_i - u_j| as an fp32 fmaf chain in ascending f; ui is row i in LDS
__device__ __forceinline__ float row_dist(const float* ui, const float* __restrict__ uj, int Nz) {
    float s = 0.f;
    for (int f = 0; f < Nz; ++f) {
        const float d = ui[f] - uj[f];
        s = fmaf(d, d, s);
    }
    return sqrtf(s);
}

enum { kSx = 0, kSz, kKl, kA, kB, kAA, kBB, kAB, kRowStats };

// Workgroup = row i.  g: G, whose row i becomes D_x's.  rowstats[i][kRowStats]: the row's softmax
// sums, its KL term and the raw moments of its sampled pairs (every pair from both of its rows).
__global__ void __launch_bounds__(256)
vladtrain_dist_kernel(float* __restrict__ g, const float* __restrict__ diag, const float* __restrict__ u, int n,
                      int Nz, SampleBits bits, double invT, double* __restrict__ rowstats) {
    __shared__ float ui[VLADENC_MAX_WIDTH];
    __shared__ float dxr[VLADTRAIN_MAX_BATCH], dzr[VLADTRAIN_MAX_BATCH];
    __shared__ double red[kRowStats][4];
    const int tid = threadIdx.x, i = blockIdx.x;
    for (int f = tid; f < Nz; f += 256) ui[f] = u[(int64_t)i * Nz + f];
    __syncthreads();
    const bool in_i = sampled(bits, i);
    const double gii = (double)diag[i];
    double s[kRowStats] = {};
    for (int j = tid; j < n; j += 256) {
        float dx = 0.f, dz = 0.f;
        if (j != i) {
            const double d2 = gii + (double)diag[j] - 2.0 * (double)g[(int64_t)i * n + j];
            dx = (float)sqrt(fmax(d2, 0.0));
            dz = row_dist(ui, u + (int64_t)j * Nz, Nz);
        }
        g[(int64_t)i * n + j] = dx;
        dxr[j] = dx;
        dzr[j] = dz;
        s[kSx] += exp(-(double)dx * invT);
        s[kSz] += exp(-(double)dz * invT);
        if (in_i && j != i && sampled(bits, j)) {
            const double a = dx, b = dz;
            s[kA] += a;
            s[kB] += b;
            s[kAA] = fma(a, a, s[kAA]);
            s[kBB] = fma(b, b, s[kBB]);
            s[kAB] = fma(a, b, s[kAB]);
        }
    }
    double tot[kRowStats];
#pragma unroll
    for (int q = 0; q < kRowStats; ++q) tot[q] = q == kKl ? 0.0 : block_sum(s[q], red[q]);
    const double lsx = log(tot[kSx]), lsz = log(tot[kSz]);
    double kl = 0.0;
    for (int j = tid; j < n; j += 256) {          // a thread re-reads only what it wrote
        const double lp = -(double)dxr[j] * invT - lsx, lq = -(double)dzr[j] * invT - lsz;
        kl = fma(exp(lp), lp - lq, kl);
    }
    tot[kKl] = block_sum(kl, red[kKl]);
    if (tid < kRowStats) rowstats[(int64_t)i * kRowStats + tid] = tot[tid];
}

enum { kAlpha = 0, kBeta, kMa, kMb, kCu };

// One workgroup: the rows' sums in row order, the three losses, the gradient's coefficients.
__global__ void __launch_bounds__(256)
vladtrain_loss_kernel(const double* __restrict__ rowstats, int n, int k, double wc, double wu, double T,
                      float* __restrict__ losses, double* __restrict__ coef) {
    __shared__ double red[kRowStats][4];
    double s[kRowStats] = {};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int q = kKl; q < kRowStats; ++q) s[q] += rowstats[(int64_t)i * kRowStats + q];
    double tot[kRowStats] = {};
#pragma unroll
    for (int q = kKl; q < kRowStats; ++q) tot[q] = block_sum(s[q], red[q]);
    if (threadIdx.x != 0) return;
    const double kk = (double)k * (double)k;
    const double ma = 0.5 * tot[kA] / kk, mb = 0.5 * tot[kB] / kk;
    const double saa = 0.5 * tot[kAA] - kk * ma * ma, sbb = 0.5 * tot[kBB] - kk * mb * mb;
    const double sab = 0.5 * tot[kAB] - kk * ma * mb;
    const double ra = sqrt(fmax(saa, 0.0)), rb = sqrt(fmax(sbb, 0.0)), den = ra * rb + 1e-8;
    const double lc = 1.0 - sab / den, lu = tot[kKl] / n;
    losses[0] = (float)(wc * lc + wu * lu);
    losses[1] = (float)lc;
    losses[2] = (float)lu;
    coef[kAlpha] = -wc / den;
    coef[kBeta] = rb > 0.0 ? wc * sab * ra / (den * den * rb) : 0.0;
    coef[kMa] = ma;
    coef[kMb] = mb;
    coef[kCu] = wu / ((double)n * T);
}

// Workgroup = row i: du[i][f] = sum_j w_ij (u_i[f] - u_j[f]), w_ij = (g_ij + g_ji) / D_z[i][j].
__global__ void __launch_bounds__(256)
vladtrain_dz_kernel(const float* __restrict__ dxm, const float* __restrict__ u, int n, int Nz, SampleBits bits,
                    double invT, const double* __restrict__ rowstats, const double* __restrict__ coef,
                    float* __restrict__ du) {
    __shared__ float ui[VLADENC_MAX_WIDTH];
    __shared__ double w[VLADTRAIN_MAX_BATCH + 256];
    const int tid = threadIdx.x, i = blockIdx.x;
    for (int f = tid; f < Nz; f += 256) ui[f] = u[(int64_t)i * Nz + f];
    __syncthreads();
    const bool in_i = sampled(bits, i);
    const double alpha = coef[kAlpha], beta = coef[kBeta], ma = coef[kMa], mb = coef[kMb], cu = coef[kCu];
    const double sxi = rowstats[(int64_t)i * kRowStats + kSx], szi = rowstats[(int64_t)i * kRowStats + kSz];
    for (int j = tid; j < n; j += 256) {
        double wj = 0.0;
        if (j != i) {
            const float dz = row_dist(ui, u + (int64_t)j * Nz, Nz);
            if (dz > 0.f) {
                const double a = dxm[(int64_t)i * n + j], b = dz;
                const double ex = exp(-a * invT), ez = exp(-b * invT);
                const double sxj = rowstats[(int64_t)j * kRowStats + kSx], szj = rowstats[(int64_t)j * kRowStats + kSz];
                double gq = cu * ((ex / sxi - ez / szi) + (ex / sxj - ez / szj));
                if (in_i && sampled(bits, j)) gq += alpha * (a - ma) + beta * (b - mb);
                wj = gq / b;
            }
        }
        w[j] = wj;
    }
    __syncthreads();
    // fw threads over the features, 256 / fw groups over j: group g adds j = g, g + groups, ... in
    // ascending order, then a feature's group sums are added in group order (fw = 256, one group,
    // for Nz >= 256; else the power of two at or above Nz)
    int fw = 256;
    while (fw / 2 >= Nz && fw > 1) fw >>= 1;
    const int groups = 256 / fw, fl = tid % fw, g = tid / fw;
    double* const gsum = w + VLADTRAIN_MAX_BATCH;          // 256 doubles after the weights
    for (int f0 = 0; f0 < Nz; f0 += fw) {                   // (one pass unless Nz > 256)
        const int f = f0 + fl;
        double acc = 0.0;
        if (f < Nz) {
            const double uf = ui[f];
#pragma unroll 4
            for (int j = g; j < n; j += groups) acc = fma(w[j], uf - (double)u[(int64_t)j * Nz + f], acc);
        }
        if (groups == 1) {
            if (f < Nz) du[(int64_t)i * Nz + f] = (float)acc;
            continue;
        }
        gsum[g * fw + fl] = acc;
        __syncthreads();
        if (g == 0 && f < Nz) {
            for (int q = 1; q < groups; ++q) acc += gsum[q * fw + fl];
            du[(int64_t)i * Nz + f] = (float)acc;
        }
    }
}

// Workgroup = row: dy = (du - u (u . du)) / |y|, u = y / |y| in float64; du / 1e-12 where the norm was clamped.
__global__ void __launch_bounds__(256)
vladtrain_normalize_bwd_kernel(const float* __restrict__ y, const double* __restrict__ stats, const float* __restrict__ du,
                               int N, float* __restrict__ dy) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * N;
    const double nrm = stats[2 * blockIdx.x], raw = stats[2 * blockIdx.x + 1];
    double s = 0.0;
    for (int f = tid; f < N; f += 256) s = fma((double)du[base + f], (double)y[base + f] / nrm, s);
    const double dot = raw >= 1e-12 ? block_sum(s, red) : 0.0;
    for (int f = tid; f < N; f += 256)
        dy[base + f] = (float)(((double)du[base + f] - (double)y[base + f] / nrm * dot) / nrm);
}

// Column sums over the batch in float64, 16 features x kColGroups row groups per workgroup: group g
// adds rows g, g + 16, ... in ascending order, then the 16 group sums of a feature are added in
// group order.  y == NULL: out0[f] = sum_r d[r][f].  Else the LayerNorm parameters: out0 (gamma) =
// sum_r d[r][f] v[r][f], out1 (beta) = sum_r d[r][f], v the forward's normalised value (recomputed
// from y and the row's mean and sd).
constexpr int kColGroups = 16;
__global__ void __launch_bounds__(256)
vladtrain_colsum_kernel(const float* __restrict__ d, const float* __restrict__ y, const double* __restrict__ stats,
                        int n, int N, float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ double part0[kColGroups][17], part1[kColGroups][17];
    const int fl = threadIdx.x & 15, g = threadIdx.x >> 4, f = blockIdx.x * 16 + fl;
    double s0 = 0.0, s1 = 0.0;
    if (f < N) {
        if (!y) {
#pragma unroll 4
            for (int r = g; r < n; r += kColGroups) s0 += (double)d[(int64_t)r * N + f];
        } else {
#pragma unroll 4
            for (int r = g; r < n; r += kColGroups) {
                const double dv = d[(int64_t)r * N + f];
                const float v = (float)(((double)y[(int64_t)r * N + f] - stats[2 * r]) / stats[2 * r + 1]);
                s0 = fma(dv, (double)v, s0);
                s1 += dv;
            }
        }
    }
    part0[g][fl] = s0;
    part1[g][fl] = s1;
    __syncthreads();
    if (g != 0 || f >= N) return;
    for (int q = 1; q < kColGroups; ++q) {
        s0 += part0[q][fl];
        s1 += part1[q][fl];
    }
    out0[f] = (float)s0;
    if (y) out1[f] = (float)s1;
}

// Workgroup = row p.  da: the gradient of the layer's post-dropout activation, replaced by the
// gradient of the LayerNorm's output (what the gamma / beta sums read); dy: of the layer's y.
__global__ void __launch_bounds__(256)
vladtrain_bwd_finish_kernel(float* __restrict__ da, const float* __restrict__ y, const double* __restrict__ stats, int N,
                            const float* __restrict__ gamma, const float* __restrict__ beta, uint64_t a, int layer,
                            uint32_t thr, float scale, float* __restrict__ dy) {
    __shared__ float vs[VLADENC_MAX_WIDTH], dvs[VLADENC_MAX_WIDTH];
    __shared__ double red[2][4];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int64_t base = (int64_t)p * N;
    const double mean = stats[2 * p], sd = stats[2 * p + 1];
    double s1 = 0.0, s2 = 0.0;
    for (int f = tid; f < N; f += 256) {
        const float v = (float)(((double)y[base + f] - mean) / sd);
        const float zh = fmaf(v, gamma[f], beta[f]);
        float d = da[base + f];
        if (thr) d = keep_at(a, layer, p, f, thr) ? d * scale : 0.f;
        const double x = zh;
        double md = 1.0;                       // Mish' = tanh(sp) + x sech^2(sp) sigmoid(x); 1 past the threshold
        if (!(zh > 20.f)) {
            const double t = tanh(log1p(exp(x)));
            md = t + x * (1.0 - t * t) / (1.0 + exp(-x));
        }
        const float dzh = (float)((double)d * md);
        da[base + f] = dzh;
        const float dv = dzh * gamma[f];
        vs[f] = v;
        dvs[f] = dv;
        s1 += (double)dv;
        s2 = fma((double)dv, (double)v, s2);
    }
    const double m1 = block_sum(s1, red[0]) / N, m2 = block_sum(s2, red[1]) / N;
    for (int f = tid; f < N; f += 256)         // a thread re-reads only what it wrote
        dy[base + f] = (float)(((double)dvs[f] - m1 - (double)vs[f] * m2) / sd);
}

// out[e] = (p_0[e] + p_1[e]) + ... in ascending split order: vladenc_reduce_kernel without the bias
__global__ void __launch_bounds__(256)
vladtrain_reduce_kernel(const float* __restrict__ part, int64_t total, int nsplit, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) out[e] = split_sum(part + e, total, nsplit);
}

struct AdamArgs {
    double b1, b2, wd, eps, step_size, bc2_sqrt;
};
// torch.optim.Adam on every element of the flat vectors, float64 from the fp32 state
__global__ void __launch_bounds__(256)
vladtrain_adam_kernel(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M, float* __restrict__ V,
                      int64_t total, AdamArgs c) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const double p = P[e], g = fma(c.wd, p, (double)G[e]);
    const double m = c.b1 * (double)M[e] + (1.0 - c.b1) * g;
    const double v = c.b2 * (double)V[e] + (1.0 - c.b2) * g * g;
    M[e] = (float)m;
    V[e] = (float)v;
    P[e] = (float)(p - c.step_size * m / (sqrt(v) / c.bc2_sqrt + c.eps));
}

// ---- host side ----------------------------------------------------------------------------------

struct Workspace : StreamHandoff {
    DevBuf<float> part, xt, gram, keep, wide[3], wt, u;
    DevBuf<double> dbl;
};

enum { kStep = 0, kGrads = 1, kEval = 2 };

// C (I x J, row-major) = A (I x K) B^T (B is J x K), imgrec_vladtrain.h "products"
int product(Workspace* w, const float* A, int I, const float* B, int J, int K, float* out, hipStream_t st) {
    const ProdSplit p = vladtrain_split(I, J, K);
    const bool split = p.sp.nsplit > 1;
    int rc = launch_linear<4, 2, 2, 2>(B, J, K, A, I, p.sp, split ? w->part.get() : out, st);
    if (rc != KNN_OK || !split) return rc;
    const int64_t total = (int64_t)I * J;
    hipLaunchKernelGGL(vladtrain_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w->part.get(),
                       total, p.sp.nsplit, out);
    KNN_HIP(hipGetLastError());
    return KNN_OK;
}

int transpose(const float* in, int R, int C, float* out, hipStream_t st) {
    hipLaunchKernelGGL(vladtrain_transpose_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32)), dim3(32, 8),
                       0, st, in, R, C, out);
    KNN_HIP(hipGetLastError());
    return KNN_OK;
}

// the four flat vectors' slots of tensor `slot` (vladtrain_layout) and its element count
int64_t slot_count(const vladtrain* h, int slot) {
    const int l = slot / 4, which = slot % 4;
    const int64_t K = h->widths[l], N = h->widths[l + 1];
    if (which == 0) return N * K;
    return which == 1 || l < h->nlayers - 1 ? N : 0;
}

// the launches of one call on `st` (w->mu held); `step` is the counter the masks and Adam use
int run_locked(Workspace* w, vladtrain* h, const float* x, int n, const SampleBits& bits, int k, int mode,
               int64_t step, float* losses, float* z, uint8_t* masks, hipStream_t st) {
    const int L = h->nlayers;
    const int* wd = h->widths;
    const TrainSizes sz = vladtrain_sizes(L, wd, n);
    const int nout = wd[L];
    int rc;
    if ((rc = w->part.reserve((size_t)std::max<int64_t>(sz.part, 1))) != KNN_OK) return rc;
    if ((rc = w->gram.reserve((size_t)sz.gram)) != KNN_OK) return rc;
    if ((rc = w->keep.reserve((size_t)sz.keep)) != KNN_OK) return rc;
    if ((rc = w->u.reserve((size_t)n * nout)) != KNN_OK) return rc;
    if ((rc = w->dbl.reserve((size_t)sz.doubles)) != KNN_OK) return rc;
    if (mode != kEval) {
        if ((rc = w->xt.reserve((size_t)sz.xt)) != KNN_OK) return rc;
        if ((rc = w->wt.reserve((size_t)std::max<int64_t>(sz.wt, 1))) != KNN_OK) return rc;
        for (auto& b : w->wide)
            if ((rc = b.reserve((size_t)sz.wide)) != KNN_OK) return rc;
    }
    // the kept values: per layer y, then (hidden layers) the activation; then G's diagonal (n floats)
    float *ykeep[VLADENC_MAX_LAYERS], *act[VLADENC_MAX_LAYERS];
    float* at = w->keep.get();
    for (int l = 0; l < L; ++l) {
        ykeep[l] = at;
        at += (int64_t)n * wd[l + 1];
        act[l] = l < L - 1 ? at : nullptr;
        if (l < L - 1) at += (int64_t)n * wd[l + 1];
    }
    float* const diag = at;
    double* const stats = w->dbl.get();                       // layer l: stats + 2 n l
    double* const rowstats = stats + (int64_t)2 * n * L;
    double* const coef = rowstats + (int64_t)n * kRowStats;
    const uint32_t thr = mode == kEval ? 0u : h->thr;
    const uint64_t a = mix64(h->cfg.seed + 0x9e3779b97f4a7c15ull * ((uint64_t)step + 1));
    const float eps = (float)h->cfg.ln_eps;
    float* const P = h->P.get();
    float* const G = h->G.get();

    // ---- forward
    const char* e = test_knob("IMGREC_VLADENC_CHUNK_ROWS");
    const long long knob = e ? std::atoll(e) : 0;
    const int chunk = vladenc_knob_set(knob) ? std::min((int)knob, n) : n;
    const float* in = x;
    for (int l = 0; l < L; ++l) {
        const int K = wd[l], N = wd[l + 1], rows = vladenc_layer_rows(K, N, chunk);
        const EncSplit sp = vladenc_split(K, N);
        const bool last = l == L - 1;
        float* const dst = last ? w->u.get() : act[l];
        for (int r0 = 0; r0 < n; r0 += rows) {
            const int m = std::min(rows, n - r0);
            const float* xin = in + (int64_t)r0 * K;
            rc = m <= 32 ? launch_linear<8, 1, 1, 1>(xin, m, K, P + h->off[4 * l], N, sp, w->part, st)
                         : launch_linear<4, 2, 2, 2>(xin, m, K, P + h->off[4 * l], N, sp, w->part, st);
            if (rc != KNN_OK) return rc;
            hipLaunchKernelGGL(vladenc_reduce_kernel, dim3((unsigned)(((int64_t)N * m + 255) / 256)), dim3(256), 0, st,
                               w->part.get(), m, N, sp.nsplit, P + h->off[4 * l + 1]);
            KNN_HIP(hipGetLastError());
            hipLaunchKernelGGL(vladtrain_finish_kernel, dim3((unsigned)m), dim3(256), 0, st, w->part.get(), m, N,
                               last ? nullptr : P + h->off[4 * l + 2], last ? nullptr : P + h->off[4 * l + 3], eps,
                               last ? 1 : 0, ykeep[l] + (int64_t)r0 * N, stats + (int64_t)2 * n * l + 2 * r0,
                               dst + (int64_t)r0 * N, a, l, r0, thr, h->scale);
            KNN_HIP(hipGetLastError());
        }
        in = dst;
    }
    const float* const u = w->u.get();
    if (z) KNN_HIP(hipMemcpyAsync(z, u, (size_t)n * nout * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (masks) {
        int hoff = 0;
        for (int l = 0; l < L - 1; ++l) {
            const int N = wd[l + 1];
            hipLaunchKernelGGL(vladtrain_mask_kernel, dim3((unsigned)(((int64_t)n * N + 255) / 256)), dim3(256), 0, st, a,
                               l, n, N, thr, masks, h->hsum, hoff);
            KNN_HIP(hipGetLastError());
            hoff += N;
        }
    }

    // ---- losses
    const double T = h->cfg.temperature, invT = 1.0 / T;
    if ((rc = product(w, x, n, x, n, wd[0], w->gram, st)) != KNN_OK) return rc;
    hipLaunchKernelGGL(vladtrain_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w->gram.get(), n, diag);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(vladtrain_dist_kernel, dim3((unsigned)n), dim3(256), 0, st, w->gram.get(), diag, u, n, nout, bits,
                       invT, rowstats);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(vladtrain_loss_kernel, dim3(1), dim3(256), 0, st, rowstats, n, k, (double)h->cfg.corr_weight,
                       (double)h->cfg.umap_weight, T, losses, coef);
    KNN_HIP(hipGetLastError());
    if (mode == kEval) return KNN_OK;

    // ---- backward
    if (mode == kGrads)                                       // a slot that no kernel writes must show: NaN bytes first
        for (int slot = 0; slot < 4 * L; ++slot)
            if (const int64_t count = slot_count(h, slot))
                KNN_HIP(hipMemsetAsync(G + h->off[slot], 0xFF, (size_t)count * sizeof(float), st));
    float *dy = w->wide[1].get(), *s1 = w->wide[2].get(), *s2 = w->wide[0].get();
    hipLaunchKernelGGL(vladtrain_dz_kernel, dim3((unsigned)n), dim3(256), 0, st, w->gram.get(), u, n, nout, bits, invT,
                       rowstats, coef, s2);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(vladtrain_normalize_bwd_kernel, dim3((unsigned)n), dim3(256), 0, st, ykeep[L - 1],
                       stats + (int64_t)2 * n * (L - 1), s2, nout, dy);
    KNN_HIP(hipGetLastError());
    if ((rc = transpose(x, n, wd[0], w->xt, st)) != KNN_OK) return rc;
    for (int l = L - 1; l >= 0; --l) {
        const int K = wd[l], N = wd[l + 1];
        hipLaunchKernelGGL(vladtrain_colsum_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, st, dy, nullptr,
                           nullptr, n, N, G + h->off[4 * l + 1], nullptr);
        KNN_HIP(hipGetLastError());
        // dW = dY^T A: features = dY^T's N rows, batch rows = A^T's K rows, depth n
        if ((rc = transpose(dy, n, N, s1, st)) != KNN_OK) return rc;
        const float* at = w->xt.get();
        if (l > 0) {
            if ((rc = transpose(act[l - 1], n, K, s2, st)) != KNN_OK) return rc;
            at = s2;
        }
        if ((rc = product(w, s1, N, at, K, n, G + h->off[4 * l], st)) != KNN_OK) return rc;
        if (l == 0) break;
        // dA = dY W: features = dY's n rows, batch rows = W^T's K rows, depth N
        if ((rc = transpose(P + h->off[4 * l], N, K, w->wt, st)) != KNN_OK) return rc;
        if ((rc = product(w, dy, n, w->wt, K, N, s1, st)) != KNN_OK) return rc;
        const int q = l - 1;                                  // the hidden layer whose output A is
        hipLaunchKernelGGL(vladtrain_bwd_finish_kernel, dim3((unsigned)n), dim3(256), 0, st, s1, ykeep[q],
                           stats + (int64_t)2 * n * q, K, P + h->off[4 * q + 2], P + h->off[4 * q + 3], a, q, thr, h->scale,
                           s2);
        KNN_HIP(hipGetLastError());
        hipLaunchKernelGGL(vladtrain_colsum_kernel, dim3((unsigned)((K + 15) / 16)), dim3(256), 0, st, s1, ykeep[q],
                           stats + (int64_t)2 * n * q, n, K, G + h->off[4 * q + 2], G + h->off[4 * q + 3]);
        KNN_HIP(hipGetLastError());
        std::swap(dy, s2);
    }
    if (mode != kStep) return KNN_OK;

    // ---- update
    const double t = (double)(step + 1), b1 = h->cfg.beta1, b2 = h->cfg.beta2;
    const AdamArgs c = {b1, b2, h->cfg.weight_decay, h->cfg.adam_eps, h->cfg.lr / (1.0 - std::pow(b1, t)),
                        std::sqrt(1.0 - std::pow(b2, t))};
    hipLaunchKernelGGL(vladtrain_adam_kernel, dim3((unsigned)((h->total + 255) / 256)), dim3(256), 0, st, P, G,
                       h->M.get(), h->V.get(), h->total, c);
    KNN_HIP(hipGetLastError());
    return KNN_OK;
}

// checks, then the launches on the handle's device; the step counter advances when a step is enqueued
int run_device(vladtrain* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k, int mode, float* losses,
               float* z, uint8_t* masks, hipStream_t st, const char* who, bool host_arrays) {
    char msg[256];
    if (vladtrain_check_call(h, x, n, sample_idx, k, losses, who, msg, sizeof msg) != 0) KNN_FAIL(KNN_EINVAL, "%s", msg);
    std::vector<unsigned char> seen((size_t)n);
    int kk = 0;
    if (vladtrain_check_sample(h->widths[0], n, sample_idx, k, seen.data(), &kk, who, msg, sizeof msg) != 0)
        KNN_FAIL(KNN_EINVAL, "%s", msg);
    SampleBits bits = {};
    for (int i = 0; i < (int)n; ++i)
        if (seen[i]) bits.w[i >> 6] |= uint64_t(1) << (i & 63);
    DeviceGuard g(h->device);
    std::lock_guard<std::mutex> lk(h->mu);
    const int64_t step = h->step;
    int rc;
    if (!host_arrays) {
        rc = on_workspace<Workspace>(
            st, [&](Workspace* w) { return run_locked(w, h, x, (int)n, bits, kk, mode, step, losses, z, masks, st); });
    } else {
        const size_t nx = (size_t)n * h->widths[0], nz = (size_t)n * h->widths[h->nlayers], nm = (size_t)n * h->hsum;
        DevBuf<float> xd, ld, zd;
        DevBuf<uint8_t> md;
        if ((rc = xd.reserve(nx)) != KNN_OK) return rc;
        if ((rc = ld.reserve(3)) != KNN_OK) return rc;
        if (z && (rc = zd.reserve(nz)) != KNN_OK) return rc;
        const bool want_masks = masks && nm > 0;
        if (want_masks && (rc = md.reserve(nm)) != KNN_OK) return rc;
        StreamGuard sg;       // declared after the buffers: the stream is drained before they are freed
        KNN_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
        KNN_HIP(hipMemcpyAsync(xd, x, nx * sizeof(float), hipMemcpyHostToDevice, sg.s));
        rc = on_workspace<Workspace>(sg.s, [&](Workspace* w) {
            return run_locked(w, h, xd, (int)n, bits, kk, mode, step, ld, z ? zd.get() : nullptr,
                              want_masks ? md.get() : nullptr, sg.s);
        });
        if (rc != KNN_OK) return rc;
        KNN_HIP(hipMemcpyAsync(losses, ld, 3 * sizeof(float), hipMemcpyDeviceToHost, sg.s));
        if (z) KNN_HIP(hipMemcpyAsync(z, zd, nz * sizeof(float), hipMemcpyDeviceToHost, sg.s));
        if (want_masks) KNN_HIP(hipMemcpyAsync(masks, md, nm, hipMemcpyDeviceToHost, sg.s));
        KNN_HIP(hipStreamSynchronize(sg.s));
    }
    if (rc == KNN_OK && mode == kStep) h->step = step + 1;
    return rc;
}

int copy_state(vladtrain* h, int which, float* const* W, float* const* b, float* const* gamma, float* const* beta,
               bool set, const char* who) {
    char msg[256];
    if (!h) KNN_FAIL(KNN_EINVAL, "%s: NULL handle", who);
    if (vladtrain_check_which(which, set, who, msg, sizeof msg) != 0) KNN_FAIL(KNN_EINVAL, "%s", msg);
    if (!W || !b || (h->nlayers > 1 && (!gamma || !beta))) KNN_FAIL(KNN_EINVAL, "%s: NULL W, b, gamma or beta", who);
    for (int l = 0; l < h->nlayers; ++l)
        if (!W[l] || !b[l] || (l < h->nlayers - 1 && (!gamma[l] || !beta[l])))
            KNN_FAIL(KNN_EINVAL, "%s: NULL array of layer %d", who, l);
    DeviceGuard g(h->device);
    std::lock_guard<std::mutex> lk(h->mu);
    KNN_HIP(hipDeviceSynchronize());
    float* const base = (which == VLADTRAIN_PARAMS ? h->P : which == VLADTRAIN_ADAM_M ? h->M
                         : which == VLADTRAIN_ADAM_V ? h->V : h->G).get();
    for (int l = 0; l < h->nlayers; ++l) {
        float* const host[4] = {W[l], b[l], l < h->nlayers - 1 ? gamma[l] : nullptr, l < h->nlayers - 1 ? beta[l] : nullptr};
        for (int q = 0; q < 4; ++q) {
            const size_t bytes = (size_t)slot_count(h, 4 * l + q) * sizeof(float);
            if (!bytes) continue;
            float* const dev = base + h->off[4 * l + q];
            if (set) KNN_HIP(hipMemcpy(dev, host[q], bytes, hipMemcpyHostToDevice));
            else KNN_HIP(hipMemcpy(host[q], dev, bytes, hipMemcpyDeviceToHost));
        }
    }
    return KNN_OK;
}

}  // namespace
}  // namespace imgrec

using namespace imgrec;

extern "C" {

int vladtrain_default_config(vladtrain_config* cfg) {
    if (!cfg) KNN_FAIL(KNN_EINVAL, "vladtrain_default_config: NULL config");
    *cfg = vladtrain_config{0.1, 1e-3, 0.9, 0.999, 1e-8, 1e-5, 2.0, 0.25, 1.5, 1e-5, 0};
    return KNN_OK;
}

int vladtrain_create(int nlayers, const int* widths, const float* const* W, const float* const* b,
                     const float* const* gamma, const float* const* beta, const vladtrain_config* cfg,
                     int device, vladtrain_t** out) {
    char msg[256];
    if (vladtrain_check_create(nlayers, widths, W, b, gamma, beta, cfg, out, "vladtrain_create", msg, sizeof msg) != 0)
        KNN_FAIL(KNN_EINVAL, "%s", msg);
    *out = nullptr;
    int rc = have_device();
    if (rc != KNN_OK) return rc;
    int ndev = 0;
    KNN_HIP(hipGetDeviceCount(&ndev));
    if (device >= ndev) KNN_FAIL(KNN_EINVAL, "vladtrain_create: device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    vladtrain* h = new vladtrain();
    struct Drop {
        vladtrain* h;
        ~Drop() { delete h; }
    } drop{h};
    h->nlayers = nlayers;
    h->cfg = *cfg;
    h->thr = (uint32_t)std::floor(cfg->dropout * 16777216.0);
    h->scale = h->thr ? (float)(1.0 / (1.0 - cfg->dropout)) : 1.f;
    KNN_HIP(hipGetDevice(&h->device));
    for (int l = 0; l <= nlayers; ++l) h->widths[l] = widths[l];
    for (int l = 1; l < nlayers; ++l) h->hsum += widths[l];
    h->total = vladtrain_layout(nlayers, widths, h->off);
    for (DevBuf<float>* v : {&h->P, &h->G, &h->M, &h->V}) {
        if ((rc = v->reserve((size_t)h->total)) != KNN_OK) return rc;
        KNN_HIP(hipMemset(v->get(), 0, (size_t)h->total * sizeof(float)));
    }
    drop.h = nullptr;
    *out = h;
    rc = copy_state(h, VLADTRAIN_PARAMS, const_cast<float* const*>(W), const_cast<float* const*>(b),
                    const_cast<float* const*>(gamma), const_cast<float* const*>(beta), true, "vladtrain_create");
    if (rc != KNN_OK) {
        *out = nullptr;
        delete h;
    }
    return rc;
}

int vladtrain_free(vladtrain_t* h) {
    if (!h) return KNN_OK;
    {
        // calls still in flight read the parameters: the device is drained before they go
        DeviceGuard g(h->device);
        (void)hipDeviceSynchronize();
    }
    delete h;
    return KNN_OK;
}

int vladtrain_step_device(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                          void* stream, float* losses) {
    return run_device(h, x, n, sample_idx, k, kStep, losses, nullptr, nullptr, (hipStream_t)stream,
                      "vladtrain_step_device", false);
}

int vladtrain_step(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k, float* losses) {
    return run_device(h, x, n, sample_idx, k, kStep, losses, nullptr, nullptr, nullptr, "vladtrain_step", true);
}

int vladtrain_grads_device(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                           void* stream, float* losses, float* z, uint8_t* masks) {
    return run_device(h, x, n, sample_idx, k, kGrads, losses, z, masks, (hipStream_t)stream, "vladtrain_grads_device",
                      false);
}

int vladtrain_grads(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k, float* losses,
                    float* z, uint8_t* masks) {
    return run_device(h, x, n, sample_idx, k, kGrads, losses, z, masks, nullptr, "vladtrain_grads", true);
}

int vladtrain_eval_device(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                          void* stream, float* losses) {
    return run_device(h, x, n, sample_idx, k, kEval, losses, nullptr, nullptr, (hipStream_t)stream,
                      "vladtrain_eval_device", false);
}

int vladtrain_eval(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k, float* losses) {
    return run_device(h, x, n, sample_idx, k, kEval, losses, nullptr, nullptr, nullptr, "vladtrain_eval", true);
}

int vladtrain_get_state(vladtrain_t* h, int which, float* const* W, float* const* b, float* const* gamma,
                        float* const* beta) {
    return copy_state(h, which, W, b, gamma, beta, false, "vladtrain_get_state");
}

int vladtrain_set_state(vladtrain_t* h, int which, const float* const* W, const float* const* b,
                        const float* const* gamma, const float* const* beta) {
    return copy_state(h, which, const_cast<float* const*>(W), const_cast<float* const*>(b),
                      const_cast<float* const*>(gamma), const_cast<float* const*>(beta), true, "vladtrain_set_state");
}

int vladtrain_get_step(const vladtrain_t* h, int64_t* step) {
    if (!h || !step) KNN_FAIL(KNN_EINVAL, "vladtrain_get_step: NULL handle or step");
    std::lock_guard<std::mutex> lk(const_cast<vladtrain_t*>(h)->mu);
    *step = h->step;
    return KNN_OK;
}

int vladtrain_set_step(vladtrain_t* h, int64_t step) {
    if (!h) KNN_FAIL(KNN_EINVAL, "vladtrain_set_step: NULL handle");
    if (step < 0 || step > (int64_t(1) << 52)) KNN_FAIL(KNN_EINVAL, "vladtrain_set_step: step must be in [0, 2^52] (got %lld)", (long long)step);
    std::lock_guard<std::mutex> lk(h->mu);
    h->step = step;
    return KNN_OK;
}

int vladtrain_product_device(const float* A, int64_t I, const float* B, int64_t J, int64_t K, float* C, void* stream) {
    char msg[256];
    if (vladtrain_check_product(A, I, B, J, K, C, "vladtrain_product_device", msg, sizeof msg) != 0)
        KNN_FAIL(KNN_EINVAL, "%s", msg);
    const int rc = have_device();
    if (rc != KNN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return on_workspace<Workspace>(st, [&](Workspace* w) {
        const int rc = w->part.reserve((size_t)std::max<int64_t>(vladtrain_part_floats((int)I, (int)J, (int)K), 1));
        return rc != KNN_OK ? rc : product(w, A, (int)I, B, (int)J, (int)K, C, st);
    });
}

int64_t vladtrain_workspace_bytes(int nlayers, const int* widths, int64_t n) {
    if (nlayers < 1 || nlayers > VLADENC_MAX_LAYERS || !widths) KNN_FAIL(KNN_EINVAL, "vladtrain_workspace_bytes: bad nlayers or NULL widths");
    for (int l = 0; l <= nlayers; ++l)
        if (widths[l] < 1 || widths[l] > (l == 0 ? VLADENC_MAX_IN : VLADENC_MAX_WIDTH))
            KNN_FAIL(KNN_EINVAL, "vladtrain_workspace_bytes: widths[%d] = %d out of range", l, widths[l]);
    if (n < 2 || n > VLADTRAIN_MAX_BATCH || n * (int64_t)widths[0] > (int64_t)VLADTRAIN_MAX_BATCH_FLOATS)
        KNN_FAIL(KNN_EINVAL, "vladtrain_workspace_bytes: n = %lld out of range", (long long)n);
    return vladtrain_workspace_total(nlayers, widths, n);
}

}  // extern "C"
