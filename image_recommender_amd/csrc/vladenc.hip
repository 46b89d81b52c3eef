// vladenc.hip — the forward pass of the SIFT-VLAD MLP encoder (include/imgrec_vladenc.h; the
// reference's SIFTVLADEncoder and compute_vectors, vector_scripts/create_sift_vector.py:59-77, 514-521).
//
// A batch runs in chunks of VLADENC_SUPER_ROWS rows; inside a chunk a layer is three launches on the
// caller's stream per group of row tiles (as many as keep the partial sums within 64 MiB: one tile
// of 128 rows for the reference's first layer, the whole chunk for its later layers):
//   1. vladenc_linear_kernel<..>  grid = feature tiles (256) x depth splits x row tiles.  A plain GEMM
//                                 on rows_tile.h's stage_stream, the loop kmeans_assign_kernel and
//                                 vlad_nn_kernel run: the weight rows are the MFMA's A rows, the batch
//                                 rows its columns, 32 depth columns per stage (load_row4's guarded
//                                 loads for ragged K, N and batch).  The kernel itself is the index
//                                 arithmetic, the stage's load and the epilogue.
//                                 A workgroup streams only its split's stages and leaves its
//                                 accumulators, one fmaf chain per (row, feature), in the workspace as
//                                 part[split][feature][row]: a lane owns a batch row, so a register's
//                                 64 stores are two 128-byte runs.  Two shapes of the same chain: 128
//                                 batch rows (4 x 2 waves, 2 x 2 accumulators each) and, for chunks
//                                 of at most 32 rows, 32 batch rows (8 x 1 waves, one accumulator
//                                 each), which spends a quarter of the MFMA work on the B = 1 weight
//                                 stream.  The chain of an element is the same in both, so which one
//                                 runs changes no byte.
//   2. vladenc_reduce_kernel      a thread per (feature, row): the splits' partial sums added in
//                                 ascending order, then the bias, in place over split 0.  Its loads
//                                 are contiguous and 16 are in flight per thread: at B = 1 the 147
//                                 partial sums of a feature would otherwise be 147 round trips.
//   3. vladenc_finish_kernel      a workgroup per row: LayerNorm and Mish or, on the last layer, the
//                                 two normalisations (float64 sums in the fixed order the header
//                                 documents), the activation to the workspace (or `out`) and to `hidden`.
//
// The split rule, the chunk rule and the argument checks are vladenc_args.h (host-checked under
// sanitizers).  At the reference's widths the first layer is 3 tiles x 147 splits = 441 workgroups
// whatever the batch; the later layers are 2 x 5 and 1 x 2.
//
// LDS: (256 + 128) x 36 floats = 55 KB, (256 + 32) x 36 = 41 KB for the narrow shape; the finish
// kernel holds a row (16 KB).  Registers per kernel: profiles/vladenc/.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../include/imgrec_vladenc.h"
#include "dev_workspace.h"
#include "rows_tile.h"
#include "vladenc_args.h"

struct vladenc {
    int nlayers = 0;
    int widths[VLADENC_MAX_LAYERS + 1] = {};
    int hsum = 0;                // the hidden widths' sum: a row of `hidden`
    int hmax = 1;                // the widest hidden layer
    float eps = 0.f;
    int device = 0;
    imgrec::DevBuf<float> W[VLADENC_MAX_LAYERS], b[VLADENC_MAX_LAYERS], g[VLADENC_MAX_LAYERS], be[VLADENC_MAX_LAYERS];
};

namespace imgrec {
namespace {

enum { kHidden = 0, kModelOutput = 1, kStored = 2 };     // what the finish kernel does after the bias

// vladenc_linear_kernel<..>, vladenc_reduce_kernel, launch_linear, mish, block_sum
#include "vladenc_kernels.h"

// Workgroup = row p of the chunk's m; ysum[feature][row] from the reduction.  dst: the row's N
// outputs; hid: its N slots of `hidden` or NULL.
__global__ void __launch_bounds__(256)
vladenc_finish_kernel(const float* __restrict__ ysum, int m, int N,
                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int mode,
                      float* __restrict__ dst, int64_t dst_stride, float* __restrict__ hid, int64_t hid_stride) {
    __shared__ float y[VLADENC_MAX_WIDTH];
    __shared__ double red[3][4];
    const int tid = threadIdx.x, p = blockIdx.x;
    for (int f = tid; f < N; f += 256) y[f] = ysum[(int64_t)f * m + p];
    __syncthreads();
    float* const o = dst + p * dst_stride;
    if (mode == kHidden) {
        double a = 0.0;
        for (int f = tid; f < N; f += 256) a += (double)y[f];
        const double mean = block_sum(a, red[0]) / N;
        a = 0.0;
        for (int f = tid; f < N; f += 256) {
            const double t = (double)y[f] - mean;
            a = fma(t, t, a);
        }
        const double sd = sqrt(block_sum(a, red[1]) / N + (double)eps);
        for (int f = tid; f < N; f += 256) {
            const float v = (float)(((double)y[f] - mean) / sd);
            const float h = mish(fmaf(v, gamma[f], beta[f]));
            o[f] = h;
            if (hid) hid[p * hid_stride + f] = h;
        }
        return;
    }
    double a = 0.0;
    for (int f = tid; f < N; f += 256) a = fma((double)y[f], (double)y[f], a);
    const double nrm = fmax(sqrt(block_sum(a, red[0])), 1e-12);
    a = 0.0;
    for (int f = tid; f < N; f += 256) {       // a thread re-reads only what it wrote
        const float u = (float)((double)y[f] / nrm);
        y[f] = u;
        a = fma((double)u, (double)u, a);
    }
    if (mode == kModelOutput) {
        for (int f = tid; f < N; f += 256) o[f] = y[f];
        return;
    }
    const double den = sqrt(block_sum(a, red[1])) + 1e-7;
    for (int f = tid; f < N; f += 256) o[f] = (float)((double)y[f] / den);
}

// ---- host side ----------------------------------------------------------------------------------

// what the calls on a device share (dev_workspace.h), whichever handle they belong to
struct Workspace : StreamHandoff {
    DevBuf<float> part;
    DevBuf<float> act[2];
};

// the launches on `st` (w->mu held)
int forward_locked(Workspace* w, const vladenc* h, const float* x, int64_t n, int flags, float* out, float* hidden,
                   hipStream_t st) {
    const char* e = test_knob("IMGREC_VLADENC_CHUNK_ROWS");
    const int L = h->nlayers, chunk = (int)std::min<int64_t>(vladenc_chunk_rows(e ? std::atoll(e) : 0), n);
    int64_t pf = 1;
    for (int l = 0; l < L; ++l) {
        const int K = h->widths[l], N = h->widths[l + 1];
        pf = std::max(pf, vladenc_part_floats(K, N, vladenc_layer_rows(K, N, chunk)));
    }
    int rc;
    if ((rc = w->part.reserve((size_t)pf)) != KNN_OK) return rc;
    for (int i = 0; i < 2; ++i)
        if ((rc = w->act[i].reserve((size_t)chunk * h->hmax)) != KNN_OK) return rc;
    const int nout = h->widths[L];
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int M = (int)std::min<int64_t>(chunk, n - c0);
        const float* in = x + c0 * h->widths[0];
        int hoff = 0;
        for (int l = 0; l < L; ++l) {
            const int K = h->widths[l], N = h->widths[l + 1], rows = vladenc_layer_rows(K, N, chunk);
            const EncSplit sp = vladenc_split(K, N);
            const bool last = l == L - 1;
            float* const dst = last ? out + c0 * nout : w->act[l & 1].get();
            float* const hid = !last && hidden ? hidden + c0 * h->hsum + hoff : nullptr;
            const int mode = !last ? kHidden : (flags & VLADENC_MODEL_OUTPUT) ? kModelOutput : kStored;
            for (int r0 = 0; r0 < M; r0 += rows) {
                const int m = std::min(rows, M - r0);
                const float* xin = in + (int64_t)r0 * K;
                rc = m <= 32 ? launch_linear<8, 1, 1, 1>(xin, m, K, h->W[l], N, sp, w->part, st)
                             : launch_linear<4, 2, 2, 2>(xin, m, K, h->W[l], N, sp, w->part, st);
                if (rc != KNN_OK) return rc;
                hipLaunchKernelGGL(vladenc_reduce_kernel, dim3((unsigned)(((int64_t)N * m + 255) / 256)), dim3(256), 0,
                                   st, w->part.get(), m, N, sp.nsplit, h->b[l].get());
                KNN_HIP(hipGetLastError());
                hipLaunchKernelGGL(vladenc_finish_kernel, dim3((unsigned)m), dim3(256), 0, st, w->part.get(), m, N,
                                   last ? nullptr : h->g[l].get(), last ? nullptr : h->be[l].get(), h->eps, mode,
                                   dst + (int64_t)r0 * N, (int64_t)N, hid ? hid + (int64_t)r0 * h->hsum : nullptr,
                                   (int64_t)h->hsum);
                KNN_HIP(hipGetLastError());
            }
            in = dst;
            hoff += N;
        }
    }
    return KNN_OK;
}

int check_forward(const vladenc* h, const float* x, int64_t n, int flags, const float* out, const char* who) {
    char msg[256];
    if (vladenc_check_forward(h, x, n, flags, out, who, msg, sizeof msg) != 0) KNN_FAIL(KNN_EINVAL, "%s", msg);
    return KNN_OK;
}

// on the handle's device (set by the caller)
int forward_device_impl(vladenc* h, const float* x, int64_t n, int flags, float* out, float* hidden, hipStream_t st) {
    return on_workspace<Workspace>(
        st, [&](Workspace* w) { return forward_locked(w, h, x, n, flags, out, hidden, st); });
}

}  // namespace
}  // namespace imgrec

using namespace imgrec;

extern "C" {

int vladenc_create(int nlayers, const int* widths, const float* const* W, const float* const* b,
                   const float* const* gamma, const float* const* beta, float ln_eps, int device,
                   vladenc_t** out) {
    char msg[256];
    if (vladenc_check_create(nlayers, widths, W, b, gamma, beta, ln_eps, out, "vladenc_create", msg, sizeof msg) != 0)
        KNN_FAIL(KNN_EINVAL, "%s", msg);
    *out = nullptr;
    int rc = have_device();
    if (rc != KNN_OK) return rc;
    int ndev = 0;
    KNN_HIP(hipGetDeviceCount(&ndev));
    if (device >= ndev) KNN_FAIL(KNN_EINVAL, "vladenc_create: device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    vladenc* h = new vladenc();
    struct Drop {
        vladenc* h;
        ~Drop() { delete h; }
    } drop{h};
    h->nlayers = nlayers;
    h->eps = ln_eps;
    KNN_HIP(hipGetDevice(&h->device));
    for (int l = 0; l <= nlayers; ++l) h->widths[l] = widths[l];
    for (int l = 1; l < nlayers; ++l) {
        h->hsum += widths[l];
        h->hmax = std::max(h->hmax, widths[l]);
    }
    auto upload = [](DevBuf<float>& d, const float* src, size_t count) -> int {
        const int rc = d.reserve(count);
        if (rc != KNN_OK) return rc;
        KNN_HIP(hipMemcpy(d.get(), src, count * sizeof(float), hipMemcpyHostToDevice));
        return KNN_OK;
    };
    for (int l = 0; l < nlayers; ++l) {
        const size_t K = (size_t)widths[l], N = (size_t)widths[l + 1];
        if ((rc = upload(h->W[l], W[l], N * K)) != KNN_OK) return rc;
        if ((rc = upload(h->b[l], b[l], N)) != KNN_OK) return rc;
        if (l < nlayers - 1) {
            if ((rc = upload(h->g[l], gamma[l], N)) != KNN_OK) return rc;
            if ((rc = upload(h->be[l], beta[l], N)) != KNN_OK) return rc;
        }
    }
    drop.h = nullptr;
    *out = h;
    return KNN_OK;
}

int vladenc_free(vladenc_t* h) {
    if (!h) return KNN_OK;
    {
        // calls still in flight read the weights: the device is drained before they go
        DeviceGuard g(h->device);
        (void)hipDeviceSynchronize();
    }
    delete h;
    return KNN_OK;
}

int vladenc_widths(const vladenc_t* h, int* out, int* nlayers) {
    if (!h) KNN_FAIL(KNN_EINVAL, "vladenc_widths: NULL handle");
    if (out)
        for (int l = 0; l <= h->nlayers; ++l) out[l] = h->widths[l];
    if (nlayers) *nlayers = h->nlayers;
    return KNN_OK;
}

int vladenc_forward_device(vladenc_t* h, const float* x, int64_t n, int flags, float* out, float* hidden,
                           void* stream) {
    const int rc = check_forward(h, x, n, flags, out, "vladenc_forward_device");
    if (rc != KNN_OK || n == 0) return rc;
    DeviceGuard g(h->device);
    return forward_device_impl(h, x, n, flags, out, hidden, (hipStream_t)stream);
}

int vladenc_forward(vladenc_t* h, const float* x, int64_t n, int flags, float* out, float* hidden) {
    int rc = check_forward(h, x, n, flags, out, "vladenc_forward");
    if (rc != KNN_OK || n == 0) return rc;
    DeviceGuard g(h->device);
    const size_t nx = (size_t)n * h->widths[0], no = (size_t)n * h->widths[h->nlayers], nh = (size_t)n * h->hsum;
    DevBuf<float> xd, od, hd;
    if ((rc = xd.reserve(nx)) != KNN_OK) return rc;
    if ((rc = od.reserve(no)) != KNN_OK) return rc;
    const bool want_hidden = hidden && nh > 0;
    if (want_hidden && (rc = hd.reserve(nh)) != KNN_OK) return rc;
    StreamGuard sg;       // declared after the buffers: the stream is drained before they are freed
    KNN_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    KNN_HIP(hipMemcpyAsync(xd, x, nx * sizeof(float), hipMemcpyHostToDevice, sg.s));
    if ((rc = forward_device_impl(h, xd, n, flags, od, want_hidden ? hd.get() : nullptr, sg.s)) != KNN_OK) return rc;
    KNN_HIP(hipMemcpyAsync(out, od, no * sizeof(float), hipMemcpyDeviceToHost, sg.s));
    if (want_hidden) KNN_HIP(hipMemcpyAsync(hidden, hd, nh * sizeof(float), hipMemcpyDeviceToHost, sg.s));
    KNN_HIP(hipStreamSynchronize(sg.s));
    return KNN_OK;
}

}  // extern "C"
