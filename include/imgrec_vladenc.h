/*
 * imgrec_vladenc.h — C ABI of the SIFT-VLAD MLP encoder's forward pass on the MI355X.
 *
 * The reference pushes every image's 32768-d VLAD vector (imgrec_vlad.h) through SIFTVLADEncoder
 * (vector_scripts/create_sift_vector.py:59-77),
 *     Linear(32768, 669) -> LayerNorm -> Mish -> Linear(669, 317) -> LayerNorm -> Mish -> Linear(317, 128),
 * then F.normalize, and compute_vectors (:514-521) divides the result once more by its norm + 1e-7;
 * that 128-d vector is what it stores and searches.  image_recommender_amd.vlad_encoder serves the
 * forward pass from the entry points below (csrc/vladenc.hip).  Training: imgrec_vladtrain.h.
 *
 * Conventions: those of imgrec_knn.h / imgrec_vlad.h.  Every function returns 0 or a negative KNN_E*
 * code (imgrec_knn.h enum knn_error) and leaves its message in knn_last_error(); streams are
 * hipStream_t passed as void* (NULL = the null stream); every argument is checked on the host before
 * any GPU call, so a bad argument is KNN_EINVAL on a machine without a GPU.  Arrays are row-major.
 *
 * Arithmetic.  Every product and accumulation is fp32 (no input or weight is rounded to a narrower
 * type) except the reductions named float64 below; there are no float atomics.
 *   linear       layer l has depth K = widths[l] and N = widths[l + 1] features.  The depth is cut
 *                into stages of 32 columns and the stages into S(K, N) splits of equal stage count
 *                (the last may be shorter); S and the cut are functions of (K, N) only:
 *                    T = ceil(N / 256), stages = ceil(K / 32),
 *                    S0 = min(max(1, 512 / T), max(1, stages / 4)),
 *                    per = ceil(stages / S0), S = ceil(stages / per),
 *                split s = stages [s per, min((s + 1) per, stages)).  Inside a split a dot product
 *                is one fmaf chain from 0 on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), stage by
 *                stage in ascending order and inside a stage in the column order
 *                0 4 1 5 2 6 3 7, 8 12 9 13 ... (columns past K contribute +0 products).  The S
 *                partial sums are added sequentially in ascending split order, then the bias is added:
 *                y = ((p_0 + p_1) + ... + p_{S-1}) + b.
 *   LayerNorm    mean = sum_f y_f / N and var = sum_f (y_f - mean)^2 / N (biased) in float64: thread
 *                t of 256 adds features t, t + 256, ... in ascending order, a wave's 64 sums meet in
 *                the xor butterfly 32, 16, ..., 1 and the four wave sums are added in wave order.
 *                v = (y - mean) / sqrt(var + ln_eps) in float64, rounded to fp32 once, then
 *                fmaf(v, gamma, beta) in fp32.
 *   Mish         x * tanhf(softplus(x)) in fp32, softplus(x) = x for x > 20 (torch's threshold) and
 *                log1pf(expf(x)) otherwise.
 *   output       z = last layer's y.  s = sum_f z_f^2 in float64 in the order of the LayerNorm sums;
 *                u = z / max(sqrt(s), 1e-12) in float64, rounded to fp32 once: F.normalize, what
 *                VLADENC_MODEL_OUTPUT returns.  By default s2 = sum_f u_f^2 the same way over the
 *                rounded u and out = u / (sqrt(s2) + 1e-7) in float64, rounded to fp32 once.
 *
 * Determinism and batch invariance.  Every output row is a pure function of its input row and the
 * weights: the orders above depend on a layer's (widths[l], widths[l + 1]) only, never on n, the
 * row's position, the row chunking, the tile shape, the grid or scheduling.  A row encoded alone,
 * inside any batch or in another chunk gives the same bytes; two calls give the same bytes.
 *
 * Workspace.  Split partial sums and the hidden activations live in a per-device workspace shared
 * by all handles and calls on the device (ordered across streams by an event).  It is bounded
 * independently of n: a batch runs in chunks of VLADENC_SUPER_ROWS rows, whose hidden activations
 * the workspace holds (two layers' worth), and inside a chunk every layer runs as many row tiles of
 * VLADENC_CHUNK_ROWS per launch as keep its partial sums within VLADENC_CHUNK_ROWS x 512 x 256
 * floats (64 MiB), at least one tile: the reference's first layer takes 128 rows per launch, its
 * later layers the whole chunk.
 */
#ifndef IMGREC_VLADENC_H
#define IMGREC_VLADENC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum vladenc_flags {
    VLADENC_MODEL_OUTPUT = 1   /* stop after F.normalize: the model's own output, not the stored vector */
};

#define VLADENC_MAX_LAYERS 8
#define VLADENC_MAX_WIDTH 4096        /* hidden and output widths: a row's LayerNorm fits one workgroup */
#define VLADENC_MAX_IN (1 << 20)      /* input width */
#define VLADENC_CHUNK_ROWS 128        /* a row tile: the unit a layer's launches count rows in */
#define VLADENC_SUPER_ROWS 2048       /* rows per chunk */

typedef struct vladenc vladenc_t;

/* An encoder of `nlayers` linear layers on HIP device `device` (-1 = current); the weights are
 * copied to the device here and stay resident.
 *   widths  int[nlayers + 1]       widths[0] the input width, widths[nlayers] the output width
 *   W       nlayers host pointers  W[l] is widths[l + 1] x widths[l] float32 (nn.Linear's layout)
 *   b       nlayers host pointers  b[l] is float32[widths[l + 1]]
 *   gamma, beta  nlayers - 1 host pointers each: the LayerNorm after layer l < nlayers - 1
 *                (may be NULL when nlayers = 1)
 *   ln_eps  the LayerNorms' eps (>= 0, finite)
 * Every layer but the last is followed by LayerNorm, then Mish. */
int vladenc_create(int nlayers, const int* widths, const float* const* W, const float* const* b,
                   const float* const* gamma, const float* const* beta, float ln_eps, int device,
                   vladenc_t** out);

int vladenc_free(vladenc_t* h);

/* out[0 .. nlayers] = the widths; *nlayers = the layer count (either may be NULL) */
int vladenc_widths(const vladenc_t* h, int* out, int* nlayers);

/* The forward pass over device-resident rows on `stream` (a stream of the handle's device);
 * nothing waits on the host.
 *   x       n x widths[0] float32
 *   out     n x widths[nlayers] float32
 *   hidden  n x (widths[1] + ... + widths[nlayers - 1]) float32, or NULL: per row the post-Mish
 *           activation of every hidden layer, concatenated in layer order
 * n = 0 is allowed (nothing is written).  IMGREC_VLADENC_CHUNK_ROWS=<rows> (tests; 1 ..
 * VLADENC_CHUNK_ROWS), read when the call starts, overrides the chunk size (and with it every
 * layer's rows per launch); the outputs do not depend on it. */
int vladenc_forward_device(vladenc_t* h, const float* x, int64_t n, int flags, float* out, float* hidden,
                           void* stream);

/* The same over host arrays: uploads, calls vladenc_forward_device on a stream of its own,
 * downloads and waits. */
int vladenc_forward(vladenc_t* h, const float* x, int64_t n, int flags, float* out, float* hidden);

#ifdef __cplusplus
}
#endif

#endif /* IMGREC_VLADENC_H */
