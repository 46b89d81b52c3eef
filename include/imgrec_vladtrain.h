/*
 * imgrec_vladtrain.h — C ABI of one training step of the SIFT-VLAD MLP encoder on the MI355X.
 *
 * The reference trains SIFTVLADEncoder (imgrec_vladenc.h) before it can store a single SIFT vector
 * (vector_scripts/create_sift_vector.py:393-404, the losses at :80-123): per step one batch X of B
 * VLAD vectors,
 *     z = model(X)  (training mode),  D_x = cdist(X, X),  D_z = cdist(z, z),
 *     loss = 2.0 * loss_corr(D_x, D_z, sample_k = 1024) + 0.25 * loss_umap(D_x, D_z, T = 1.5),
 *     loss.backward(),  Adam(lr = 1e-3, weight_decay = 1e-5).step().
 * image_recommender_amd.vlad_trainer serves that step from the entry points below
 * (csrc/vladtrain.hip).  The quirks named below are the reference's and are reproduced.
 *
 * Conventions: those of imgrec_vladenc.h.  Every function returns 0 or a negative KNN_E* code and
 * leaves its message in knn_last_error(); streams are hipStream_t passed as void*; every argument is
 * checked on the host before any GPU call, so a bad argument is KNN_EINVAL on a machine without a
 * GPU.  Arrays are row-major; parameter arrays are passed as in vladenc_create.
 *
 * Arithmetic.  Every product is exact fp32 on v_mfma_f32_32x32x2_f32; every scalar reduction is
 * float64 in a fixed order; there are no float atomics.  "row sum" below is the workgroup sum of
 * imgrec_vladenc.h's LayerNorm: thread t of 256 adds elements t, t + 256, ... in ascending order,
 * a wave's 64 sums meet in the xor butterfly 32, 16, ..., 1, the four wave sums are added in wave order.
 *   forward      imgrec_vladenc.h's linear / LayerNorm / Mish chain, same split rule and orders.
 *                After Mish on every hidden layer l (0-based), dropout: h' = keep ? h * s : 0 with
 *                s = (float)(1 / (1 - p)) in fp32; with p = 0 nothing is multiplied.  The model
 *                output u = F.normalize(y_last) is VLADENC_MODEL_OUTPUT's, byte for byte at p = 0.
 *   mask         keep(seed, step, l, row, f), all arithmetic modulo 2^64:
 *                    mix(v): v ^= v >> 30; v *= 0xbf58476d1ce4e5b9; v ^= v >> 27;
 *                            v *= 0x94d049bb133111eb; v ^= v >> 31              (splitmix64's)
 *                    a = mix(seed + 0x9e3779b97f4a7c15 * (step + 1))
 *                    b = mix(a ^ ((uint64)l << 32 | (uint64)row))
 *                    c = mix(b + f)
 *                    keep = (c >> 40) >= floor(p * 2^24)                       (p the double given)
 *                `step` is the handle's counter when the call starts (0 for the first step).  The
 *                mask depends on nothing else: not on chunking, grid or stream.
 *   products     A product C[i][j] = sum_k A[i][k] B[j][k] of depth K with I x J outputs is the
 *                forward's fmaf chain (stage order, column order 0 4 1 5 2 6 3 7 ...), cut into
 *                S splits whose partial sums are added in ascending order:
 *                    T = ceil(I / 256) * ceil(J / 128), stages = ceil(K / 32),
 *                    S0 = min(max(1, 512 / T), max(1, stages / 4)),
 *                    per = ceil(stages / S0), S = ceil(stages / per).
 *                The weight gradient dW_l = dY_l^T A_l (I = N, J = K, depth B), the data gradient
 *                dA_l = dY_l W_l (I = B, J = K, depth N; not for l = 0) and the Gram matrix
 *                G = X X^T (I = J = B) run this way over transposed copies where the depth is an
 *                operand's slow axis.  The reference's dW_0 (669 x 32768, depth B >= 32) is S = 1.
 *   D_x          G is bitwise symmetric (the chain's products commute).  D_x[i][j] =
 *                sqrt(max(G[i][i] + G[j][j] - 2 G[i][j], 0)) in float64 from the fp32 G, rounded to
 *                fp32; D_x[i][i] = 0.  Bitwise-equal rows are at distance exactly 0.  X is data: no
 *                gradient.
 *   D_z          D_z[i][j] = sqrtf(sum_f (u_i[f] - u_j[f])^2), an fp32 fmaf chain in ascending f.
 *   loss_corr    1 - Pearson(D_x.triu(1).flatten(), D_z.triu(1).flatten()) over the k x k
 *                restriction to sample_idx (all rows without one), with the reference's quirk: the
 *                vectors have k^2 entries, the zeros of the diagonal and the lower triangle
 *                included in the means and sums.  Computed from the raw moments of the pairs in
 *                float64: row i sums a, b, a^2, b^2, ab over its pairs (row sum), a single workgroup
 *                adds the rows' sums (row sum over i), every pair is counted twice and halved.
 *                corr = S_ab / (sqrt(S_aa) sqrt(S_bb) + 1e-8).
 *   loss_umap    kl_div(log softmax(-D_z / T, 1), softmax(-D_x / T, 1), "batchmean") over all B rows,
 *                diagonal included; the largest logit of a row is its diagonal's 0, so the
 *                softmax sums are plain row sums of exp in float64.
 *   loss         corr_weight * loss_corr + umap_weight * loss_umap.  losses[3] = {loss, loss_corr,
 *                loss_umap}, rounded to fp32 once.
 *   backward     dL/du_i = sum_j (g_ij + g_ji) (u_i - u_j) / D_z[i][j] in float64 (0 where
 *                D_z[i][j] = 0, as torch.cdist's backward), rounded to fp32: with fw = 256 for an
 *                output width >= 256, else the power of two at or above it, group g of 256 / fw adds
 *                j = g, g + 256 / fw, ... in ascending order and the group sums are added in group
 *                order.  "column sum" below: over the batch in float64, row group g of 16 adds rows
 *                g, g + 16, ... in ascending order, the 16 group sums are added in group order.  Through
 *                F.normalize in float64 (two row sums); through each layer: bias gradient = the
 *                column sum of dY; the products above; dropout, Mish'
 *                (float64, at the fp32 pre-activation) and the LayerNorm backward (biased variance,
 *                its two row sums) in one workgroup per row; gamma / beta gradients = column sums
 *                of dz and dz v.  The forward keeps each layer's pre-LayerNorm y,
 *                its mean and sd (float64) and the post-dropout activation; masks are regenerated.
 *   Adam         torch.optim.Adam: g += weight_decay * p (L2, not AdamW); m = b1 m + (1 - b1) g;
 *                v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),
 *                t = step + 1.  Every element in float64 from the fp32 state, each of p, m, v
 *                rounded to fp32 once; one kernel over all parameters (biases, gamma and beta too).
 *
 * Determinism.  The same parameters, batch, sample_idx, seed and step give the same bytes whatever
 * the stream or IMGREC_VLADENC_CHUNK_ROWS (which chunks the forward's launches as in
 * imgrec_vladenc.h).  Batch invariance does not apply: the loss couples the rows.
 *
 * Limits.  2 <= n <= VLADTRAIN_MAX_BATCH rows per step, n * widths[0] <= VLADTRAIN_MAX_BATCH_FLOATS;
 * the widths as in imgrec_vladenc.h.  sample_idx: NULL (all rows), or k distinct indices in
 * [0, n), 2 <= k <= n, in any order, a HOST array in every entry point (it is checked, and packed
 * into the launches' arguments, before the call returns).
 *
 * Workspace.  Per device, shared by all handles (dev_workspace.h), a function of (widths, n) only
 * and largest at n = VLADTRAIN_MAX_BATCH: the transposed batch (n * widths[0] floats, at most 1 GiB),
 * G / D_x (n^2 floats), per hidden layer y and the activation, three n x max-width gradient
 * buffers, one transposed weight matrix of a later layer, and at most 64 MiB of split partial sums
 * (as the forward's).  vladtrain_workspace_bytes returns the sum.
 */
#ifndef IMGREC_VLADTRAIN_H
#define IMGREC_VLADTRAIN_H

#include <stdint.h>

#include "imgrec_vladenc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VLADTRAIN_MAX_BATCH 4096
#define VLADTRAIN_MAX_BATCH_FLOATS (1 << 28)

/* hyper-parameters; vladtrain_default_config fills the reference's */
typedef struct vladtrain_config {
    double dropout;        /* 0.1   in [0, 1); below 2^-24 is no dropout */
    double lr;             /* 1e-3 */
    double beta1, beta2;   /* 0.9, 0.999   in [0, 1) */
    double adam_eps;       /* 1e-8 */
    double weight_decay;   /* 1e-5 */
    double corr_weight;    /* 2.0 */
    double umap_weight;    /* 0.25 */
    double temperature;    /* 1.5   > 0 */
    double ln_eps;         /* 1e-5, rounded to fp32 as in imgrec_vladenc.h */
    uint64_t seed;         /* of the dropout masks */
} vladtrain_config;

enum vladtrain_state {
    VLADTRAIN_PARAMS = 0,  /* the parameters */
    VLADTRAIN_ADAM_M = 1,  /* Adam's first moments (exp_avg) */
    VLADTRAIN_ADAM_V = 2,  /* Adam's second moments (exp_avg_sq) */
    VLADTRAIN_GRADS = 3    /* the gradients of the last step or vladtrain_grads call (get only) */
};

typedef struct vladtrain vladtrain_t;

int vladtrain_default_config(vladtrain_config* cfg);

/* A trainer from initial parameters (as vladenc_create's; copied to the device), zero moments and
 * step 0. */
int vladtrain_create(int nlayers, const int* widths, const float* const* W, const float* const* b,
                     const float* const* gamma, const float* const* beta, const vladtrain_config* cfg,
                     int device, vladtrain_t** out);

int vladtrain_free(vladtrain_t* h);

/* One step over device-resident x (n x widths[0] float32) on `stream`: forward with dropout, both
 * losses, backward, Adam; the step counter advances.  losses: DEVICE float[3].  Nothing waits on
 * the host. */
int vladtrain_step_device(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                          void* stream, float* losses);

/* The same over a host batch and host losses[3]: uploads, steps on a stream of its own, waits. */
int vladtrain_step(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                   float* losses);

/* The step's forward, losses and backward at the current step counter, without the update; the
 * gradients stay in the handle (vladtrain_get_state(VLADTRAIN_GRADS)), which is filled with NaN
 * bytes first, so a slot that no kernel wrote shows.  Optional outputs (NULL to
 * skip), on the device: z (n x widths[nlayers]) the model output u; masks (n x hidden width sum,
 * uint8, layers concatenated per row) 1 where kept. */
int vladtrain_grads_device(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                           void* stream, float* losses, float* z, uint8_t* masks);

/* The same over host arrays. */
int vladtrain_grads(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                    float* losses, float* z, uint8_t* masks);

/* The losses of a batch in eval mode: no dropout, no gradients, no update. */
int vladtrain_eval_device(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                          void* stream, float* losses);

int vladtrain_eval(vladtrain_t* h, const float* x, int64_t n, const int32_t* sample_idx, int64_t k,
                   float* losses);

/* Copies one of enum vladtrain_state to / from host arrays laid out as vladtrain_create's; waits
 * for the device first.  VLADTRAIN_GRADS cannot be set. */
int vladtrain_get_state(vladtrain_t* h, int which, float* const* W, float* const* b, float* const* gamma,
                        float* const* beta);
int vladtrain_set_state(vladtrain_t* h, int which, const float* const* W, const float* const* b,
                        const float* const* gamma, const float* const* beta);

/* the number of steps taken (Adam's t - 1 of the next step; the masks' `step`) */
int vladtrain_get_step(const vladtrain_t* h, int64_t* step);
int vladtrain_set_step(vladtrain_t* h, int64_t step);

/* One product of the step alone (the "products" rule above), for tests and measurement:
 * C (I x J) = A (I x K) B^T, B being J x K, all device-resident float32 on `stream`.
 * 1 <= I <= VLADENC_MAX_WIDTH, 1 <= J, K <= VLADENC_MAX_IN.  It runs on the CURRENT device: the
 * pointers and the stream must belong to it. */
int vladtrain_product_device(const float* A, int64_t I, const float* B, int64_t J, int64_t K, float* C,
                             void* stream);

/* the workspace a step of n rows needs, in bytes (< 0: an error code) */
int64_t vladtrain_workspace_bytes(int nlayers, const int* widths, int64_t n);

#ifdef __cplusplus
}
#endif

#endif /* IMGREC_VLADTRAIN_H */
