/*
 * imgrec_vlad.h — C ABI of the soft-assignment VLAD encoding of local descriptors on the MI355X.
 *
 * The reference aggregates an image's (up to 1000) RootSIFT descriptors against a 256-word
 * vocabulary into a 256 x 128 VLAD vector (vector_scripts/create_sift_vector.py:448-475,
 * _compute_sift_vlad_worker): the 4 nearest words of every descriptor, a weight
 * exp(-dist / (2 sigma^2)) each, the weighted residuals summed per word, then a per-word L2
 * normalisation, a signed square root and a global L2 normalisation.  image_recommender_amd.vlad
 * serves that loop from the entry points below (csrc/vlad.hip); the vocabulary comes from
 * imgrec_kmeans.h.
 *
 * Conventions: those of imgrec_knn.h / imgrec_kmeans.h.  Every function returns 0 or a negative
 * KNN_E* code (imgrec_knn.h enum knn_error) and leaves its message in knn_last_error(); streams are
 * hipStream_t passed as void* (NULL = the null stream); every argument is checked on the host before
 * any GPU call, so a bad argument is KNN_EINVAL on a machine without a GPU.  Arrays are row-major.
 *
 * Per descriptor x (a row of `x`):
 *   neighbours   the nn codebook rows with the smallest fp32 key |c|^2 - 2 x.c (x.c on the exact-fp32
 *                MFMA, one summation order for every pair: the k-means kernel's convention), an exact
 *                tie to the smaller id, listed best first in (key, id) order.  Two bitwise-equal
 *                codebook rows have bitwise-equal keys, so the smaller id is always listed first.
 *   distance     |x - c|^2 of a listed row, summed directly in fp32 (not the key; >= 0): lane l of a
 *                wave adds columns l, l + 64, ... in ascending order with fmaf, then the 64 lane sums
 *                meet in a fixed xor butterfly (offsets 32, 16, ..., 1).
 *   weight       w = expf(-distance / t), t = 2 sigma^2 computed in float64 and rounded to fp32 once.
 * Per image i (descriptors offsets[i] .. offsets[i + 1] - 1) and codebook row c:
 *   raw          V[c][:] = sum_j w_jc (x_j - C[c])  over the image's descriptors j that list c, taken
 *                sequentially in ascending descriptor order from 0: V = fmaf(w, x - C, V) per
 *                member and coordinate.  A row nobody lists is exactly 0.  VLAD_RAW stops here.
 *   epilogue     s_c = sum_col V[c][col]^2 and a_c = sum_col |V[c][col]| in float64 (lane l of a wave
 *                adds columns l, l + 64, ... in ascending order, then the xor butterfly 32 .. 1);
 *                r_c = sqrt(s_c); g = sqrt(sum_c a_c / r_c) over the rows with r_c > 0 (float64:
 *                thread t of 256 adds rows t, t + 256, ... in ascending order, then the 256 sums are
 *                added in thread order): that is the L2 norm of the signed square roots.
 *                out = sign(V) * sqrt(|V| / r_c) / g, computed in float64 and rounded to fp32 once.
 *                A row with r_c = 0 stays 0; with g = 0 the whole vector is 0.
 * An image without descriptors yields the zero vector.
 *
 * Determinism and batch invariance: no float atomics.  Every output is a pure function of the
 * inputs; the orders above depend on d, k and the image's own descriptors only: not on the image's
 * position in the batch, the other images, the grid, the cluster tiling or scheduling.  Encoding an
 * image alone and inside a batch gives the same bytes; two calls give the same bytes.
 *
 * Limits: N < 2^31 descriptors and nimg < 2^31 images per call; 1 <= nn <= VLAD_MAX_NN and nn <= k;
 * 1 <= d <= VLAD_MAX_D (one codebook row's accumulator must fit the CU's LDS; k is tiled over
 * workgroups, so k * d is bounded only by the memory of the output).  Neither an image's descriptor
 * count, k nor d needs to be a multiple of anything.
 */
#ifndef IMGREC_VLAD_H
#define IMGREC_VLAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum vlad_flags {
    VLAD_RAW = 1           /* vlad receives the raw accumulator V: no normalisation, no square root */
};

#define VLAD_MAX_NN 8
#define VLAD_MAX_D 16384

/* The encoding over device-resident data on `stream`; nothing waits on the host.
 *   x         N x d float32      the descriptors of all images, concatenated
 *   offsets   int64[nimg + 1]    device pointer; non-decreasing, offsets[0] = 0, offsets[nimg] = N
 *                                (not checked here: the values are clamped to [0, N], so a bad
 *                                array gives wrong vectors, never an access outside x)
 *   codebook  k x d float32
 *   vlad      nimg x (k * d) float32
 *   nn_idx    int32[N x nn]      the neighbours, best first (may be NULL)
 *   nn_dist   float32[N x nn]    their distances (may be NULL)
 * N = 0 and nimg = 0 are allowed.  IMGREC_VLAD_LDS_FLOATS=<floats> (tests), read when the call
 * starts, overrides the accumulator size that decides the cluster tiling (the default fits
 * 256 x 128); the outputs do not depend on it. */
int vlad_encode_device(const float* x, int64_t N, const int64_t* offsets, int64_t nimg, int d,
                       const float* codebook, int k, int nn, float sigma, int flags, float* vlad,
                       int32_t* nn_idx, float* nn_dist, void* stream);

/* The same over host arrays on HIP device `device` (-1 = current): checks offsets (KNN_EINVAL
 * unless they start at 0, never decrease and end at N), uploads, calls vlad_encode_device on a
 * stream of its own, downloads and waits. */
int vlad_encode(const float* x, int64_t N, const int64_t* offsets, int64_t nimg, int d,
                const float* codebook, int k, int nn, float sigma, int flags, float* vlad,
                int32_t* nn_idx, float* nn_dist, int device);

#ifdef __cplusplus
}
#endif

#endif /* IMGREC_VLAD_H */
