/*
 * imgrec_kmeans.h — C ABI of Lloyd k-means on the MI355X (faiss.Kmeans / faiss Clustering::train).
 *
 * The reference trains its SIFT visual vocabulary with
 *   faiss.Kmeans(128, 256, niter=25, verbose=True, gpu=True).train(x); kmeans.centroids
 * (vector_scripts/create_sift_vector.py:221-227).  faiss_compat.Kmeans serves that call from the
 * entry points below (csrc/knn_kmeans.hip).
 *
 * Conventions: those of imgrec_knn.h.  Every function returns 0 or a negative KNN_E* code
 * (imgrec_knn.h enum knn_error) and leaves its message in knn_last_error(); streams are hipStream_t
 * passed as void* (NULL = the null stream); every argument is checked on the host before any GPU
 * call, so a bad argument is KNN_EINVAL on a machine without a GPU.  Arrays are row-major float32.
 *
 * Determinism: every output of kmeans_step_device is a pure function of its inputs and of the
 * update's part size (IMGREC_KMEANS_PART, below): no float atomics, no order that depends on the
 * grid or on scheduling.  Two calls on the same inputs give the same bytes.
 */
#ifndef IMGREC_KMEANS_H
#define IMGREC_KMEANS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum kmeans_flags {
    KMEANS_SPHERICAL = 1   /* assign by the largest inner product; dist holds that product */
};

/* One Lloyd step over device-resident data on `stream`; nothing waits on the host.
 *   x             n x d        the points
 *   centroids     k x d        the current centroids
 *   assign        int32[n]     the nearest centroid: the smallest fp32 key |c|^2 - 2 x.c (x.c on the
 *                              exact-fp32 MFMA, one summation order for every pair), an exact tie to
 *                              the smaller centroid id.  KMEANS_SPHERICAL: the key is -x.c.
 *   dist          float32[n]   |x - c|^2 to that centroid, summed directly in fp32 (not the key);
 *                              KMEANS_SPHERICAL: x.c
 *   new_centroids k x d        the mean of every cluster's members (members added in ascending point
 *                              index inside parts of a fixed number of members, part sums added in
 *                              part order); an empty cluster's row is the old row, byte for byte.
 *                              Must not alias `centroids`.
 *   counts        int64[k]     members per cluster
 *   obj           float64[1]   the sum of dist, in float64 in a fixed order
 * 1 <= k <= n < 2^31, d >= 1; neither n, k nor d needs to be a multiple of anything.
 * IMGREC_KMEANS_PART=<members> (tests), read when the call starts, overrides the part size (256). */
int kmeans_step_device(const float* x, int64_t n, int d, const float* centroids, int k, int flags,
                       int32_t* assign, float* dist, float* new_centroids, int64_t* counts,
                       double* obj, void* stream);

/* faiss's empty-cluster repair (Clustering.cpp split_clusters) on k x d device centroids.
 * counts_host (int64[k], host, read and updated) are the cluster sizes.  For every empty cluster
 * ci, in ascending order, a donor cj with more than one member is drawn with probability
 * proportional to its size - 1 (std::mt19937 seeded 1234 at every call, faiss's loop); row ci
 * becomes row cj with even columns times 1 + 1/1024 and odd columns times 1 - 1/1024, row cj gets
 * the opposite, and ci takes half of cj's count.  The donor choice is made on the host; the rows are
 * rewritten by one kernel on `stream` (the pair list is uploaded first).  *nsplit (may be NULL)
 * receives the number of clusters repaired.  KNN_EINVAL when a cluster is empty and no cluster has
 * more than one member. */
int kmeans_split_device(float* centroids, int k, int d, int64_t* counts_host, int* nsplit,
                        void* stream);

typedef struct kmeans_params {
    int niter;        /* Lloyd iterations per run (faiss: 25) */
    int nredo;        /* runs; the one with the best final objective is kept (faiss: 1) */
    int spherical;    /* inner-product assignment, centroids L2-normalised after every update */
    int verbose;      /* one line per iteration on stderr */
    int64_t seed;     /* initialisation: run r samples k distinct rows with std::mt19937_64(seed + r) */
    int device;       /* kmeans_train only: the HIP device (-1 = current) */
} kmeans_params_t;

/* Doubles per iteration in stats_out: the objective of the iteration's assignment (before the
 * update, faiss's convention), seconds since the run started, seconds of that in the step, the
 * imbalance factor k sum(cnt^2) / (sum cnt)^2, the clusters split, and the step's GPU milliseconds
 * in the assignment, the sort and the segmented sums. */
#define KMEANS_STATS_PER_ITER 8

/* faiss Clustering::train over n host rows (kmeans_train: uploaded once) or n device rows on
 * `stream`.  Per run: initial centroids (init_centroids, k x d on the host, when given; else a
 * seeded sample of k distinct rows), then niter times: kmeans_step_device, the counts and the
 * objective read back (k + 1 numbers), kmeans_split_device, and with `spherical` a row
 * normalisation.  centroids_out (k x d, host), *obj_out (the last iteration's objective) and
 * stats_out (niter * KMEANS_STATS_PER_ITER doubles, may be NULL) are those of the best run: the
 * smallest final objective, the largest with `spherical`.  Both wait for the GPU. */
int kmeans_train(const float* x_host, int64_t n, int d, int k, const kmeans_params_t* params,
                 const float* init_centroids, float* centroids_out, double* obj_out,
                 double* stats_out);
int kmeans_train_device(const float* x_dev, int64_t n, int d, int k, const kmeans_params_t* params,
                        const float* init_centroids, float* centroids_out, double* obj_out,
                        double* stats_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* IMGREC_KMEANS_H */
