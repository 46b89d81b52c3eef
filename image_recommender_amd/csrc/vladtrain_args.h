// vladtrain_args.h — the host-side rules of include/imgrec_vladtrain.h: the argument checks, the
// split rule of the backward products, the parameter layout and the workspace bound.  Plain C++17
// with no HIP include, so that the host check (tests/fuzz/vladtrain_args_check.cpp) compiles the
// same code under sanitizers.  A check returns 0, or -1 (KNN_EINVAL) with a message in `msg`.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/imgrec_vladtrain.h"
#include "vladenc_args.h"

namespace imgrec {

inline int vladtrain_check_config(const vladtrain_config* c, const char* who, char* msg, size_t cap) {
    if (!c) ARGS_BAD("%s: NULL config", who);
    if (!(c->dropout >= 0.) || !(c->dropout < 1.)) ARGS_BAD("%s: dropout must be in [0, 1) (got %g)", who, c->dropout);
    if (!(c->lr >= 0.) || !(c->lr <= 1e18)) ARGS_BAD("%s: lr must be finite and >= 0 (got %g)", who, c->lr);
    if (!(c->beta1 >= 0.) || !(c->beta1 < 1.) || !(c->beta2 >= 0.) || !(c->beta2 < 1.))
        ARGS_BAD("%s: betas must be in [0, 1) (got %g, %g)", who, c->beta1, c->beta2);
    if (!(c->adam_eps > 0.) || !(c->adam_eps <= 1e18)) ARGS_BAD("%s: adam_eps must be finite and > 0 (got %g)", who, c->adam_eps);
    if (!(c->weight_decay >= 0.) || !(c->weight_decay <= 1e18))
        ARGS_BAD("%s: weight_decay must be finite and >= 0 (got %g)", who, c->weight_decay);
    if (!(std::fabs(c->corr_weight) <= 1e18) || !(std::fabs(c->umap_weight) <= 1e18))
        ARGS_BAD("%s: the loss weights must be finite (got %g, %g)", who, c->corr_weight, c->umap_weight);
    if (!(c->temperature > 0.) || !(c->temperature <= 1e18))
        ARGS_BAD("%s: temperature must be finite and > 0 (got %g)", who, c->temperature);
    if (!(c->ln_eps >= 0.) || !(c->ln_eps <= 1e18)) ARGS_BAD("%s: ln_eps must be finite and >= 0 (got %g)", who, c->ln_eps);
    return 0;
}

inline int vladtrain_check_create(int nlayers, const int* widths, const float* const* W, const float* const* b,
                                  const float* const* gamma, const float* const* beta, const vladtrain_config* cfg,
                                  const void* out, const char* who, char* msg, size_t cap) {
    if (vladtrain_check_config(cfg, who, msg, cap) != 0) return -1;
    return vladenc_check_create(nlayers, widths, W, b, gamma, beta, (float)cfg->ln_eps, out, who, msg, cap);
}

// What a step, a grads or an eval call can check without reading the handle.
inline int vladtrain_check_call(const void* h, const void* x, int64_t n, const int32_t* sample_idx, int64_t k,
                                const void* losses, const char* who, char* msg, size_t cap) {
    if (!h) ARGS_BAD("%s: NULL handle", who);
    if (n < 2 || n > VLADTRAIN_MAX_BATCH) ARGS_BAD("%s: n must be in [2, %d] rows (got %lld)", who, VLADTRAIN_MAX_BATCH, (long long)n);
    if (!x || !losses) ARGS_BAD("%s: NULL x or losses", who);
    if (sample_idx && (k < 2 || k > n)) ARGS_BAD("%s: k must be in [2, n = %lld] (got %lld)", who, (long long)n, (long long)k);
    return 0;
}

// What needs the handle's widths[0] = in_width, after vladtrain_check_call has passed: the batch's
// size and the sample.  `seen` is scratch of n bytes for the distinctness check; on success
// seen[i] = 1 exactly for the sampled rows (all n without sample_idx) and *kout is their count.
inline int vladtrain_check_sample(int in_width, int64_t n, const int32_t* sample_idx, int64_t k, unsigned char* seen,
                                  int* kout, const char* who, char* msg, size_t cap) {
    if (n * (int64_t)in_width > (int64_t)VLADTRAIN_MAX_BATCH_FLOATS)
        ARGS_BAD("%s: n x width = %lld x %d floats exceeds %d", who, (long long)n, in_width, VLADTRAIN_MAX_BATCH_FLOATS);
    if (!sample_idx) {
        for (int64_t i = 0; i < n; ++i) seen[i] = 1;
        *kout = (int)n;
        return 0;
    }
    for (int64_t i = 0; i < n; ++i) seen[i] = 0;
    for (int64_t q = 0; q < k; ++q) {
        const int32_t i = sample_idx[q];
        if (i < 0 || i >= n) ARGS_BAD("%s: sample_idx[%lld] = %d is not a row of the batch", who, (long long)q, (int)i);
        if (seen[i]) ARGS_BAD("%s: sample_idx[%lld] = %d appears twice", who, (long long)q, (int)i);
        seen[i] = 1;
    }
    *kout = (int)k;
    return 0;
}

inline int vladtrain_check_product(const void* A, int64_t I, const void* B, int64_t J, int64_t K, const void* C,
                                   const char* who, char* msg, size_t cap) {
    if (!A || !B || !C) ARGS_BAD("%s: NULL A, B or C", who);
    if (I < 1 || I > VLADENC_MAX_WIDTH) ARGS_BAD("%s: I must be in [1, %d] (got %lld)", who, VLADENC_MAX_WIDTH, (long long)I);
    if (J < 1 || J > VLADENC_MAX_IN) ARGS_BAD("%s: J must be in [1, %d] (got %lld)", who, VLADENC_MAX_IN, (long long)J);
    if (K < 1 || K > VLADENC_MAX_IN) ARGS_BAD("%s: K must be in [1, %d] (got %lld)", who, VLADENC_MAX_IN, (long long)K);
    return 0;
}

inline int vladtrain_check_which(int which, bool set, const char* who, char* msg, size_t cap) {
    if (which < VLADTRAIN_PARAMS || which > VLADTRAIN_GRADS) ARGS_BAD("%s: unknown state %d", who, which);
    if (set && which == VLADTRAIN_GRADS) ARGS_BAD("%s: the gradients cannot be set", who);
    return 0;
}

// How a product of I x J outputs and depth K is cut (imgrec_vladtrain.h "products"): tiles of
// kBN x kBM outputs, splits of whole stages, about kEncTargetWgs workgroups.
struct ProdSplit {
    int ti, tj;    // output tiles along I (kBN each) and J (kBM each)
    EncSplit sp;   // .tiles = ti; stages, per, nsplit as vladenc_split's
};

inline ProdSplit vladtrain_split(int I, int J, int K) {
    ProdSplit p;
    p.ti = (I + kBN - 1) / kBN;
    p.tj = (J + kBM - 1) / kBM;
    p.sp.tiles = p.ti;
    p.sp.stages = (K + kBK - 1) / kBK;
    const int64_t T = (int64_t)p.ti * p.tj;
    const int want = kEncTargetWgs / T > 1 ? (int)(kEncTargetWgs / T) : 1;
    const int cap = p.sp.stages / kEncMinStages > 1 ? p.sp.stages / kEncMinStages : 1;
    const int s0 = want < cap ? want : cap;
    p.sp.per = (p.sp.stages + s0 - 1) / s0;
    p.sp.nsplit = (p.sp.stages + p.sp.per - 1) / p.sp.per;
    return p;
}

// partial sums of a split product, in floats (0 when it is not split: it writes its output itself)
inline int64_t vladtrain_part_floats(int I, int J, int K) {
    const ProdSplit p = vladtrain_split(I, J, K);
    return p.sp.nsplit > 1 ? (int64_t)p.sp.nsplit * I * J : 0;
}

// The flat parameter layout: per layer W, b, then gamma, beta (hidden layers), each at a multiple of
// 4 floats.  off[4 l + {0, 1, 2, 3}]; returns the total.
inline int64_t vladtrain_layout(int nlayers, const int* widths, int64_t* off) {
    int64_t at = 0;
    auto put = [&](int slot, int64_t count) {
        if (off) off[slot] = at;
        at += (count + 3) / 4 * 4;
    };
    for (int l = 0; l < nlayers; ++l) {
        const int64_t K = widths[l], N = widths[l + 1];
        put(4 * l, N * K);
        put(4 * l + 1, N);
        put(4 * l + 2, l < nlayers - 1 ? N : 0);
        put(4 * l + 3, l < nlayers - 1 ? N : 0);
    }
    return at;
}

// what a call of n rows reserves, buffer by buffer (floats but for the named doubles)
struct TrainSizes {
    int64_t part;      // split partial sums: the forward's and the backward products'
    int64_t xt;        // the transposed batch
    int64_t gram;      // G, then D_x
    int64_t keep;      // y of every layer and every post-dropout activation
    int64_t wide;      // one n x (widest of widths[1..]) gradient buffer (three of them)
    int64_t wt;        // the largest transposed weight matrix of a layer l >= 1
    int64_t doubles;   // row statistics: per layer mean and sd, the loss rows' eight sums, coefficients
};

inline TrainSizes vladtrain_sizes(int nlayers, const int* widths, int64_t n) {
    TrainSizes s = {};
    int64_t wmax = 1, hsum = 0;
    auto part = [&](int64_t v) { if (v > s.part) s.part = v; };
    part(vladtrain_part_floats((int)n, (int)n, widths[0]));
    for (int l = 0; l < nlayers; ++l) {
        const int K = widths[l], N = widths[l + 1];
        part(vladenc_part_floats(K, N, vladenc_layer_rows(K, N, (int)n)));
        part(vladtrain_part_floats(N, K, (int)n));                 // dW
        if (l > 0) {
            part(vladtrain_part_floats((int)n, K, N));             // dA
            if ((int64_t)K * N > s.wt) s.wt = (int64_t)K * N;
            hsum += K;
        }
        if (N > wmax) wmax = N;
    }
    s.xt = n * widths[0];
    s.gram = n * n;
    s.keep = n * (2 * hsum + widths[nlayers] + 1);      // + G's diagonal
    s.wide = n * wmax;
    s.doubles = n * (2 * nlayers + 8) + 16;
    return s;
}

inline int64_t vladtrain_workspace_total(int nlayers, const int* widths, int64_t n) {
    const TrainSizes s = vladtrain_sizes(nlayers, widths, n);
    return 4 * (s.part + s.xt + s.gram + s.keep + 3 * s.wide + s.wt + widths[nlayers] * n) + 8 * s.doubles;
}

}  // namespace imgrec
