// vladenc_args.h — the host-side rules of include/imgrec_vladenc.h: the argument checks, the depth
// split of a layer and the row chunking.  Plain C++17 with no HIP include, so that the host check
// (tests/fuzz/vladenc_args_check.cpp) compiles the same code under sanitizers.  A check returns 0,
// or -1 (KNN_EINVAL) with a message in `msg`.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/imgrec_vladenc.h"
#include "rows_geom.h"

namespace imgrec {

// a workgroup takes kBN features (a row tile) and streams stages of kBK depth columns (rows_geom.h)
constexpr int kEncTargetWgs = 512;     // feature tiles x splits aimed at: two workgroups per CU
constexpr int kEncMinStages = 4;       // a split is at least this deep (but for a short layer)
// the most partial sums a launch leaves, whatever the layer (vladenc_split: tiles x splits <= 512)
constexpr int64_t kEncMaxPartFloats = (int64_t)VLADENC_CHUNK_ROWS * kEncTargetWgs * kBN;

inline int vladenc_check_create(int nlayers, const int* widths, const float* const* W, const float* const* b,
                                const float* const* gamma, const float* const* beta, float ln_eps,
                                const void* out, const char* who, char* msg, size_t cap) {
    if (nlayers < 1 || nlayers > VLADENC_MAX_LAYERS)
        ARGS_BAD("%s: nlayers must be in [1, %d] (got %d)", who, VLADENC_MAX_LAYERS, nlayers);
    if (!widths || !W || !b || !out || (nlayers > 1 && (!gamma || !beta)))
        ARGS_BAD("%s: NULL widths, W, b, gamma, beta or handle pointer", who);
    for (int l = 0; l <= nlayers; ++l) {
        const int lim = l == 0 ? VLADENC_MAX_IN : VLADENC_MAX_WIDTH;
        if (widths[l] < 1 || widths[l] > lim)
            ARGS_BAD("%s: widths[%d] must be in [1, %d] (got %d)", who, l, lim, widths[l]);
    }
    for (int l = 0; l < nlayers; ++l) {
        if (!W[l] || !b[l]) ARGS_BAD("%s: NULL weight or bias of layer %d", who, l);
        if (l < nlayers - 1 && (!gamma[l] || !beta[l])) ARGS_BAD("%s: NULL LayerNorm weight or bias of layer %d", who, l);
    }
    if (!(ln_eps >= 0.f) || !(ln_eps <= 1e18f)) ARGS_BAD("%s: ln_eps must be finite and >= 0 (got %g)", who, (double)ln_eps);
    return 0;
}

inline int vladenc_check_forward(const void* h, const void* x, int64_t n, int flags, const void* out,
                                 const char* who, char* msg, size_t cap) {
    if (!h) ARGS_BAD("%s: NULL handle", who);
    if (flags & ~VLADENC_MODEL_OUTPUT) ARGS_BAD("%s: unknown flags 0x%x", who, flags);
    if (n < 0 || n >= (int64_t(1) << 31)) ARGS_BAD("%s: n = %lld rows (limit 2^31 - 1)", who, (long long)n);
    if (n > 0 && (!x || !out)) ARGS_BAD("%s: NULL x or out", who);
    return 0;
}

// How a layer of depth K and N features is cut (imgrec_vladenc.h "linear"): a function of (K, N) only.
struct EncSplit {
    int tiles;     // feature tiles of kBN
    int stages;    // stages of kBK columns
    int per;       // stages per split
    int nsplit;    // splits: split s = stages [s * per, min((s + 1) * per, stages))
};

inline EncSplit vladenc_split(int K, int N) {
    EncSplit s;
    s.tiles = (N + kBN - 1) / kBN;
    s.stages = (K + kBK - 1) / kBK;
    const int want = kEncTargetWgs / s.tiles > 1 ? kEncTargetWgs / s.tiles : 1;
    const int cap = s.stages / kEncMinStages > 1 ? s.stages / kEncMinStages : 1;
    const int s0 = want < cap ? want : cap;
    s.per = (s.stages + s0 - 1) / s0;
    s.nsplit = (s.stages + s.per - 1) / s.per;
    return s;
}

// partial sums of `rows` rows of a layer, in floats
inline int64_t vladenc_part_floats(int K, int N, int64_t rows) { return (int64_t)vladenc_split(K, N).nsplit * N * rows; }

// The knob IMGREC_VLADENC_CHUNK_ROWS (0 = unset) counts where it is in [1, VLADENC_CHUNK_ROWS].
inline bool vladenc_knob_set(long long knob) { return knob >= 1 && knob <= VLADENC_CHUNK_ROWS; }

// Rows per chunk, the rows whose hidden activations the workspace holds at a time: the knob, else
// VLADENC_SUPER_ROWS; never a function of n.
inline int vladenc_chunk_rows(long long knob) { return vladenc_knob_set(knob) ? (int)knob : VLADENC_SUPER_ROWS; }

// Rows of a chunk that layer (K, N) takes per launch: as many row tiles of VLADENC_CHUNK_ROWS as
// keep its partial sums within kEncMaxPartFloats (at least one tile), at most the chunk.
inline int vladenc_layer_rows(int K, int N, int chunk) {
    int64_t rows = kEncMaxPartFloats / ((int64_t)vladenc_split(K, N).nsplit * N) / VLADENC_CHUNK_ROWS * VLADENC_CHUNK_ROWS;
    if (rows < VLADENC_CHUNK_ROWS) rows = VLADENC_CHUNK_ROWS;
    return (int)(rows < chunk ? rows : chunk);
}

}  // namespace imgrec
