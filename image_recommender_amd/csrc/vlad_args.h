// vlad_args.h — the host-side argument checks of include/imgrec_vlad.h.  Plain C++17 with no HIP
// include, so that the host check (tests/fuzz/vlad_args_check.cpp) compiles the same code under
// sanitizers.  Each function returns 0, or -1 (KNN_EINVAL) with a message in `msg`.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/imgrec_vlad.h"
#include "rows_geom.h"

namespace imgrec {

struct VladArgs {
    const void* x;
    int64_t N;
    const void* offsets;
    int64_t nimg;
    int d;
    const void* codebook;
    int k;
    int nn;
    float sigma;
    int flags;
    const void* vlad;
};

// the default accumulator, in floats: 256 rows of 128 sums (128 KiB)
constexpr int64_t kVladAccFloats = 256 * 128;

inline int vlad_check_args(const VladArgs& a, const char* who, char* msg, size_t cap) {
    if (a.d <= 0 || a.d > VLAD_MAX_D) ARGS_BAD("%s: d must be in [1, %d] (got %d)", who, VLAD_MAX_D, a.d);
    if (a.k <= 0) ARGS_BAD("%s: k must be positive (got %d)", who, a.k);
    if (a.nn < 1 || a.nn > VLAD_MAX_NN) ARGS_BAD("%s: nn must be in [1, %d] (got %d)", who, VLAD_MAX_NN, a.nn);
    if (a.nn > a.k) ARGS_BAD("%s: nn = %d exceeds the codebook's k = %d rows", who, a.nn, a.k);
    if (!(a.sigma > 0.f) || !(a.sigma <= 1e18f)) ARGS_BAD("%s: sigma must be positive and finite (got %g)", who, (double)a.sigma);
    if (a.flags & ~VLAD_RAW) ARGS_BAD("%s: unknown flags 0x%x", who, a.flags);
    if (a.N < 0 || a.N >= (int64_t(1) << 31)) ARGS_BAD("%s: N = %lld descriptors (limit 2^31 - 1)", who, (long long)a.N);
    if (a.nimg < 0 || a.nimg >= (int64_t(1) << 31)) ARGS_BAD("%s: nimg = %lld images (limit 2^31 - 1)", who, (long long)a.nimg);
    if (!a.offsets || !a.codebook || (!a.x && a.N > 0) || (!a.vlad && a.nimg > 0))
        ARGS_BAD("%s: NULL descriptors, offsets, codebook or vlad", who);
    if (!row_stages_fit(a.k, a.d)) ARGS_BAD("%s: k x d too large (%d x %d)", who, a.k, a.d);
    return 0;
}

// host offsets: start at 0, never decrease, end at N
inline int vlad_check_offsets(const int64_t* off, int64_t nimg, int64_t N, const char* who, char* msg, size_t cap) {
    if (off[0] != 0) ARGS_BAD("%s: offsets[0] = %lld, must be 0", who, (long long)off[0]);
    for (int64_t i = 0; i < nimg; ++i)
        if (off[i + 1] < off[i])
            ARGS_BAD("%s: offsets decrease at image %lld (%lld after %lld)", who, (long long)i,
                     (long long)off[i + 1], (long long)off[i]);
    if (off[nimg] != N) ARGS_BAD("%s: offsets[nimg] = %lld, must be N = %lld", who, (long long)off[nimg], (long long)N);
    return 0;
}

// Codebook rows per aggregation workgroup: as many rows of d sums as fit `acc_floats` (at least
// one, at most k).  *ntiles = the workgroups per image; -1 when nimg * ntiles does not fit a grid.
inline int vlad_cluster_tile(int k, int d, int64_t acc_floats, int64_t nimg, int* ct, int64_t* ntiles,
                             const char* who, char* msg, size_t cap) {
    int64_t rows = acc_floats / d;
    if (rows < 1) rows = 1;
    if (rows > k) rows = k;
    *ct = (int)rows;
    *ntiles = ((int64_t)k + rows - 1) / rows;
    if (nimg * *ntiles >= (int64_t(1) << 31))
        ARGS_BAD("%s: %lld images x %lld cluster tiles exceed a grid (limit 2^31 - 1)", who, (long long)nimg,
                 (long long)*ntiles);
    return 0;
}

}  // namespace imgrec
