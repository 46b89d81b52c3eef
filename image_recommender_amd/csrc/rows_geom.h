// rows_geom.h — the numbers of the fp32 row tile (rows_tile.h) that host rules count with: the split
// rule of vladenc_args.h, the stage limit of the k-means and VLAD argument checks.  Plain C++17 with
// no HIP include, so that the host checks (tests/fuzz/*_args_check.cpp) compile the same numbers
// under sanitizers; rows_tile.h builds the device side on them.
#pragma once

#include <cstdint>
#include <cstdio>

namespace imgrec {

constexpr int kBM = 128;                // points per workgroup
constexpr int kBN = 256;                // rows per tile
constexpr int kBK = 32;                 // depth per stage: a row's 128-byte line
constexpr int kLDK = kBK + 4;           // LDS row stride (floats)
constexpr int kNT = 512;                // threads: eight waves
constexpr int kQ = kBK / 4;             // float4 per row and stage

// k rows of depth d are tiles x stages-per-tile stages, which the stream counts in an int
inline bool row_stages_fit(int k, int d) {
    return ((int64_t)k + kBN - 1) / kBN * (((int64_t)d + kBK - 1) / kBK) < (int64_t(1) << 31);
}

// an argument check's failure: the message into `msg` (of `cap` bytes), then -1
#define ARGS_BAD(...)                         \
    do {                                      \
        std::snprintf(msg, cap, __VA_ARGS__); \
        return -1;                            \
    } while (0)

}  // namespace imgrec
