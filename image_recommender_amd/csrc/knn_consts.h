// knn_consts.h — the plain tile and padding constants that both the kernels (knn_kernels.h) and the
// host-side launch plan (knn_plan.h) read.  No HIP header: the plan unit builds without ROCm.
#pragma once

#include <stdint.h>

namespace imgrec {

constexpr int kTileRowsMax = 256;   // corpus capacity is rounded to this many rows
constexpr int kDepthPad = 16;       // row stride is rounded to this many floats

// Split-path tile: (1,4) workgroups of kSplitWB-block waves, kSplitBK-word stages, kSplitNS ring.
#ifndef IMGREC_SPLIT_BK
#define IMGREC_SPLIT_BK 32
#endif
#ifndef IMGREC_SPLIT_NS
#define IMGREC_SPLIT_NS 2
#endif
#ifndef IMGREC_SPLIT_WB
#define IMGREC_SPLIT_WB 4
#endif
constexpr int kSplitBK = IMGREC_SPLIT_BK, kSplitNS = IMGREC_SPLIT_NS, kSplitWB = IMGREC_SPLIT_WB;

// bf16 candidate-pass tile: (kB16WR, kB16WQ) workgroups of kB16WB-block waves, 64-deep stages
// (32 words), kB16NS ring, kB16WGPCU workgroups per CU; rows of the bf16 copy padded to
// kB16Pad elements.
#ifndef IMGREC_B16_WR
#define IMGREC_B16_WR 1
#endif
#ifndef IMGREC_B16_WQ
#define IMGREC_B16_WQ 4
#endif
#ifndef IMGREC_B16_WB
#define IMGREC_B16_WB 4
#endif
#ifndef IMGREC_B16_NS
#define IMGREC_B16_NS 2
#endif
#ifndef IMGREC_B16_WGPCU
#define IMGREC_B16_WGPCU 2
#endif
constexpr int kB16WR = IMGREC_B16_WR, kB16WQ = IMGREC_B16_WQ, kB16WB = IMGREC_B16_WB;
constexpr int kB16NS = IMGREC_B16_NS, kB16WGPCU = IMGREC_B16_WGPCU, kB16Pad = 64;

// 256 x 256-tile bf16 kernel (knn_b16w.hip): one 8-wave workgroup per CU, k <= 10, batches of at
// least kB16BigMinQ queries.
#ifndef IMGREC_B16_BIG_MINQ
#define IMGREC_B16_BIG_MINQ 512
#endif
// packed candidate lists while a split's row index fits this many bits: the
// approximate keys keep 23 - ib mantissa bits (relative truncation <= 2^(ib - 23))
#ifndef IMGREC_B16_PACK_MAXIB
#define IMGREC_B16_PACK_MAXIB 14
#endif
constexpr int kB16PackMaxIB = IMGREC_B16_PACK_MAXIB;
constexpr int kB16BigRows = 256, kB16BigQueries = 256, kB16BigMinQ = IMGREC_B16_BIG_MINQ;

// Bytes per row of the int8 copy: 64 per block, no padding (round 4; rows were whole 1-KiB
// groups of 16 blocks, 25 % zeros at d = 768).  Blocks sit in groups of 16 (the scan's 16 lanes of
// a row): group g = b / 16 holds m = min(16, nblk - 16 g) blocks at byte 1024 g, chunk c (16 B)
// of its block j = b % 16 at 16-B slot m c + j, so lane j's load c of a row reads 16 m contiguous
// bytes with its group's other lanes (256 B for a full group).  (constexpr: host and kernels alike)
constexpr int64_t i8_row_bytes(int nblk) { return (int64_t)64 * nblk; }

}  // namespace imgrec
