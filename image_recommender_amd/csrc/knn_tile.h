// knn_tile.h — the tile core shared by the kernels that send every (row, query) pair through the
// exact contraction: knn_tile_topk (knn_kernels.hip), knn_range_tile (knn_range.hip) and
// knn_filter_tile (knn_filter.hip).  One definition of the tile geometry, the per-lane layout, the
// stage consumer (counted wait, fragment reads, MFMA chain) and the epilogue's key forming, so the
// depth order and the key formula — what makes the three kernels' results bitwise equal — cannot
// drift apart.  Each kernel keeps its DMA producer (contiguous or list-gathered rows) and what it
// does with the surviving keys.  Included by .hip translation units only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"
#include "lds_dma.h"

namespace imgrec {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 16-B fragment chunk c of a per-lane float array, reinterpreted as 8 bf16 (split layout)
template <int N>
__device__ __forceinline__ bf16x8 frag_bf16(const float (&v)[N], int c) {
    const f32x4 f = {v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]};
    return __builtin_bit_cast(bf16x8, f);
}

// ---------------------------------------------------------------------------------------------
// Tile geometry
//
// Workgroup = WR x WQ waves; wave tile = 32*WB corpus rows (WB MFMA row blocks, 4 or 8) x 32
// queries, so the workgroup tile is BM = 32*WB*WR rows x BQ = 32*WQ queries.  A workgroup owns one
// query block and a range of row tiles (a "row split") and streams it as one continuous sequence of
// BK-deep K stages: (tile t0, stage 0..nsteps-1), (t0+1, 0..), ...
//
// Staging is LDS-DMA (global_load_lds_dwordx4): each wave instruction moves one 1-KiB piece
// (RPP rows x 4*BK bytes) straight into LDS, no staging VGPRs, into an NS-deep ring; a stage is
// read NS-1 iterations after its loads were issued, behind a counted `s_waitcnt vmcnt` and one raw
// s_barrier per stage (cdna_hip_programming.md §5 "Pipelining across barriers").  The ring runs
// across tile boundaries, so a tile's epilogue overlaps the next tile's loads.
//
// LDS image: rows of BK floats; 16-B chunk c of row r stored at chunk c ^ ((r / RPB) % CPR)
// (RPB = rows per 256-B bank row, CPR = chunks per row).  The XOR is applied to the per-lane
// GLOBAL source address (the DMA destination is lane-linear); the fragment reads apply the same
// XOR, which makes every ds_read_b128 16-lane group hit 16 distinct 16-B bank slots.
// ---------------------------------------------------------------------------------------------
template <int WR_, int WQ_, int NS_, int BK_, int WB_ = 4>
struct TileGeom {
    static constexpr int WR = WR_, WQ = WQ_, NS = NS_, BK = BK_, WB = WB_;
    static constexpr int NW = WR * WQ, NT = NW * 64;
    static constexpr int RW = 32 * WB;                 // corpus rows per wave
    static constexpr int BM = WR * RW, BQ = WQ * 32;
    static constexpr int CPR = BK / 4;                 // 16-B chunks per staged row
    static constexpr int RPP = 64 / CPR;               // rows per 1-KiB DMA piece
    static constexpr int RPB = 64 / BK;                // rows per 256-B bank row
    static constexpr int SA = BM * BK, SB = BQ * BK, STAGE = SA + SB;   // floats
    static constexpr int PA = BM / RPP, PB = BQ / RPP, PIECES = PA + PB;
    static constexpr int LPW = PIECES / NW;            // pieces per wave per stage
    // epilogue key parking in a spent stage: all 16 keys of a block in one round when they fit
    static constexpr int PR = (SA + SB) >= NW * 16 * 64 ? 16 : 8;
    static constexpr int PARK = NW * PR * 64;
    // the ring: NS stages and the NS tiles' row norms
    static constexpr int LDS_FLOATS = NS * STAGE + NS * BM;
    // __launch_bounds__' second argument: 4-wave workgroups run two per CU (two waves per SIMD),
    // which holds them to 256 VGPR+AGPR per lane
    static constexpr int MIN_WAVES = NW == 4 ? 2 : 1;
    static_assert(BK == 16 || BK == 32, "stage depth");
    static_assert(PIECES % NW == 0, "pieces must divide evenly over waves");
    static_assert(BM % 64 == 0, "norm DMA uses whole waves");
    static_assert(STAGE >= PARK, "epilogue parking must fit in one stage");
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
};

// Insert into an ascending list when labels reach this lane in increasing order (true inside
// the tile kernels: a lane visits its rows in increasing row order), so "ranks before" is a plain
// key comparison and an equal key always lands behind the existing entries.
template <int K>
__device__ __forceinline__ void list_insert_mono(float (&kd)[K], int (&ki)[K], float d, int id) {
    // c[p]: d goes before slot p of the old list (monotone); one compare, four selects per slot
    bool c[K];
#pragma unroll
    for (int p = 0; p < K; ++p) c[p] = d < kd[p];
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
        // the same select on an ascending list is the median of (kd[p-1], d, kd[p]): one v_med3
        kd[p] = __builtin_amdgcn_fmed3f(kd[p - 1], d, kd[p]);
        ki[p] = c[p - 1] ? ki[p - 1] : (c[p] ? id : ki[p]);
    }
    kd[0] = c[0] ? d : kd[0];
    ki[0] = c[0] ? id : ki[0];
}

// The per-lane layout of a wave (uniform index `wave`) in a G tile.
template <class G>
struct TileLanes {
    int wave;
    int wr, wq;                 // the wave's place in the WR x WQ grid
    int li, lh;                 // accumulator column (query) and row half of this lane
    // per-lane fragment offsets inside a 32-row block: logical chunks lh*CPR/2 + c of row li
    int fo[G::CPR / 2];
    // This lane's 16 B of a 1-KiB DMA piece: row `pr` of the piece's RPP rows, at float offset
    // gsw[0] (even pieces) or gsw[1] (odd pieces) plus the stage's depth inside that row.  The
    // swizzle depends on the piece index modulo 2 — on the piece's place in the tile, not on the
    // row it holds — so a producer is free to gather any row there.
    int pr, gsw[2];

    __device__ __forceinline__ TileLanes(int lane, int wave_) : wave(wave_) {
        constexpr int CPR = G::CPR, RPP = G::RPP, RPB = G::RPB;
        wr = wave / G::WQ;
        wq = wave % G::WQ;
        li = lane & 31;
        lh = lane >> 5;
        const int fsw = (li / RPB) % CPR;
#pragma unroll
        for (int c = 0; c < CPR / 2; ++c) fo[c] = li * G::BK + 4 * ((lh * (CPR / 2) + c) ^ fsw);
        pr = lane / CPR;
        const int pchk = lane % CPR;
        gsw[0] = 4 * (pchk ^ (((0 * RPP + pr) / RPB) % CPR));
        gsw[1] = 4 * (pchk ^ (((1 * RPP + pr) / RPB) % CPR));
    }
    // Piece j (< LPW) of this wave is piece wave*LPW + j of a stage: an A piece (RPP rows of the
    // tile) or a B piece (RPP queries), wave-uniform.
    __device__ __forceinline__ bool is_a(int j) const { return wave * G::LPW + j < G::PA; }
    // its first row in the tile (or in the query block)
    __device__ __forceinline__ int prow0(int j) const {
        return (is_a(j) ? wave * G::LPW + j : wave * G::LPW + j - G::PA) * G::RPP;
    }
    // the row this lane sources and its swizzled float offset inside that row
    __device__ __forceinline__ int prow(int j) const { return prow0(j) + pr; }
    __device__ __forceinline__ int psw(int j) const { return ((prow0(j) / G::RPP) & 1) ? gsw[1] : gsw[0]; }
    // this lane's source offset when the piece's rows are contiguous at stride dp
    __device__ __forceinline__ int64_t poff(int j, int dp) const {
        return (int64_t)prow0(j) * dp + (pr * dp + psw(j));
    }
    // LDS byte offset of the piece inside a stage (the DMA destination is lane-linear)
    __device__ __forceinline__ uint32_t pdst(int j) const {
        const int pc = wave * G::LPW + j;
        return (uint32_t)(is_a(j) ? pc * 256 : G::SA + (pc - G::PA) * 256) * 4u;
    }
};

// Before a stage is read: this wave's own DMA of the stage landed (later stages may stay in
// flight), then everyone's did and the previous stage was read by all.  `remaining` = the stages
// not yet consumed after this one; the stages issued after it number min(NS - 2, remaining).
template <class G>
__device__ __forceinline__ void tile_stage_wait(int remaining) {
    if (remaining >= G::NS - 2) wait_vmcnt<G::LPW * (G::NS - 2)>();
    else if (G::NS > 3 && remaining == 1) wait_vmcnt<G::LPW>();
    else wait_vmcnt<0>();
    barrier_lds();
}

// One stage at `st` into the wave's WB accumulator blocks: the swizzled fragment reads of B and
// of the A blocks, the caller's issue_next (the next stage's DMA pieces), the MFMA chain.
// The pieces go out right after the fragment reads (their address math overlaps the LDS latency),
// before the MFMAs.  Measured alternatives, all slower: pieces pinned between MFMAs (38.6 ms vs
// 33.5 at BK=16), staggered per wave (38.8), a 5-deep ring (39.0).
template <class G, int MODE, class Issue>
__device__ __forceinline__ void tile_stage(const float* st, const TileLanes<G>& L, f32x16 (&acc)[G::WB],
                                           Issue&& issue_next) {
    constexpr int WB = G::WB, BK = G::BK, CPR = G::CPR;
    constexpr int KH = BK / 2;          // MFMA sub-steps per stage (each covers depth 2)
    float a[WB][KH], bq[KH];
    {
        const float* bp = st + G::SA + L.wq * 32 * BK;
#pragma unroll
        for (int c = 0; c < CPR / 2; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(bp + L.fo[c]);
            bq[4 * c] = v.x; bq[4 * c + 1] = v.y; bq[4 * c + 2] = v.z; bq[4 * c + 3] = v.w;
        }
    }
#pragma unroll
    for (int b = 0; b < WB; ++b) {
        const float* ap = st + (L.wr * G::RW + b * 32) * BK;
#pragma unroll
        for (int c = 0; c < CPR / 2; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(ap + L.fo[c]);
            a[b][4 * c] = v.x; a[b][4 * c + 1] = v.y; a[b][4 * c + 2] = v.z; a[b][4 * c + 3] = v.w;
        }
    }
    issue_next();                            // refills the buffer the previous stage used
    if constexpr (MODE == kModeBF16) {
        // bf16 rows (2 elements per 32-bit word): this lane half's chunk c holds the 8
        // elements of MFMA k-step c (depth 32h + 8c + 0..7 of the 64-deep stage, the same
        // permutation on both operands); one bf16 MFMA per product
#pragma unroll
        for (int c = 0; c < CPR / 2; ++c) {
            const bf16x8 bv = frag_bf16(bq, c);
#pragma unroll
            for (int b = 0; b < WB; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_bf16(a[b], c), bv, acc[b], 0, 0, 0);
        }
    } else if constexpr (MODE == kModeSplit) {
        // split layout: this lane half's chunks 2s / 2s+1 are the hi / lo bf16 planes of
        // MFMA k-step s; dot ~= hi.hi + hi.lo + lo.hi (the lo.lo term is below the bound)
#pragma unroll
        for (int s2 = 0; s2 < CPR / 4; ++s2) {
            const bf16x8 bh = frag_bf16(bq, 2 * s2), bl = frag_bf16(bq, 2 * s2 + 1);
#pragma unroll
            for (int b = 0; b < WB; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_bf16(a[b], 2 * s2), bh, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < WB; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_bf16(a[b], 2 * s2), bl, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < WB; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_bf16(a[b], 2 * s2 + 1), bh, acc[b], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < KH; ++kk) {
#pragma unroll
            for (int b = 0; b < WB; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[b][kk], bq[kk], acc[b], 0, 0, 0);
        }
    }
}

// The key of one pair from its inner product: the L2 distance (faiss exhaustive_L2sqr_blas form
// (|q|^2 + |x|^2) - 2 q.x, clamped at 0) when metric == 1, else -q.x.
__device__ __forceinline__ float tile_key(float ip, float qn, float xn, int metric) {
    if (metric != 1) return -ip;
    const float kv = fmaf(-2.f, ip, qn + xn);
    return kv < 0.f ? 0.f : kv;
}

// The 16 keys of one 32-row accumulator block.  `rb` = the tile row of accumulator register 0
// (register r holds row rb + (r & 3) + 8 * (r >> 2)), nrm = the tile's row norms in LDS, qn =
// |q|^2.  Returns the mask of the registers whose (row - rb, key) the caller's predicate passes;
// a NaN key fails any comparison there, so it is never returned.
template <class Pass>
__device__ __forceinline__ unsigned tile_keys(const f32x16& acc, const float* nrm, int rb, int metric,
                                              float qn, float (&key)[16], Pass&& pass) {
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                      // regs 4j..4j+3 = rows rb+8j+0..3
        float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (metric == 1) n4 = *reinterpret_cast<const float4*>(nrm + rb + 8 * j);
        const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * j + i;
            const float kv = tile_key(acc[r], qn, nv[i], metric);
            key[r] = kv;
            mask |= (unsigned)pass(8 * j + i, kv) << r;
        }
    }
    return mask;
}

// ---------------------------------------------------------------------------------------------
// Host side of the range and filter kernels: one geometry per batch size (256 rows x 32 queries
// for batches of <= 32, 128 x 128 beyond), one stage depth per row stride (32 when it divides, 16
// otherwise: the depth order of the keys), two workgroups per CU over the row splits.
// ---------------------------------------------------------------------------------------------
struct TilePlan { int wr, wq, bk, bm, bq, nqb, nq_pad, ntiles, nsplit; };

inline TilePlan make_tile_plan(int64_t ntotal, int64_t nq, int dp, int cus) {
    TilePlan p{};
    if (nq <= 32) { p.wr = 2; p.wq = 1; } else { p.wr = 1; p.wq = 4; }
    p.bk = dp % 32 == 0 ? 32 : 16;
    p.bm = p.wr * 128;
    p.bq = p.wq * 32;
    p.nqb = (int)((nq + p.bq - 1) / p.bq);
    p.nq_pad = p.nqb * p.bq;
    p.ntiles = (int)((ntotal + p.bm - 1) / p.bm);
    const int target = cus * 2;
    p.nsplit = std::max(1, std::min((target + p.nqb - 1) / p.nqb, p.ntiles));
    return p;
}

// launch(TileGeom<...>{}) with the ring of the plan's (wr, bk).
// 2-slot rings at 32-deep stages: 74 / 66 KiB of LDS, so two workgroups share a CU (a 3-slot
// ring of the 256 x 32 tile leaves one 2-wave workgroup, half the SIMDs, per CU)
template <class Launch>
inline void with_tile_ring(const TilePlan& p, Launch&& launch) {
    if (p.wr == 2 && p.bk == 32) launch(TileGeom<2, 1, 2, 32>{});
    else if (p.wr == 2) launch(TileGeom<2, 1, 3, 16>{});
    else if (p.bk == 32) launch(TileGeom<1, 4, 2, 32>{});
    else launch(TileGeom<1, 4, 2, 16>{});
}

}  // namespace imgrec
