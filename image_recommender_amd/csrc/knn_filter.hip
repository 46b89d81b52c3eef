// knn_filter.hip — filtered search (faiss SearchParameters::sel): the k nearest rows among the rows
// an IDSelectorBitmap-style bitmap selects, at a cost that follows the number of selected rows.
//
// Pipeline of one call (filtered_search_locked):
//   1. compaction, once per call: filter_count_kernel (a popcount per 8192-row block),
//      filter_scan_kernel (one workgroup: exclusive scan of the block counts, the count m, and the
//      list's tail padded to 256 entries with row 0) and filter_scatter_kernel -> the ascending
//      list of the selected local rows (uint32) and m, both in device memory.  On a shard of a
//      multi-device index the bit of local row r is bit lmap[r] of the global bitmap.  (remove_ids,
//      knn_remove.hip, runs the same compaction on the inverted bitmap: compact_rows.)
//   2. knn_filter_tile_kernel per query chunk: the contraction of knn_range_tile_kernel
//      (v_mfma_f32_32x32x2_f32, the same stage depth, geometries, depth order and block map), but
//      tile t holds the list entries [t BM, (t + 1) BM): every lane's 16-B DMA source is
//      xb + list[position] * dp + chunk, re-derived once per tile from the tile's list entries,
//      which reach LDS by a DMA of their own one tile ahead.  The grid is planned on the host from
//      ntotal; every workgroup reads m and derives its own tiles.
//      k <= KNN_MAX_K: per-lane sorted register lists of km (key, position) entries, strict `<`
//      insertion (positions ascend within a lane, so equal keys keep the smaller label), written
//      as [nq][lists][km] with labels list[position] + id_offset; launch_merge produces D / I.
//      k > KNN_MAX_K: every selected pair's (key bits << 32 | row) stored at q * m_pad + position
//      (the position is known: no atomics), one segmented sort over equal segments and an unpack
//      of the first k.  That route needs m on the host to size the sort: it waits once per call.
//
// Arithmetic: a pair's key is the bits knn_range_search returns for it: an MFMA output element
// depends on its own row and column only and the depth order is fixed by the row stride, so where
// a row sits in a gathered tile does not matter.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <math.h>

#include <algorithm>

#include "knn_index.h"
#include "lds_dma.h"
#include "wave_ops.h"

namespace imgrec {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- compaction ---------------------------------------------------------------------------------
constexpr int kCompThreads = 256;
constexpr int kCompRows = kCompThreads * 32;       // rows per block: one 32-row word per thread

// Bits of the local rows [32 w, 32 w + 32): row r is selected iff r < ntotal and bit g of the
// bitmap is set, g = lmap ? lmap[r] : r, g < nbits.
__device__ __forceinline__ uint32_t filter_word(const uint8_t* __restrict__ bm, int64_t nbits,
                                                const int64_t* __restrict__ lmap, int64_t ntotal,
                                                int64_t w) {
    const int64_t r0 = w * 32;
    if (r0 >= ntotal) return 0u;
    uint32_t bits = 0;
    if (lmap) {
        const int n = (int)min((int64_t)32, ntotal - r0);
        for (int i = 0; i < n; ++i) {
            const int64_t g = lmap[r0 + i];
            if (g >= 0 && g < nbits) bits |= (uint32_t)((bm[g >> 3] >> (g & 7)) & 1) << i;
        }
        return bits;
    }
    const int64_t lim = min(ntotal, nbits);
    if (r0 >= lim) return 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (r0 + 8 * b < lim) bits |= (uint32_t)bm[4 * w + b] << (8 * b);
    if (lim - r0 < 32) bits &= (1u << (int)(lim - r0)) - 1u;
    return bits;
}

// invert (remove_ids' survivors): the stored rows of the word whose bit is clear
__device__ __forceinline__ uint32_t comp_word(const uint8_t* __restrict__ bm, int64_t nbits,
                                              const int64_t* __restrict__ lmap, int64_t ntotal,
                                              int64_t w, int invert) {
    const uint32_t bits = filter_word(bm, nbits, lmap, ntotal, w);
    if (!invert) return bits;
    const int64_t left = ntotal - w * 32;
    const uint32_t stored = left >= 32 ? ~0u : (left > 0 ? (1u << (int)left) - 1u : 0u);
    return ~bits & stored;
}

__global__ void __launch_bounds__(kCompThreads)
filter_count_kernel(const uint8_t* __restrict__ bm, int64_t nbits, const int64_t* __restrict__ lmap,
                    int64_t ntotal, int invert, uint32_t* __restrict__ blk) {
    __shared__ int part[kCompThreads / 64];
    const int t = threadIdx.x;
    const uint32_t w = comp_word(bm, nbits, lmap, ntotal, (int64_t)blockIdx.x * kCompThreads + t, invert);
    const int s = wave_sum_i32(__popc(w));
    if ((t & 63) == 0) part[t >> 6] = s;
    __syncthreads();
    if (t == 0) blk[blockIdx.x] = (uint32_t)(part[0] + part[1] + part[2] + part[3]);
}

// blk[i] -> the start of block i's rows in the list (in place), *m = the selected count, and the
// list's tail [m, round_up(m, 256)) = row 0 (the tile kernel reads whole tiles).
__global__ void __launch_bounds__(256)
filter_scan_kernel(uint32_t* __restrict__ blk, int nblk, uint32_t* __restrict__ m,
                   uint32_t* __restrict__ list) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t tot;
    const int t = threadIdx.x;
    const int per = (nblk + 255) / 256;
    const int i0 = min(nblk, t * per), i1 = min(nblk, i0 + per);
    uint32_t s = 0;
    for (int i = i0; i < i1; ++i) s += blk[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int j = 0; j < 256; ++j) { const uint32_t v = part[j]; part[j] = run; run += v; }
        tot = run;
    }
    __syncthreads();
    uint32_t run = part[t];
    for (int i = i0; i < i1; ++i) { const uint32_t v = blk[i]; blk[i] = run; run += v; }
    const uint32_t mm = tot;
    if (t == 0) *m = mm;
    const uint32_t pad = (256u - (mm & 255u)) & 255u;
    if ((uint32_t)t < pad) list[(size_t)mm + t] = 0u;
}

__global__ void __launch_bounds__(kCompThreads)
filter_scatter_kernel(const uint8_t* __restrict__ bm, int64_t nbits, const int64_t* __restrict__ lmap,
                      int64_t ntotal, int invert, const uint32_t* __restrict__ blk,
                      uint32_t* __restrict__ list) {
    __shared__ int part[kCompThreads / 64];
    const int t = threadIdx.x;
    const int64_t wi = (int64_t)blockIdx.x * kCompThreads + t;
    uint32_t w = comp_word(bm, nbits, lmap, ntotal, wi, invert);
    const int c = __popc(w);
    const int ex = wave_excl_scan_i32(c);
    const int s = wave_sum_i32(c);
    if ((t & 63) == 0) part[t >> 6] = s;
    __syncthreads();
    int before = 0;
    for (int j = 0; j < (t >> 6); ++j) before += part[j];
    size_t at = (size_t)blk[blockIdx.x] + (size_t)(before + ex);
    const uint32_t r0 = (uint32_t)(wi * 32);
    while (w) {
        const int b = __builtin_ctz(w);
        w &= w - 1u;
        list[at++] = r0 + (uint32_t)b;
    }
}

// ---- the gathered tile kernel ---------------------------------------------------------------------
// knn_range.hip's tile geometry (WR x WQ waves of 128 rows x 32 queries, BK-deep stages in an NS
// ring, the tiles' norms in an NS ring) plus two slots of a tile's list entries.
template <int WR, int WQ, int NS, int BK>
struct FilterGeom {
    static constexpr int WB = 4;
    static constexpr int NW = WR * WQ, NT = NW * 64;
    static constexpr int RW = 32 * WB;
    static constexpr int BM = WR * RW, BQ = WQ * 32;
    static constexpr int CPR = BK / 4;                 // 16-B chunks per staged row
    static constexpr int RPP = 64 / CPR;               // rows per 1-KiB DMA piece
    static constexpr int RPB = 64 / BK;                // rows per 256-B bank row
    static constexpr int SA = BM * BK, SB = BQ * BK, STAGE = SA + SB;   // floats
    static constexpr int PA = BM / RPP, PB = BQ / RPP, PIECES = PA + PB;
    static constexpr int LPW = PIECES / NW;
    static constexpr int LDS_FLOATS = NS * STAGE + NS * BM + 2 * BM;
    static_assert(BK == 16 || BK == 32, "stage depth");
    static_assert(PIECES % NW == 0, "pieces must divide evenly over waves");
    static_assert(BM % 64 == 0, "norm and list DMAs use whole waves");
    static_assert(NS == 2 || NS == 3, "the prologue and the vmcnt waits assume a 2- or 3-slot ring");
    static_assert(LDS_FLOATS * 4 <= (NW == 4 || BK == 32 ? 80 : 160) * 1024, "LDS budget (two workgroups per CU)");
};

__device__ __forceinline__ void dma16(const float* g, uint32_t lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep) : "v"(g), "s"(__builtin_amdgcn_readfirstlane(lds)) : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// knn_kernels.hip's list_insert_mono: insertion into an ascending list when a lane's ids arrive
// in increasing order, so an equal key lands behind the entries already there.
template <int K>
__device__ __forceinline__ void list_insert_mono(float (&kd)[K], int (&ki)[K], float d, int id) {
    bool c[K];
#pragma unroll
    for (int p = 0; p < K; ++p) c[p] = d < kd[p];
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
        kd[p] = __builtin_amdgcn_fmed3f(kd[p - 1], d, kd[p]);
        ki[p] = c[p - 1] ? ki[p - 1] : (c[p] ? id : ki[p]);
    }
    kd[0] = c[0] ? d : kd[0];
    ki[0] = c[0] ? id : ki[0];
}

struct FilterArgs {
    const float* xb;            // corpus, row stride dp
    const float* xnorm;
    int dp;
    const float* qp;            // nqb x BQ padded queries
    const float* qnorm;
    int nq, metric;             // metric 1 = L2, otherwise inner product
    const uint32_t* list;       // the selected rows, ascending, padded with row 0 to 256 entries
    const uint32_t* m;          // their count (device)
    int nsplit, nqb;
    int64_t id_offset;
    float* cand_d;              // k <= KNN_MAX_K: nq x ncand keys ...
    int64_t* cand_i;            // ... and labels (-1 = empty)
    int ncand;
    uint64_t* all;              // k > KNN_MAX_K: nq x m_pad (key bits << 32 | row), preset to ~0
    uint32_t m_pad;
};

// KM = 16 / 32: the register-list epilogue; KM = 0: the store-everything epilogue (any k)
template <int WR, int WQ, int NS, int BK, int KM>
__global__ void __launch_bounds__(WR * WQ * 64, WR * WQ == 4 ? 2 : 1)
knn_filter_tile_kernel(const FilterArgs a) {
    using G = FilterGeom<WR, WQ, NS, BK>;
    constexpr int WB = G::WB, RW = G::RW;
    constexpr int NW = G::NW, BM = G::BM, BQ = G::BQ, SA = G::SA, STAGE = G::STAGE;
    constexpr int PA = G::PA, LPW = G::LPW, CPR = G::CPR, RPP = G::RPP, RPB = G::RPB;
    constexpr int KH = BK / 2;
    constexpr int KL = KM > 0 ? KM : 1;
    __shared__ __attribute__((aligned(16))) float smem[G::LDS_FLOATS];
    // XCD-aware block -> (query block, row split) map of the exact kernel
    const int nwg = gridDim.x, wg = blockIdx.x;
    const int xcd = wg & 7, qq = nwg >> 3, rr8 = nwg & 7;
    const int wgid = (xcd < rr8 ? xcd * (qq + 1) : rr8 * (qq + 1) + (xcd - rr8) * qq) + (wg >> 3);
    const int nqb = a.nqb, nsplit = a.nsplit, dp = a.dp;
    if (wgid >= nqb * nsplit) return;
    float* const norm_base = smem + NS * STAGE;
    const uint32_t* const list_base = reinterpret_cast<const uint32_t*>(norm_base + NS * BM);
    const int qb = wgid % nqb;
    const int split = wgid / nqb;
    // the tiles of the compacted list: workgroup-uniform, from the device count
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)*a.m);
    const int ntiles = (int)((m + (uint32_t)(BM - 1)) / (uint32_t)BM);
    const int t1 = split < ntiles ? (ntiles - split + nsplit - 1) / nsplit : 0;
    auto tile = [&](int j) { return split + j * nsplit; };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WQ;
    const int wq = wave % WQ;
    const int li = lane & 31;
    const int lh = lane >> 5;
    const int qcol = qb * BQ + wq * 32 + li;     // < nq_pad
    const bool qvalid = qcol < a.nq;
    const int metric = a.metric;
    float qn = (metric == 1) ? a.qnorm[qcol] : 0.f;
    asm volatile("" : "+v"(qn));

    const int prow = lane / CPR, pchk = lane % CPR;
    // a piece's swizzled chunk offset depends on its place in the tile (piece parity), not on the
    // row it holds: the swizzle goes through the source address
    const int gsw0 = 4 * (pchk ^ (((0 * RPP + prow) / RPB) % CPR));
    const int gsw1 = 4 * (pchk ^ (((1 * RPP + prow) / RPB) % CPR));
    const int fsw = (li / RPB) % CPR;
    int fo[CPR / 2];
#pragma unroll
    for (int c = 0; c < CPR / 2; ++c) fo[c] = li * BK + 4 * ((lh * (CPR / 2) + c) ^ fsw);

    float kd[KL];
    int ki[KL];
#pragma unroll
    for (int p = 0; p < KL; ++p) { kd[p] = INFINITY; ki[p] = -1; }

    const int nsteps = dp / BK;
    const float* qbase = a.qp + (size_t)qb * BQ * dp;

    int64_t poff[LPW];          // query pieces: fixed; corpus pieces: re-derived per tile
    bool pis_a[LPW];
    uint32_t pdst[LPW];
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
        const int pc = wave * LPW + j;
        pis_a[j] = pc < PA;
        const int prow0 = pis_a[j] ? pc * RPP : (pc - PA) * RPP;
        poff[j] = (int64_t)(prow0 + prow) * dp + (((prow0 / RPP) & 1) ? gsw1 : gsw0);
        pdst[j] = (uint32_t)(pis_a[j] ? pc * 256 : SA + (pc - PA) * 256) * 4u;
    }
    const uint32_t smem_u32 = lds_u32(smem);
    const uint32_t norm_u32 = lds_u32(norm_base);
    const uint32_t list_u32 = lds_u32(list_base);
    // the list entries of this split's j-th tile into list slot j & 1 (one dword per lane)
    auto issue_list = [&](int j) __attribute__((always_inline)) {
        for (int jj = wave; jj < BM / 64; jj += NW)
            dma4_norm(reinterpret_cast<const float*>(a.list + (size_t)tile(j) * BM + jj * 64 + lane),
                      list_u32 + (uint32_t)((j & 1) * BM + jj * 64) * 4u);
    };
    int it = 0, is = 0, ibuf = 0;
    // One stage's DMAs.  At a tile's first stage: the tile's list entries (landed in LDS: their DMA
    // went out a whole issue call earlier, before that call's pieces, and every consumer wait
    // leaves at most the last call's pieces in flight) give the corpus pieces' row bases and the
    // norm gather; then the next tile's entries go out, all before this stage's pieces.
    auto issue_next = [&]() __attribute__((always_inline)) {
        if (it >= t1) return;
        const uint32_t st = smem_u32 + (uint32_t)(ibuf * STAGE) * 4u;
        if (is == 0) {
            const uint32_t* ls = list_base + (it & 1) * BM;
#pragma unroll
            for (int j = 0; j < LPW; ++j) {
                if (pis_a[j]) {
                    const int pc = wave * LPW + j;
                    poff[j] = (int64_t)ls[pc * RPP + prow] * dp + ((pc & 1) ? gsw1 : gsw0);
                }
            }
            for (int jj = wave; jj < BM / 64; jj += NW)
                dma4_norm(a.xnorm + ls[jj * 64 + lane],
                          norm_u32 + (uint32_t)((it % NS) * BM + jj * 64) * 4u);
            if (it + 1 < t1) issue_list(it + 1);
        }
        const int k0 = is * BK;
#pragma unroll
        for (int j = 0; j < LPW; ++j) dma16((pis_a[j] ? a.xb : qbase) + poff[j] + k0, st + pdst[j]);
        if (++is == nsteps) { is = 0; ++it; }
        ibuf = (ibuf + 1 == NS) ? 0 : ibuf + 1;
    };

    if (t1 > 0) {                                // workgroup-uniform
        issue_list(0);
        wait_vmcnt<0>();
        barrier_lds();
#pragma unroll
        for (int j = 0; j < NS - 1; ++j) {
            issue_next();
            if (j + 1 < NS - 1) {                // a second prologue stage may start the next tile
                wait_vmcnt<0>();
                barrier_lds();
            }
        }
    }
    int remaining = t1 * nsteps;
    int cbuf = 0;

    for (int t = 0; t < t1; ++t) {
        const uint32_t pos0 = (uint32_t)tile(t) * BM;
        f32x16 acc[WB];
#pragma unroll
        for (int b = 0; b < WB; ++b) acc[b] = (f32x16){0.f};

        for (int s = 0; s < nsteps; ++s) {
            --remaining;
            if (remaining >= NS - 2) wait_vmcnt<LPW * (NS - 2)>();
            else wait_vmcnt<0>();
            barrier_lds();                       // everyone's DMA landed; previous stage read

            const float* st = smem + cbuf * STAGE;
            cbuf = (cbuf + 1 == NS) ? 0 : cbuf + 1;
            float av[WB][KH], bq[KH];
            {
                const float* bp = st + SA + wq * 32 * BK;
#pragma unroll
                for (int c = 0; c < CPR / 2; ++c) {
                    const float4 v = *reinterpret_cast<const float4*>(bp + fo[c]);
                    bq[4 * c] = v.x; bq[4 * c + 1] = v.y; bq[4 * c + 2] = v.z; bq[4 * c + 3] = v.w;
                }
            }
#pragma unroll
            for (int b = 0; b < WB; ++b) {
                const float* ap = st + (wr * RW + b * 32) * BK;
#pragma unroll
                for (int c = 0; c < CPR / 2; ++c) {
                    const float4 v = *reinterpret_cast<const float4*>(ap + fo[c]);
                    av[b][4 * c] = v.x; av[b][4 * c + 1] = v.y; av[b][4 * c + 2] = v.z; av[b][4 * c + 3] = v.w;
                }
            }
            issue_next();                        // refills the buffer the previous stage used
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) {
#pragma unroll
                for (int b = 0; b < WB; ++b)
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[b][kk], bq[kk], acc[b], 0, 0, 0);
            }
        }

        // ---- epilogue.  The tile's norms landed before its first stage's barrier; their ring
        // slot is rewritten NS tiles later, behind a barrier every wave reaches only after this
        // epilogue.  Positions at or past m are the sentinel entries (row 0): excluded.
        const float* nrm = norm_base + (t % NS) * BM;
#pragma unroll
        for (int b = 0; b < WB; ++b) {
            float key[16];
            unsigned mask = 0;
            const float tau = kd[KL - 1];
            const float tau_p = __shfl_xor(tau, 32, 64);       // the query's other rows' list
            const int rb = wr * RW + b * 32 + 4 * lh;          // position of accumulator reg 0
#pragma unroll
            for (int j = 0; j < 4; ++j) {                      // regs 4j..4j+3 = positions rb+8j+0..3
                float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (metric == 1) n4 = *reinterpret_cast<const float4*>(nrm + rb + 8 * j);
                const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 4 * j + i;
                    const float ip = acc[b][r];
                    float kv;
                    if (metric == 1) {
                        kv = fmaf(-2.f, ip, qn + nv[i]);
                        kv = kv < 0.f ? 0.f : kv;
                    } else {
                        kv = -ip;
                    }
                    key[r] = kv;
                    bool pass = qvalid && (pos0 + (uint32_t)(rb + 8 * j + i) < m);
                    // a NaN key fails the comparisons: never returned
                    if (KM > 0) pass = pass && kv < tau && kv <= tau_p;
                    mask |= (unsigned)pass << r;
                }
            }
            if constexpr (KM > 0) {
                // a lane's positions ascend with r, b and t: strict `<` keeps the smaller label
                // (one survivor per lane and iteration, ctz walk of the lane's own mask; the key
                // comes out of its register by a select chain, so there is one insertion site)
                while (__any(mask != 0)) {
                    if (mask) {
                        const int r = __builtin_ctz(mask);
                        mask &= mask - 1u;
                        float kv = key[0];
#pragma unroll
                        for (int i = 1; i < 16; ++i) kv = r == i ? key[i] : kv;
                        if (kv < kd[KL - 1])
                            list_insert_mono<KL>(kd, ki, kv, (int)(pos0 + (uint32_t)(rb + (r & 3) + 8 * (r >> 2))));
                    }
                }
            } else {
                uint64_t* out = a.all + (size_t)qcol * a.m_pad;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if ((mask >> r) & 1u) {
                        const uint32_t pos = pos0 + (uint32_t)(rb + (r & 3) + 8 * (r >> 2));
                        const float kv = key[r];
                        out[pos] = kv != kv ? ~0ull
                                            : (((uint64_t)key_bits_ordered(kv) << 32) | a.list[pos]);
                    }
                }
            }
        }
    }

    if constexpr (KM > 0) {
        // a workgroup with no tile writes empty lists: the merge reads every list
        if (qvalid) {
            const size_t base = (size_t)qcol * a.ncand + (size_t)((split * WR + wr) * 2 + lh) * KM;
#pragma unroll
            for (int p = 0; p < KM; ++p) {
                a.cand_d[base + p] = kd[p];
                a.cand_i[base + p] = ki[p] < 0 ? (int64_t)-1 : (int64_t)a.list[ki[p]] + a.id_offset;
            }
        }
    }
}

__global__ void filter_offsets_kernel(unsigned* off, int nseg, uint32_t seg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= nseg) off[i] = (unsigned)i * seg;
}

// Row q of D / I from the first k sorted values of segment q (~0 = empty: past m, or a NaN key).
__global__ void __launch_bounds__(256)
filter_unpack_kernel(const uint64_t* __restrict__ sorted, uint32_t seg, int k, int metric,
                     int64_t id_offset, float* __restrict__ D, int64_t* __restrict__ I) {
    const int64_t q = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const uint64_t x = i < (int64_t)seg ? sorted[q * seg + i] : ~0ull;
    if (x == ~0ull) {
        D[q * k + i] = metric == 1 ? FLT_MAX : -FLT_MAX;
        I[q * k + i] = -1;
    } else {
        const float key = key_from_ordered((uint32_t)(x >> 32));
        D[q * k + i] = metric == 1 ? key : -key;
        I[q * k + i] = (int64_t)(uint32_t)x + id_offset;
    }
}

struct FilterPlan { int wr, wq, bk, bm, bq, nqb, nq_pad, nsplit, km, ncand; };

// knn_range.hip's plan: one geometry per batch size, one stage depth per row stride.  The row
// splits are planned from ntotal, an upper bound of the selected count.
FilterPlan make_filter_plan(int64_t ntotal, int64_t nq, int k, int dp, int cus) {
    FilterPlan p{};
    if (nq <= 32) { p.wr = 2; p.wq = 1; } else { p.wr = 1; p.wq = 4; }
    p.bk = dp % 32 == 0 ? 32 : 16;
    p.bm = p.wr * 128;
    p.bq = p.wq * 32;
    p.nqb = (int)((nq + p.bq - 1) / p.bq);
    p.nq_pad = p.nqb * p.bq;
    const int ntiles = (int)((ntotal + p.bm - 1) / p.bm);
    const int target = cus * 2;
    p.nsplit = std::max(1, std::min((target + p.nqb - 1) / p.nqb, ntiles));
    p.km = k > KNN_MAX_K ? 0 : (k <= 16 ? 16 : 32);
    p.ncand = p.nsplit * p.wr * 2 * p.km;
    return p;
}

template <int KM>
hipError_t launch_filter_tile_km(const FilterPlan& p, const FilterArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)(p.nqb * p.nsplit));
#define IMGREC_FILTER_LAUNCH(WRV, WQV, NSV, BKV)                                                  \
    hipLaunchKernelGGL((knn_filter_tile_kernel<WRV, WQV, NSV, BKV, KM>), grid, dim3(WRV * WQV * 64), 0, st, a)
    // the rings of knn_range.hip's launches
    if (p.wr == 2 && p.bk == 32) IMGREC_FILTER_LAUNCH(2, 1, 2, 32);
    else if (p.wr == 2) IMGREC_FILTER_LAUNCH(2, 1, 3, 16);
    else if (p.bk == 32) IMGREC_FILTER_LAUNCH(1, 4, 2, 32);
    else IMGREC_FILTER_LAUNCH(1, 4, 2, 16);
#undef IMGREC_FILTER_LAUNCH
    return hipGetLastError();
}

hipError_t launch_filter_tile(const FilterPlan& p, const FilterArgs& a, hipStream_t st) {
    if (p.km == 16) return launch_filter_tile_km<16>(p, a, st);
    if (p.km == 32) return launch_filter_tile_km<32>(p, a, st);
    return launch_filter_tile_km<0>(p, a, st);
}

// keys of one any-k chunk: knn_hugek.hip's workspace cap (1 GiB of u64, twice for the sort)
constexpr int64_t kFilterSortEntries = int64_t(1) << 27;
constexpr int64_t kFilterSortMaxQ = 65535;         // the unpack grid's y extent

int compact(knn_index* ix, const uint8_t* bits, int64_t nbits, const int64_t* lmap, bool invert,
            hipStream_t st) {
    int rc;
    const int nblk = (int)((ix->ntotal + kCompRows - 1) / kCompRows);
    if ((rc = grow(&ix->ft_list, &ix->ft_list_cap, (size_t)round_up(ix->ntotal, 256) + 256)) != KNN_OK) return rc;
    if ((rc = grow(&ix->ft_blk, &ix->ft_blk_cap, (size_t)nblk)) != KNN_OK) return rc;
    if ((rc = grow(&ix->ft_m, &ix->ft_m_cap, (size_t)1)) != KNN_OK) return rc;
    hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)nblk), dim3(kCompThreads), 0, st, bits, nbits,
                       lmap, ix->ntotal, invert ? 1 : 0, ix->ft_blk);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(256), 0, st, ix->ft_blk, nblk, ix->ft_m, ix->ft_list);
    KNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(filter_scatter_kernel, dim3((unsigned)nblk), dim3(kCompThreads), 0, st, bits, nbits,
                       lmap, ix->ntotal, invert ? 1 : 0, ix->ft_blk, ix->ft_list);
    KNN_HIP(hipGetLastError());
    return KNN_OK;
}

FilterArgs base_args(const knn_index* ix, const FilterPlan& p, int64_t cn) {
    FilterArgs a{};
    a.xb = ix->xb; a.xnorm = ix->xn; a.dp = ix->dp;
    a.qp = ix->qpad; a.qnorm = ix->qnorm; a.nq = (int)cn;
    a.metric = ix->metric == KNN_METRIC_L2 ? 1 : 0;
    a.list = ix->ft_list; a.m = ix->ft_m;
    a.nsplit = p.nsplit; a.nqb = p.nqb; a.id_offset = ix->id_offset;
    return a;
}

// k <= KNN_MAX_K: register lists and the list merge; nothing reaches the host
int filtered_lists(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I, hipStream_t st) {
    const int normalize = ix->metric == KNN_METRIC_COSINE;
    int rc;
    for (int64_t c0 = 0; c0 < nq; c0 += kQueryChunk) {
        const int64_t cn = std::min(kQueryChunk, nq - c0);
        const FilterPlan p = make_filter_plan(ix->ntotal, cn, k, ix->dp, ix->cus);
        if ((rc = grow(&ix->qpad, &ix->qpad_cap, (size_t)p.nq_pad * ix->dp)) != KNN_OK) return rc;
        if ((rc = grow(&ix->qnorm, &ix->qnorm_cap, (size_t)p.nq_pad)) != KNN_OK) return rc;
        if ((rc = grow(&ix->cand_d, &ix->cand_d_cap, (size_t)cn * p.ncand)) != KNN_OK) return rc;
        if ((rc = grow(&ix->cand_i, &ix->cand_i_cap, (size_t)cn * p.ncand)) != KNN_OK) return rc;
        KNN_HIP(launch_rows_ingest(q + c0 * ix->d, cn, ix->d, ix->dp, p.nq_pad, normalize, ix->qpad,
                                   ix->qnorm, st));
        FilterArgs a = base_args(ix, p, cn);
        a.cand_d = ix->cand_d; a.cand_i = ix->cand_i; a.ncand = p.ncand;
        hipEvent_t e1 = nullptr;                  // knn_set_timing: the tile kernel's own time
        if ((rc = timed_begin(ix, st, &e1)) != KNN_OK) return rc;
        KNN_HIP(launch_filter_tile(p, a, st));
        if (e1) KNN_HIP(hipEventRecord(e1, st));
        KNN_HIP(launch_merge(ix->cand_d, ix->cand_i, cn, p.ncand / p.km, p.km, p.ncand, p.km, k, a.metric,
                             0, D + c0 * k, I + c0 * k, st));
    }
    return KNN_OK;
}

// k > KNN_MAX_K: every selected pair's key, a segmented sort, the first k.  Waits once for m.
int filtered_sorted(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I, hipStream_t st) {
    const int normalize = ix->metric == KNN_METRIC_COSINE;
    const int kmetric = ix->metric == KNN_METRIC_L2 ? 1 : 0;
    int rc;
    if (!ix->ft_m_h) KNN_HIP(hipHostMalloc((void**)&ix->ft_m_h, sizeof(uint32_t), hipHostMallocDefault));
    KNN_HIP(hipMemcpyAsync(ix->ft_m_h, ix->ft_m, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KNN_HIP(hipStreamSynchronize(st));
    const int64_t m = (int64_t)*ix->ft_m_h;
    if (m == 0) {
        KNN_HIP(launch_fill_empty(D, I, nq * (int64_t)k, kmetric, st));
        return KNN_OK;
    }
    const int64_t m_pad = round_up(m, 256);
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>({nq, kFilterSortEntries / m_pad, kFilterSortMaxQ,
                                                                kQueryChunk}));
    if ((rc = grow(&ix->hk_a, &ix->hk_a_cap, (size_t)(per * m_pad))) != KNN_OK) return rc;
    if ((rc = grow(&ix->hk_b, &ix->hk_b_cap, (size_t)(per * m_pad))) != KNN_OK) return rc;
    if ((rc = grow(&ix->hk_off, &ix->hk_off_cap, (size_t)per + 1)) != KNN_OK) return rc;
    for (int64_t c0 = 0; c0 < nq; c0 += per) {
        const int64_t cn = std::min(per, nq - c0);
        const FilterPlan p = make_filter_plan(ix->ntotal, cn, k, ix->dp, ix->cus);
        if ((rc = grow(&ix->qpad, &ix->qpad_cap, (size_t)p.nq_pad * ix->dp)) != KNN_OK) return rc;
        if ((rc = grow(&ix->qnorm, &ix->qnorm_cap, (size_t)p.nq_pad)) != KNN_OK) return rc;
        KNN_HIP(launch_rows_ingest(q + c0 * ix->d, cn, ix->d, ix->dp, p.nq_pad, normalize, ix->qpad,
                                   ix->qnorm, st));
        KNN_HIP(hipMemsetAsync(ix->hk_a, 0xff, (size_t)(cn * m_pad) * sizeof(uint64_t), st));
        FilterArgs a = base_args(ix, p, cn);
        a.all = ix->hk_a; a.m_pad = (uint32_t)m_pad;
        hipEvent_t e1 = nullptr;
        if ((rc = timed_begin(ix, st, &e1)) != KNN_OK) return rc;
        KNN_HIP(launch_filter_tile(p, a, st));
        if (e1) KNN_HIP(hipEventRecord(e1, st));
        hipLaunchKernelGGL(filter_offsets_kernel, dim3((unsigned)((cn + 256) / 256)), dim3(256), 0, st,
                           ix->hk_off, (int)cn, (uint32_t)m_pad);
        KNN_HIP(hipGetLastError());
        KNN_HIP(sort_u64_segments(ix->hk_a, ix->hk_b, cn * m_pad, (int)cn, ix->hk_off, 64u, &ix->hk_tmp,
                                  &ix->hk_tmp_cap, false, st));
        hipLaunchKernelGGL(filter_unpack_kernel, dim3((unsigned)((k + 255) / 256), (unsigned)cn), dim3(256), 0,
                           st, ix->hk_b, (uint32_t)m_pad, k, kmetric, ix->id_offset, D + c0 * k, I + c0 * k);
        KNN_HIP(hipGetLastError());
    }
    return KNN_OK;
}

}  // namespace

int filtered_search_locked(knn_index* ix, const float* q, int64_t nq, int k, const uint8_t* bits,
                           int64_t nbits, const int64_t* lmap, float* D, int64_t* I, hipStream_t st) {
    if (ix->ntotal >= (int64_t(1) << 32))
        KNN_FAIL(KNN_EINVAL, "filtered search: %lld rows in one shard (limit 2^32 - 1): split the index "
                 "over more shards", (long long)ix->ntotal);
    ix->last_path = 0;
    ix->last_split_queries = 0;
    ix->stat_valid = false;
    if (nq == 0) return KNN_OK;
    if (ix->ntotal == 0 || nbits == 0) {
        KNN_HIP(launch_fill_empty(D, I, nq * (int64_t)k, ix->metric == KNN_METRIC_L2 ? 1 : 0, st));
        return KNN_OK;
    }
    int rc;
    if ((rc = compact(ix, bits, nbits, lmap, false, st)) != KNN_OK) return rc;
    return k <= KNN_MAX_K ? filtered_lists(ix, q, nq, k, D, I, st) : filtered_sorted(ix, q, nq, k, D, I, st);
}

int compact_rows(knn_index* ix, const uint8_t* bits, int64_t nbits, const int64_t* lmap, bool invert,
                 hipStream_t st) {
    return compact(ix, bits, nbits, lmap, invert, st);
}

void filter_free(knn_index* ix) {
    for (void* p : {(void*)ix->ft_list, (void*)ix->ft_blk, (void*)ix->ft_m, (void*)ix->ft_bits})
        if (p) (void)hipFree(p);
    if (ix->ft_m_h) (void)hipHostFree(ix->ft_m_h);
    ix->ft_list = ix->ft_blk = ix->ft_m = ix->ft_m_h = nullptr;
    ix->ft_bits = nullptr;
    ix->ft_list_cap = ix->ft_blk_cap = ix->ft_m_cap = ix->ft_bits_cap = 0;
}

}  // namespace imgrec
