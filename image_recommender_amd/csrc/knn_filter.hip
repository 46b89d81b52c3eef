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
//   2. knn_filter_tile_kernel per query chunk: the tile core of knn_tile.h, as the range kernel
//      uses it (v_mfma_f32_32x32x2_f32, the same stage depth, geometries, depth order and block
//      map), but tile t holds the list entries [t BM, (t + 1) BM): every lane's 16-B DMA source is
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
#include "knn_tile.h"
#include "wave_ops.h"

namespace imgrec {
namespace {

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
// The tile core's ring (NS stages, the tiles' norms in an NS ring) plus two slots of a tile's list
// entries; the plan's geometries at two workgroups per CU.
template <class G>
struct FilterLds {
    static constexpr int FLOATS = G::LDS_FLOATS + 2 * G::BM;
    static_assert(G::NS == 2 || G::NS == 3, "the prologue and the vmcnt waits assume a 2- or 3-slot ring");
    static_assert(FLOATS * 4 <= (G::NW == 4 || G::BK == 32 ? 80 : 160) * 1024, "LDS budget (two workgroups per CU)");
};

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
__global__ void __launch_bounds__(WR * WQ * 64, (TileGeom<WR, WQ, NS, BK>::MIN_WAVES))
knn_filter_tile_kernel(const FilterArgs a) {
    using G = TileGeom<WR, WQ, NS, BK>;
    constexpr int WB = G::WB, RW = G::RW, NW = G::NW, BM = G::BM, BQ = G::BQ, STAGE = G::STAGE;
    constexpr int LPW = G::LPW;
    constexpr int KL = KM > 0 ? KM : 1;
    __shared__ __attribute__((aligned(16))) float smem[FilterLds<G>::FLOATS];
    const int wgid = xcd_wgid();                 // block -> (query block, row split)
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
    const TileLanes<G> L(lane, wave);
    const int wr = L.wr, lh = L.lh;
    const int qcol = qb * BQ + L.wq * 32 + L.li; // < nq_pad
    const bool qvalid = qcol < a.nq;
    const int metric = a.metric;
    float qn = (metric == 1) ? a.qnorm[qcol] : 0.f;
    asm volatile("" : "+v"(qn));

    float kd[KL];
    int ki[KL];
#pragma unroll
    for (int p = 0; p < KL; ++p) { kd[p] = INFINITY; ki[p] = -1; }

    const int nsteps = dp / BK;
    const float* qbase = a.qp + (size_t)qb * BQ * dp;

    // this lane's source of piece j (TileLanes).  Query pieces: fixed; corpus pieces: re-derived
    // per tile from the list entry at the piece row's position
    int64_t poff[LPW];
#pragma unroll
    for (int j = 0; j < LPW; ++j) poff[j] = L.poff(j, dp);
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
            for (int j = 0; j < LPW; ++j)
                if (L.is_a(j)) poff[j] = (int64_t)ls[L.prow(j)] * dp + L.psw(j);
            for (int jj = wave; jj < BM / 64; jj += NW)
                dma4_norm(a.xnorm + ls[jj * 64 + lane],
                          norm_u32 + (uint32_t)((it % NS) * BM + jj * 64) * 4u);
            if (it + 1 < t1) issue_list(it + 1);
        }
        const int k0 = is * BK;
#pragma unroll
        for (int j = 0; j < LPW; ++j) dma16((L.is_a(j) ? a.xb : qbase) + poff[j] + k0, st + L.pdst(j));
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
            tile_stage_wait<G>(remaining);
            const float* st = smem + cbuf * STAGE;
            cbuf = (cbuf + 1 == NS) ? 0 : cbuf + 1;
            tile_stage<G, kModeF32>(st, L, acc, issue_next);
        }

        // ---- epilogue.  The tile's norms landed before its first stage's barrier; their ring
        // slot is rewritten NS tiles later, behind a barrier every wave reaches only after this
        // epilogue.  Positions at or past m are the sentinel entries (row 0): excluded.
        const float* nrm = norm_base + (t % NS) * BM;
#pragma unroll
        for (int b = 0; b < WB; ++b) {
            float key[16];
            const float tau = kd[KL - 1];
            const float tau_p = __shfl_xor(tau, 32, 64);       // the query's other rows' list
            const int rb = wr * RW + b * 32 + 4 * lh;          // position of accumulator reg 0
            // tile_keys' loop with this kernel's test written in place: through the shared helper
            // and a predicate the 128 x 128 tiles ran 0.5 - 0.75 % slower at a full mask
            // (profiles/tile_core/README.md); the key formula itself is the shared tile_key
            unsigned mask = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {                      // regs 4j..4j+3 = positions rb+8j+0..3
                float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (metric == 1) n4 = *reinterpret_cast<const float4*>(nrm + rb + 8 * j);
                const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 4 * j + i;
                    const float kv = tile_key(acc[b][r], qn, nv[i], metric);
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

// The tile plan (the row splits are planned from ntotal, an upper bound of the selected count)
// and the candidate lists of the k <= KNN_MAX_K route.
struct FilterPlan : TilePlan { int km, ncand; };

FilterPlan make_filter_plan(int64_t ntotal, int64_t nq, int k, int dp, int cus) {
    FilterPlan p{};
    static_cast<TilePlan&>(p) = make_tile_plan(ntotal, nq, dp, cus);
    p.km = k > KNN_MAX_K ? 0 : (k <= 16 ? 16 : 32);
    p.ncand = p.nsplit * p.wr * 2 * p.km;
    return p;
}

template <int KM>
hipError_t launch_filter_tile_km(const FilterPlan& p, const FilterArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)(p.nqb * p.nsplit));
    with_tile_ring(p, [&](auto g) {
        using G = decltype(g);
        hipLaunchKernelGGL((knn_filter_tile_kernel<G::WR, G::WQ, G::NS, G::BK, KM>), grid, dim3(G::NT), 0, st, a);
    });
    return hipGetLastError();
}

hipError_t launch_filter_tile(const FilterPlan& p, const FilterArgs& a, hipStream_t st) {
    if (p.km == 16) return launch_filter_tile_km<16>(p, a, st);
    if (p.km == 32) return launch_filter_tile_km<32>(p, a, st);
    return launch_filter_tile_km<0>(p, a, st);
}

// keys of one any-k chunk: knn_hugek.hip's workspace cap (1 GiB of u64, twice for the sort)
constexpr int64_t kFilterSortEntries = int64_t(1) << 27;
constexpr int64_t kFilterSortMaxQ = 65535;         // the write grid's y extent

int compact(knn_index* ix, const uint8_t* bits, int64_t nbits, const int64_t* lmap, bool invert,
            hipStream_t st) {
    int rc;
    const int nblk = (int)((ix->ntotal + kCompRows - 1) / kCompRows);
    if ((rc = ix->ft_list.reserve((size_t)round_up(ix->ntotal, 256) + 256)) != KNN_OK) return rc;
    if ((rc = ix->ft_blk.reserve((size_t)nblk)) != KNN_OK) return rc;
    if ((rc = ix->ft_m.reserve((size_t)1)) != KNN_OK) return rc;
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
        if ((rc = ix->qpad.reserve((size_t)p.nq_pad * ix->dp)) != KNN_OK) return rc;
        if ((rc = ix->qnorm.reserve((size_t)p.nq_pad)) != KNN_OK) return rc;
        if ((rc = ix->cand_d.reserve((size_t)cn * p.ncand)) != KNN_OK) return rc;
        if ((rc = ix->cand_i.reserve((size_t)cn * p.ncand)) != KNN_OK) return rc;
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
    if ((rc = ix->ft_m_h.reserve(1)) != KNN_OK) return rc;
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
    if ((rc = ix->hk_a.reserve((size_t)(per * m_pad))) != KNN_OK) return rc;
    if ((rc = ix->hk_b.reserve((size_t)(per * m_pad))) != KNN_OK) return rc;
    if ((rc = ix->hk_off.reserve((size_t)per + 1)) != KNN_OK) return rc;
    for (int64_t c0 = 0; c0 < nq; c0 += per) {
        const int64_t cn = std::min(per, nq - c0);
        const FilterPlan p = make_filter_plan(ix->ntotal, cn, k, ix->dp, ix->cus);
        if ((rc = ix->qpad.reserve((size_t)p.nq_pad * ix->dp)) != KNN_OK) return rc;
        if ((rc = ix->qnorm.reserve((size_t)p.nq_pad)) != KNN_OK) return rc;
        KNN_HIP(launch_rows_ingest(q + c0 * ix->d, cn, ix->d, ix->dp, p.nq_pad, normalize, ix->qpad,
                                   ix->qnorm, st));
        KNN_HIP(hipMemsetAsync(ix->hk_a, 0xff, (size_t)(cn * m_pad) * sizeof(uint64_t), st));
        FilterArgs a = base_args(ix, p, cn);
        a.all = ix->hk_a; a.m_pad = (uint32_t)m_pad;
        hipEvent_t e1 = nullptr;
        if ((rc = timed_begin(ix, st, &e1)) != KNN_OK) return rc;
        KNN_HIP(launch_filter_tile(p, a, st));
        if (e1) KNN_HIP(hipEventRecord(e1, st));
        // ~0 = empty (past m, or a NaN key): sorts last, written as a padding entry
        KNN_HIP(sort_equal_segments(ix->hk_a, ix->hk_b, (int)cn, m_pad, 64u, ix->hk_off, ix->hk_tmp, st));
        KNN_HIP(launch_sorted_write(ix->hk_b, m_pad, (int)cn, k, kmetric, 32, ix->id_offset, true, D + c0 * k,
                                    I + c0 * k, st));
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

}  // namespace imgrec
