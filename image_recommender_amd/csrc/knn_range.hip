// knn_range.hip — range search (faiss Index::range_search): every stored row within a radius of
// each query, in one pass over the corpus that writes only what passes.
//
// Pipeline of one query chunk (range_search_locked):
//   1. knn_range_tile_kernel: the exact fp32 contraction and key forming of the tile core
//      (knn_tile.h: v_mfma_f32_32x32x2_f32, LDS-DMA ring; key (|q|^2 + |x|^2) - 2 q.x clamped at 0,
//      or -q.x) over contiguous row tiles; the epilogue tests `key < r` (r = -radius for IP) and
//      appends the survivors to a buffer: per 32-row block a wave counts its lanes' survivors,
//      reserves their slots with ONE returning agent-scope atomic and every lane stores its
//      (key bits << 32 | row, query) entries with plain stores.  Per-query hit counts are kept in
//      a register over the whole row split and added once per lane pair at the end.
//   2. range_scan_kernel: exclusive scan of the counts -> segment offsets and `lims`.
//   3. the chunk's total reaches the host (the one wait): the result is allocated; a total past
//      the append buffer's capacity grows the buffer and runs step 1 again (the counts and the
//      total were complete; the entries were not).
//   4. range_scatter_kernel: entries into their query's segment (one atomic per run of
//      consecutive entries of one query).
//   5. sort_u64_segments (knn_hugek.hip): every segment into (key, row) order.
//   6. range_unpack_kernel: D (IP sign restored) and I (row + id_offset).
//
// Arithmetic: a pair's key depends on (q, x, d, metric) only.  The depth order of the MFMA chain
// is fixed by the stage depth, which is chosen from the row stride alone (32 when it divides, 16
// otherwise); the two geometries (256 rows x 32 queries for batches of <= 32, 128 x 128 beyond)
// share it: an MFMA output element depends on its own row and column only.  So results are
// bitwise independent of N, the batch, the append capacity and the sharding.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "knn_index.h"
#include "knn_tile.h"
#include "wave_ops.h"

namespace imgrec {
namespace {

struct RangeArgs {
    const float* xb;            // corpus, rows padded to 256, stride dp
    const float* xnorm;
    uint32_t nrows;
    int dp;
    const float* qp;            // nqb x BQ padded queries
    const float* qnorm;
    int nq, metric;             // metric 1 = L2, otherwise inner product
    float r;                    // a pair passes when key < r
    int ntiles, nsplit, nqb;
    uint64_t* ent;              // append buffer: key bits << 32 | row ...
    uint32_t* entq;             // ... and the chunk-local query of each entry
    unsigned long long cap;     // entries the buffer holds
    unsigned long long* total;  // survivors of the chunk (counted past cap as well)
    uint32_t* counts;           // per query
};

template <int WR, int WQ, int NS, int BK>
__global__ void __launch_bounds__(WR * WQ * 64, (TileGeom<WR, WQ, NS, BK>::MIN_WAVES))
knn_range_tile_kernel(const RangeArgs a) {
    using G = TileGeom<WR, WQ, NS, BK>;
    constexpr int WB = G::WB, RW = G::RW, NW = G::NW, BM = G::BM, BQ = G::BQ, STAGE = G::STAGE;
    constexpr int LPW = G::LPW;
    __shared__ __attribute__((aligned(16))) float smem[G::LDS_FLOATS];
    const int wgid = xcd_wgid();                 // block -> (query block, row split)
    const int nqb = a.nqb, nsplit = a.nsplit, dp = a.dp;
    if (wgid >= nqb * nsplit) return;
    float* const norm_base = smem + NS * STAGE;
    const int qb = wgid % nqb;
    const int split = wgid / nqb;
    const int t1 = split < a.ntiles ? (a.ntiles - split + nsplit - 1) / nsplit : 0;
    auto tile = [&](int j) { return split + j * nsplit; };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const TileLanes<G> L(lane, wave);
    const int wr = L.wr, lh = L.lh;
    const int qcol = qb * BQ + L.wq * 32 + L.li; // < nq_pad
    const bool qvalid = qcol < a.nq;
    const int metric = a.metric;
    const float rad = a.r;
    float qn = (metric == 1) ? a.qnorm[qcol] : 0.f;
    asm volatile("" : "+v"(qn));

    const int nsteps = dp / BK;
    const float* qbase = a.qp + (size_t)qb * BQ * dp;

    int64_t poff[LPW];                           // this lane's source of piece j (TileLanes)
#pragma unroll
    for (int j = 0; j < LPW; ++j) poff[j] = L.poff(j, dp);
    const uint32_t smem_u32 = lds_u32(smem);
    const uint32_t norm_u32 = lds_u32(norm_base);
    int it = 0, is = 0, ibuf = 0;
    const float* itile = a.xb + (size_t)tile(0) * BM * dp;
    auto issue_next = [&]() __attribute__((always_inline)) {
        if (it >= t1) return;
        const uint32_t st = smem_u32 + (uint32_t)(ibuf * STAGE) * 4u;
        if (is == 0) {
            for (int j = wave; j < BM / 64; j += NW)
                dma4_norm(a.xnorm + (size_t)tile(it) * BM + j * 64 + lane,
                          norm_u32 + (uint32_t)((it % NS) * BM + j * 64) * 4u);
        }
        const int k0 = is * BK;
#pragma unroll
        for (int j = 0; j < LPW; ++j) dma16((L.is_a(j) ? itile : qbase) + poff[j] + k0, st + L.pdst(j));
        if (++is == nsteps) { is = 0; ++it; itile += (size_t)nsplit * BM * dp; }
        ibuf = (ibuf + 1 == NS) ? 0 : ibuf + 1;
    };

#pragma unroll
    for (int j = 0; j < NS - 1; ++j) issue_next();
    int remaining = t1 * nsteps;
    int cbuf = 0;
    int nhits = 0;                               // this lane's survivors over the whole split

    for (int t = 0; t < t1; ++t) {
        const uint32_t row0 = (uint32_t)tile(t) * BM;
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

        // ---- epilogue: threshold and append.  The tile's norms landed before its first stage's
        // barrier; their ring slot is rewritten NS tiles later, behind a barrier every wave
        // reaches only after this epilogue.
        const float* nrm = norm_base + (t % NS) * BM;
#pragma unroll
        for (int b = 0; b < WB; ++b) {
            float key[16];
            const int rb = wr * RW + b * 32 + 4 * lh;          // row of accumulator reg 0
            const unsigned mask = tile_keys(acc[b], nrm, rb, metric, qn, key, [&](int off, float kv) __attribute__((always_inline)) {
                return qvalid && (row0 + (uint32_t)(rb + off) < a.nrows) && kv < rad;
            });
            if (__any(mask != 0)) {                            // wave-uniform: all lanes inside
                const int cnt = __popc(mask);
                const int ex = wave_excl_scan_i32(cnt);
                const int tot = wave_sum_i32(cnt);
                unsigned long long base = 0;
                if (lane == 0)
                    base = __hip_atomic_fetch_add(a.total, (unsigned long long)tot, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
                unsigned long long slot = (((unsigned long long)bhi << 32) | blo) + (unsigned)ex;
                nhits += cnt;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if ((mask >> r) & 1u) {
                        if (slot < a.cap) {
                            const uint32_t row = row0 + (uint32_t)(rb + (r & 3) + 8 * (r >> 2));
                            a.ent[slot] = ((uint64_t)key_bits_ordered(key[r]) << 32) | row;
                            a.entq[slot] = (uint32_t)qcol;
                        }
                        ++slot;
                    }
                }
            }
        }
    }

    // the two lanes of a query (its rows' halves) add their count once
    const int both = nhits + __shfl_xor(nhits, 32, 64);
    if (lh == 0 && qvalid && both > 0)
        __hip_atomic_fetch_add(a.counts + qcol, (uint32_t)both, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Exclusive scan of a chunk's counts (nqc <= kQueryChunk): off[i] and cur[i] = the start of query
// i's segment (i <= nqc: off[nqc] = the total), lims[i] = base + off[i].  One 256-thread workgroup.
__global__ void __launch_bounds__(256)
range_scan_kernel(const uint32_t* __restrict__ counts, int nqc, int64_t base, uint32_t* __restrict__ off,
                  uint32_t* __restrict__ cur, int64_t* __restrict__ lims) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t tot;
    const int t = threadIdx.x;
    const int per = (nqc + 255) / 256;
    const int i0 = t * per, i1 = min(nqc, i0 + per);
    uint32_t s = 0;
    for (int i = i0; i < i1; ++i) s += counts[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int j = 0; j < 256; ++j) { const uint32_t v = part[j]; part[j] = run; run += v; }
        tot = run;
    }
    __syncthreads();
    uint32_t run = part[t];
    for (int i = i0; i < i1; ++i) {
        off[i] = run; cur[i] = run; lims[i] = base + (int64_t)run;
        run += counts[i];
    }
    if (t == 0) { off[nqc] = tot; cur[nqc] = tot; lims[nqc] = base + (int64_t)tot; }
}

// Entry e of the append buffer -> its query's segment.  A run of consecutive entries of one query
// inside a wave (a lane's survivors of a block are consecutive) takes one atomic for the run.
__global__ void __launch_bounds__(256)
range_scatter_kernel(const uint64_t* __restrict__ ent, const uint32_t* __restrict__ entq, int64_t total,
                     uint32_t* __restrict__ cur, uint64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = e < total;
    const uint32_t q = valid ? entq[e] : 0xffffffffu;
    const uint64_t v = valid ? ent[e] : 0;
    const uint32_t qprev = (uint32_t)__shfl_up((int)q, 1, 64);
    const bool head = valid && (lane == 0 || qprev != q);
    const uint64_t heads = __ballot(head);
    const int nvalid = __popcll(__ballot(valid));              // valid lanes are a prefix
    // this lane's run: from the last head at or below it to the next head (or the valid end)
    const uint64_t below = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
    const int h = below ? 63 - __builtin_clzll(below) : 0;
    const uint64_t above = h == 63 ? 0ull : heads >> (h + 1);
    const int next = above ? h + 1 + __builtin_ctzll(above) : nvalid;
    uint32_t base = 0;
    if (head) base = __hip_atomic_fetch_add(cur + q, (uint32_t)(next - h), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
    base = (uint32_t)__shfl((int)base, h, 64);
    if (valid) out[(size_t)base + (uint32_t)(lane - h)] = v;
}

__global__ void __launch_bounds__(256)
range_unpack_kernel(const uint64_t* __restrict__ sorted, int64_t total, int metric, int64_t id_offset,
                    float* __restrict__ D, int64_t* __restrict__ I) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const uint64_t x = sorted[e];
    const float key = key_from_ordered((uint32_t)(x >> 32));
    D[e] = metric == 1 ? key : -key;
    I[e] = (int64_t)(uint32_t)x + id_offset;
}

hipError_t launch_range_tile(const TilePlan& p, const RangeArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)(p.nqb * p.nsplit));
    with_tile_ring(p, [&](auto g) {
        using G = decltype(g);
        hipLaunchKernelGGL((knn_range_tile_kernel<G::WR, G::WQ, G::NS, G::BK>), grid, dim3(G::NT), 0, st, a);
    });
    return hipGetLastError();
}

int new_result(int device, int64_t nq, knn_range_result** out) {
    knn_range_result* r = new knn_range_result();
    r->device = device;
    r->nq = nq;
    *out = r;
    KNN_HIP(hipEventCreateWithFlags(&r->done, hipEventDisableTiming));
    return r->lims.reserve((size_t)(nq + 1));
}

// D / I of `n` entries (never NULL: an empty result keeps one unused element)
int alloc_hits(int64_t n, DevBuf<float>& D, DevBuf<int64_t>& I) {
    const int rc = D.reserve((size_t)std::max<int64_t>(n, 1));
    return rc != KNN_OK ? rc : I.reserve((size_t)std::max<int64_t>(n, 1));
}

struct ChunkHits { DevBuf<float> D; DevBuf<int64_t> I; int64_t n = 0; };

int range_chunks(knn_index* ix, const float* q, int64_t nq, float radius, hipStream_t st,
                 knn_range_result* res, std::vector<ChunkHits>& chunks) {
    const int kmetric = ix->metric == KNN_METRIC_L2 ? 1 : 0;
    const int normalize = ix->metric == KNN_METRIC_COSINE;
    int rc;
    if ((rc = ix->rg_total_h.reserve(1)) != KNN_OK) return rc;
    if ((rc = ix->rg_total.reserve((size_t)1)) != KNN_OK) return rc;
    int64_t base = 0;
    for (int64_t c0 = 0; c0 < nq; c0 += kQueryChunk) {
        const int64_t cn = std::min(kQueryChunk, nq - c0);
        const TilePlan p = make_tile_plan(ix->ntotal, cn, ix->dp, ix->cus);
        if ((rc = ix->qpad.reserve((size_t)p.nq_pad * ix->dp)) != KNN_OK) return rc;
        if ((rc = ix->qnorm.reserve((size_t)p.nq_pad)) != KNN_OK) return rc;
        if ((rc = ix->rg_cnt.reserve((size_t)cn)) != KNN_OK) return rc;
        if ((rc = ix->rg_off.reserve((size_t)cn + 1)) != KNN_OK) return rc;
        if ((rc = ix->rg_cur.reserve((size_t)cn + 1)) != KNN_OK) return rc;
        if ((rc = ix->rg_ent.reserve(ix->range_cap0)) != KNN_OK) return rc;
        if ((rc = ix->rg_entq.reserve(ix->range_cap0)) != KNN_OK) return rc;
        KNN_HIP(launch_rows_ingest(q + c0 * ix->d, cn, ix->d, ix->dp, p.nq_pad, normalize, ix->qpad,
                                   ix->qnorm, st));
        RangeArgs a{};
        a.xb = ix->xb; a.xnorm = ix->xn; a.nrows = (uint32_t)ix->ntotal; a.dp = ix->dp;
        a.qp = ix->qpad; a.qnorm = ix->qnorm; a.nq = (int)cn; a.metric = kmetric;
        a.r = kmetric ? radius : -radius;
        a.ntiles = p.ntiles; a.nsplit = p.nsplit; a.nqb = p.nqb;
        a.total = ix->rg_total; a.counts = ix->rg_cnt;
        auto pass = [&]() -> int {
            a.ent = ix->rg_ent; a.entq = ix->rg_entq;
            a.cap = (unsigned long long)std::min(ix->rg_ent.cap(), ix->rg_entq.cap());
            KNN_HIP(hipMemsetAsync(ix->rg_total, 0, sizeof(unsigned long long), st));
            KNN_HIP(hipMemsetAsync(ix->rg_cnt, 0, (size_t)cn * sizeof(uint32_t), st));
            hipEvent_t e1 = nullptr;              // knn_set_timing: the tile kernel's own time
            int rc2;
            if ((rc2 = timed_begin(ix, st, &e1)) != KNN_OK) return rc2;
            KNN_HIP(launch_range_tile(p, a, st));
            if (e1) KNN_HIP(hipEventRecord(e1, st));
            hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(256), 0, st, ix->rg_cnt, (int)cn, base,
                               ix->rg_off, ix->rg_cur, res->lims + c0);
            KNN_HIP(hipGetLastError());
            return KNN_OK;
        };
        if ((rc = pass()) != KNN_OK) return rc;
        KNN_HIP(hipMemcpyAsync(ix->rg_total_h, ix->rg_total, sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, st));
        KNN_HIP(hipStreamSynchronize(st));
        const unsigned long long total = *ix->rg_total_h;
        if (total > (unsigned long long)UINT32_MAX)
            KNN_FAIL(KNN_EINVAL, "range search: %llu hits in one chunk of %lld queries (limit 2^32 - 1): "
                     "lower the radius or split the batch", total, (long long)cn);
        chunks.emplace_back();
        chunks.back().n = (int64_t)total;
        if ((rc = alloc_hits((int64_t)total, chunks.back().D, chunks.back().I)) != KNN_OK) return rc;
        if (total > 0) {
            if (total > a.cap) {
                // the counts were complete, the entries were not: the same pass with room for all
                if ((rc = ix->rg_ent.reserve((size_t)total)) != KNN_OK) return rc;
                if ((rc = ix->rg_entq.reserve((size_t)total)) != KNN_OK) return rc;
                if ((rc = pass()) != KNN_OK) return rc;
            }
            if ((rc = ix->rg_seg.reserve((size_t)total)) != KNN_OK) return rc;
            const unsigned blocks = (unsigned)((total + 255) / 256);
            hipLaunchKernelGGL(range_scatter_kernel, dim3(blocks), dim3(256), 0, st, ix->rg_ent, ix->rg_entq,
                               (int64_t)total, ix->rg_cur, ix->rg_seg);
            KNN_HIP(hipGetLastError());
            // sorted segments land back in the append buffer (its capacity covers the total)
            KNN_HIP(sort_u64_segments(ix->rg_seg, ix->rg_ent, (int64_t)total, (int)cn, ix->rg_off, 64u,
                                      ix->hk_tmp, st));
            hipLaunchKernelGGL(range_unpack_kernel, dim3(blocks), dim3(256), 0, st, ix->rg_ent, (int64_t)total,
                               kmetric, ix->id_offset, chunks.back().D, chunks.back().I);
            KNN_HIP(hipGetLastError());
        }
        base += (int64_t)total;
    }
    return KNN_OK;
}

}  // namespace

int range_search_locked(knn_index* ix, const float* q, int64_t nq, float radius, hipStream_t st,
                        knn_range_result** out) {
    *out = nullptr;
    if (ix->ntotal > (int64_t)UINT32_MAX)
        KNN_FAIL(KNN_EINVAL, "range search: %lld rows in one shard (limit 2^32 - 1): split the index "
                 "over more shards", (long long)ix->ntotal);
    knn_range_result* res = nullptr;
    int rc = new_result(ix->device, nq, &res);
    std::vector<ChunkHits> chunks;
    const bool l2 = ix->metric == KNN_METRIC_L2;
    if (rc == KNN_OK) {
        if (ix->ntotal == 0 || nq == 0 || (l2 && radius <= 0.f)) {
            const hipError_t e = hipMemsetAsync(res->lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st);
            if (e != hipSuccess) { set_err("hipMemsetAsync failed: %s", hipGetErrorString(e)); rc = KNN_EHIP; }
        } else {
            rc = range_chunks(ix, q, nq, radius, st, res, chunks);
        }
    }
    if (rc == KNN_OK) {
        int64_t size = 0;
        for (const ChunkHits& c : chunks) size += c.n;
        res->size = size;
        if (chunks.size() == 1) {
            res->D = std::move(chunks[0].D);
            res->I = std::move(chunks[0].I);
            chunks.clear();
        } else if ((rc = alloc_hits(size, res->D, res->I)) == KNN_OK) {
            int64_t at = 0;
            for (const ChunkHits& c : chunks) {
                if (c.n == 0) continue;
                hipError_t e = hipMemcpyAsync(res->D + at, c.D, (size_t)c.n * sizeof(float), hipMemcpyDeviceToDevice, st);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(res->I + at, c.I, (size_t)c.n * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) { set_err("hipMemcpyAsync failed: %s", hipGetErrorString(e)); rc = KNN_EHIP; break; }
                at += c.n;
            }
            if (rc == KNN_OK && !chunks.empty() && hipStreamSynchronize(st) != hipSuccess) {
                set_err("hipStreamSynchronize failed");
                rc = KNN_EHIP;
            }
        }
    }
    if (rc == KNN_OK && hipEventRecord(res->done, st) != hipSuccess) {
        set_err("hipEventRecord failed");
        rc = KNN_EHIP;
    }
    chunks.clear();
    if (rc != KNN_OK) {
        (void)hipStreamSynchronize(st);          // nothing in flight may still write the buffers
        range_result_free(res);
        return rc;
    }
    *out = res;
    return KNN_OK;
}

int range_result_from_host(int device, int64_t nq, const int64_t* lims, const float* D, const int64_t* I,
                           hipStream_t st, knn_range_result** out) {
    *out = nullptr;
    knn_range_result* res = nullptr;
    int rc = new_result(device, nq, &res);
    const int64_t size = lims[nq];
    if (rc == KNN_OK) rc = alloc_hits(size, res->D, res->I);
    if (rc == KNN_OK) {
        res->size = size;
        hipError_t e = hipMemcpyAsync(res->lims, lims, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && size > 0)
            e = hipMemcpyAsync(res->D, D, (size_t)size * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && size > 0)
            e = hipMemcpyAsync(res->I, I, (size_t)size * sizeof(int64_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);     // the host arrays are the caller's
        if (e == hipSuccess) e = hipEventRecord(res->done, st);
        if (e != hipSuccess) { set_err("range result upload failed: %s", hipGetErrorString(e)); rc = KNN_EHIP; }
    }
    if (rc != KNN_OK) {
        range_result_free(res);
        return rc;
    }
    *out = res;
    return KNN_OK;
}

void range_result_free(knn_range_result* r) {
    if (!r) return;
    DeviceGuard g(r->device);
    if (r->done) {
        (void)hipEventSynchronize(r->done);
        (void)hipEventDestroy(r->done);
    }
    delete r;                            // (its buffers, while the guard holds)
}

}  // namespace imgrec
