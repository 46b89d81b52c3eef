// knn_plan.cpp — the route of a query chunk (choose_route), the launch geometry of the fused
// distance + top-k kernels and the relative error-bound coefficients of the candidate paths'
// certificate (DESIGN.md "Launch plan", "bf16 path", "Split path").  HIP-free (knn_plan.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "knn_plan.h"

namespace imgrec {

// The counts of a tiled plan whose tile (wr, wq, bm, bq) and list length are set: query blocks, row
// tiles, row splits for `target` workgroups in all, `lists` lists of km per (query, split).
static Plan tiled(Plan p, int64_t ntotal, int64_t nq, int target, int lists) {
    p.nqb = (int)((nq + p.bq - 1) / p.bq);
    p.nq_pad = p.nqb * p.bq;
    p.ntiles = (int)((ntotal + p.bm - 1) / p.bm);
    p.nsplit = std::max(1, std::min((target + p.nqb - 1) / p.nqb, p.ntiles));
    p.ncand = p.nsplit * lists * p.km;
    p.wgs = p.nqb * p.nsplit;
    return p;
}

// Fused-kernel geometry for one query chunk of the exact fp32 path.
Plan make_plan(int64_t ntotal, int64_t nq, int k, int cus) {
    Plan p{};
    p.km = fallback_km(k);
    int wg_per_cu;
    if (nq <= 32) { p.wr = 2; p.wq = 1; wg_per_cu = 3; }
    else if (nq <= 128) { p.wr = 2; p.wq = 2; wg_per_cu = 2; }
    // Two independent 4-wave workgroups per CU: their barriers do not line up, so one
    // workgroup's stage bubble is filled by the other's MFMAs (31.4 vs 32.2 ms for one 8-wave
    // (1,8) workgroup, bench config).
    else { p.wr = 1; p.wq = 4; wg_per_cu = 2; }
    p.bm = p.wr * 128; p.bq = p.wq * 32;
    return tiled(p, ntotal, nq, cus * wg_per_cu, p.wr * 2);
}

int fallback_km(int k) { return k <= 8 ? 8 : (k <= 10 ? 10 : (k <= 16 ? 16 : 32)); }

// Split-path geometry: one tile shape for every batch size ((1,4) workgroups, two per CU,
// kSplitWB row blocks per wave).
Plan make_split_plan(int64_t ntotal, int64_t nq, int kc, int cus) {
    Plan p{};
    p.km = kc; p.wr = 1; p.wq = 4;
    p.bm = p.wr * 32 * kSplitWB; p.bq = p.wq * 32;
    return tiled(p, ntotal, nq, cus * 2, p.wr * 2);
}

// Split-bf16 candidate path (knn_refine.hip): used for batches the (1,4) plan covers, k <= 16,
// rows padded to 32 floats.  K' = candidates kept per query for the exact rerank.
int split_kc(int k) { return k <= 10 ? 16 : (k <= 16 ? 32 : 0); }

// Relative error-bound coefficients of the certificate (DESIGN.md "Split path"), multiplied by
// |q| * max|x| in the kernel:
//   split dot:  3.1 * 2^-16 (dropped lo.lo / residual terms of x = hi + lo + r, |r| <= 2^-16 |x|)
//               + 1.02 * gamma_n, n = 3 MFMAs x (dp/16) steps x 5 (a 16-term tree inside each),
//               with unit roundoff 2^-23 (allows truncating accumulation);
//   rerank dot: 1.02 * gamma_n, n = 4*ceil(dp/256) + 8 fp32 FMAs + butterfly levels, u = 2^-24.
float split_coef(int dp) {
    return (float)(3.1 * std::ldexp(1.0, -16) + 1.02 * (15.0 * (dp / 16) + 16.0) * std::ldexp(1.0, -23));
}
float rerank_coef(int dp) {
    return (float)(1.02 * (4.0 * ((dp + 255) / 256) + 8.0) * std::ldexp(1.0, -24));
}

// bf16 candidate pass (one bf16 MFMA per product): the products of two bf16 values are exact in
// fp32, so the only arithmetic error besides the operand rounding (bounded in the rerank kernel
// from the stored residual norms) is the fp32 accumulation: 1.02 * gamma_n, n = (dpb/16) MFMAs x 5
// (a 16-term tree inside each) + 16, with unit roundoff 2^-23 (allows truncating accumulation),
// relative to |qh| |xh|.
float b16_acc_coef(int dpb) {
    return (float)(1.02 * (5.0 * (dpb / 16) + 16.0) * std::ldexp(1.0, -23));
}
// int8 tail of the 256 x 256 kernel: derived at knn_certify.h i8tail_e_ip
float i8t_acc_coef(int head) {
    return (float)(1.02 * (5.0 * (head / 16) + 16.0 + 3.0) * std::ldexp(1.0, -23));
}

// The int8 tail's split column H from the corpus-wide max |x| of each 64-column block: the
// smallest block boundary such that every block at or after it is within 2x of the (lower) median
// of those blocks: one scale per row then fits the whole tail, and large leading parts stay in
// bf16.  The route is off (-1) when fewer than kI8TMinTail tail columns remain or the head would be
// more than half the row.
int i8t_pick_head(const float* blkmax, int nblk) {
    for (int j = 0; j < nblk; ++j) {
        std::vector<float> v(blkmax + j, blkmax + nblk);
        std::nth_element(v.begin(), v.begin() + (v.size() - 1) / 2, v.end());
        const float med = v[(v.size() - 1) / 2];
        bool ok = true;
        for (int b = j; b < nblk && ok; ++b) ok = blkmax[b] <= 2.f * med && 2.f * blkmax[b] >= med;
        if (!ok) continue;
        const int head = 64 * j, dpb = 64 * nblk;
        return dpb - head >= kI8TMinTail && head <= dpb / 2 ? head : -1;
    }
    return -1;
}

// The joint row of the int8 tail copy (knn_plan.h): dpt bytes of codes, 2 head bytes of bf16.
int i8t_joint_row_bytes(int head, int dpt) {
    if (head < 0 || head % 64 != 0 || dpt < kI8TStageBytes || dpt % kI8TStageBytes != 0) return -1;
    return dpt + 2 * head;
}
int i8t_tail_stages(int dpt) { return dpt / kI8TStageBytes; }
int i8t_row_stages(int head, int dpt) {
    const int rb = i8t_joint_row_bytes(head, dpt);
    return rb < 0 ? -1 : rb / kI8TStageBytes;
}

// int8 small-batch pass (knn_i8.hip): per block an exact int32 dot of the row's and the query's
// codes per level (exact in fp32 as well, |D| < 2^24), the fold s_x (s_hi D_hi + s_lo D_lo) into
// the lane's accumulator (three roundings), ceil(nblk/16) blocks per lane, then the 16-lane DPP
// sum: gamma_n with n = 3 + ceil(nblk/16) + 4 — bounded here, generously, by
// 1.02 * (16 + 4 ceil(nblk/16)) u, u = 2^-23, relative to (|q| + dq)(|x~|) as the bf16 one.
float i8_acc_coef(int nblk) {
    return (float)(1.02 * (16.0 + 4.0 * ((nblk + 15) / 16)) * std::ldexp(1.0, -23));
}

// int8-path geometry: one workgroup per row split, kI8WGPCU per CU, all of the batch's queries
// in each; one folded list of km per (query, split)
// (two 4-wave workgroups per CU are resident at the kernel's 222 VGPRs; three per CU, i.e. a
// second partial round, measured faster at nq = 1 / 2: 0.366 / 0.375 vs 0.386 / 0.399 ms kernel,
// profiles/r03/i8_small_batch/sweep.jsonl; IMGREC_I8_WGPCU overrides for measurements)
// Workgroups per CU of the int8 scan: 3 from three queries, 2 for one or two (fewer lists for the
// merge, no slower a scan: profiles/r04/i8_wgpcu/), 1 for ONE query on rows of >= 24 blocks (the
// 1M x 1968 scan 0.311 -> 0.308 ms and the search 3 us shorter on two boxes, while 1M x 768 rows
// lose 28 us with one: sweep_nq1_b.txt).  IMGREC_I8_WGPCU overrides.
Plan make_i8_plan(int64_t ntotal, int64_t nq, int k, int cus, int wgpcu, int nblk) {
    const int kI8WGPCU = wgpcu > 0 ? wgpcu : (nq == 1 && nblk >= 24 ? 1 : nq <= 2 ? 2 : 3);
    Plan p{};
    p.km = b16_km(k);
    p.wr = 1; p.wq = 1; p.bm = 8;
    p.bq = (int)nq; p.nqb = 1; p.nq_pad = (int)nq;
    const int64_t groups = (ntotal + 7) / 8;
    p.ntiles = (int)groups;
    p.nsplit = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)cus * kI8WGPCU, groups));
    p.ncand = p.nsplit * p.km;
    p.wgs = p.nsplit;
    return p;
}

// per-lane list length of the generic bf16 tile (the merge floor covers what a lane list drops)
int b16_km(int k) { return k <= 16 ? 16 : 32; }

constexpr int kB16NarrowQ = 32;   // batches up to this use the 32-query tile

// bf16-path geometry: large batches with k <= 10 on the 256 x 256-tile kernel (one workgroup
// per CU, lane lists of 8 / 10); otherwise (kB16WR, kB16WQ) workgroups, kB16WGPCU per CU.
Plan make_b16_plan(int64_t ntotal, int64_t nq, int k, int cus, int dpb) {
    Plan p{};
    // (dpb bound: the 256 x 256 kernel's 32-bit lane offsets, see launch_b16_big)
    if (nq >= kB16BigMinQ && k <= 10 && dpb <= 16384) {
        p.big = true;
        p.km = k <= 8 ? 8 : 10;
        p.wr = 2; p.wq = 4;
        p.bm = kB16BigRows; p.bq = kB16BigQueries;
        p = tiled(p, ntotal, nq, cus, 1);        // lists folded to one per (query, split)
        // packed lists: split-local row index t * 256 + tile row of every tile of the largest
        // split must fit ib bits
        const int64_t groups = (ntotal + 7) / 8, cnt = (groups + p.nsplit - 1) / p.nsplit;
        const int64_t idx_max = (cnt + 31) / 32 * 256 - 1;
        int ib = 1;
        while ((int64_t{1} << ib) <= idx_max) ++ib;
        p.ib = ib <= kB16PackMaxIB ? ib : 0;
        return p;
    }
    p.km = b16_km(k);
    // batches of <= 32 queries: a 32-query tile (the (1,4) tile would pad them to 128 and spend
    // four times the matrix work of an HBM-bound search)
    const bool narrow = nq <= kB16NarrowQ;
    p.wr = narrow ? 2 : kB16WR;
    p.wq = narrow ? 1 : kB16WQ;
    p.bm = p.wr * 32 * kB16WB; p.bq = p.wq * 32;
    return tiled(p, ntotal, nq, cus * kB16WGPCU, p.wr * 2);
}

namespace {

// AUTO: the bf16 path at every corpus size.  Large batches are matrix-bound (bf16 MFMA vs fp32
// MFMA), small ones HBM-bound (the bf16 copy streams half the bytes), and on small corpora the
// exact kernel has a latency floor of its own: one 256-row tile's whole depth of fp32 MFMAs per
// workgroup, ~0.16 ms from 1000 rows up, against the candidate path's ~0.05-0.1 ms
// (profiles/r03/small_corpora/: 1000-131072 rows x nq 9-1024, bf16 1.8-2.8x faster).
// (I8 mode: batches the int8 path does not take are served as AUTO serves them)
bool b16_serves(const IndexShape& ix) {
    return ix.b16_ok && (ix.mode == KNN_SEARCH_BF16 || ix.mode == KNN_SEARCH_AUTO || ix.mode == KNN_SEARCH_I8);
}

// AUTO: batches of <= kI8AutoQ queries at every corpus size (the int8 copy streams about half of
// the bf16 copy's bytes; its dot products grow with the batch: nq <= 4 is HBM-bound, nq = 5-8
// VALU-bound and still faster than the bf16 pass; one query on 1000-65536 rows 0.05-0.075 ms
// against the exact kernel's 0.18-0.22, profiles/r03/small_corpora/)
// A row's 16-lane group in the scan has one lane per 64-element block, so narrow rows leave most
// lanes idle (d = 128: 2 of 16).  One or two queries stay HBM-bound at every width since the
// rows are compact (round 4): one query on 1M rows, int8 against bf16, 0.133 / 0.143 ms at
// d = 64, 0.134 / 0.154 at 128, 0.137 / 0.183 at 256, 0.140 / 0.221 at 384, 0.140 / 0.247 at 512
// (profiles/r05/small_d/), so they take the int8 path at any width.  Larger batches multiply the
// dot products per byte: below kI8MinBlocks blocks they take it only while the copy is small
// enough (<= 64 MB, ~10 us of streaming) for the fixed costs to decide.
constexpr int kI8AutoQ = 8;
constexpr int kI8MinBlocks = 8;
// 5-8 queries run the scan's 8-query instance, VALU-bound: its time steps with the blocks per
// lane (NBI = ceil(blocks / 16)), the bf16 pass's grows with d.  One box, 1M rows
// (profiles/r05/modes_nq/, small_d/): 8 queries int8 / bf16 0.355 / 0.326 ms at 12 blocks,
// 0.339 / 0.397 at 16, 0.530 / 0.496 at 20, 0.585 / 0.679 at 31 — the int8 route at 14-16 blocks
// and from 23
bool i8_wins_8q(int nblk) { return (nblk >= 14 && nblk <= 16) || nblk >= 23; }
constexpr int64_t kI8SmallCopyBytes = 64ll << 20;
bool i8_serves(const IndexShape& ix, int64_t nq) {
    if (ix.nblk8 <= 0 || nq > kI8MaxQ) return false;
    if (ix.mode == KNN_SEARCH_I8) return true;
    if (ix.mode != KNN_SEARCH_AUTO || nq > kI8AutoQ) return false;
    const int64_t i8_row = i8_row_bytes(ix.nblk8) + 4 * ix.nblk8;
    const bool wide_enough = nq <= 2 ? true : nq <= 4 ? ix.nblk8 >= kI8MinBlocks : i8_wins_8q(ix.nblk8);
    return !ix.b16_ok || wide_enough || ix.ntotal * i8_row <= kI8SmallCopyBytes;
}

bool split_serves(const IndexShape& ix, int64_t nq, int k) {
    if (!ix.split_ok || ix.mode == KNN_SEARCH_EXACT || split_kc(k) == 0) return false;
    if (ix.mode == KNN_SEARCH_SPLIT) return true;
    // auto (when the bf16 path is unavailable): batches the (1,4) plan covers, corpora with
    // enough rows to amortise the rerank
    return (ix.mode == KNN_SEARCH_AUTO || ix.mode == KNN_SEARCH_I8) && nq > 128 && ix.ntotal >= 16384;
}

}  // namespace

RoutePlan choose_route(const IndexShape& ix, int64_t nq, int k) {
    RoutePlan r{};
    const bool cand = k <= KNN_MAX_K;      // (larger k: the exact plan, as knn_plan reports it)
    if (cand && i8_serves(ix, nq)) {
        r.route = Route::I8;
        r.plan = make_i8_plan(ix.ntotal, nq, k, ix.cus, ix.i8_wgpcu, ix.nblk8);
        r.i8_inst = nq <= 2 ? (int)nq : (nq <= 4 ? 4 : 8);
    } else if (cand && b16_serves(ix)) {
        r.route = Route::B16;
        r.plan = make_b16_plan(ix.ntotal, nq, k, ix.cus, ix.dpb);
        // The 256 x 256 kernel's int8 tail: AUTO and the i8 mode, on the big plan, unless the knob
        // turned it off at creation or the index turned out not to be eligible (ensure_i8tail;
        // dpb <= 4096: the fused query prep writes the query side).  search_mode = "bf16" stays the
        // pure bf16 pass.
        r.tail_ok = r.plan.big && ix.i8tail && ix.xt_state != TailCopy::Ineligible && ix.dpb <= 4096 &&
                    ix.ntotal > 0 && (ix.mode == KNN_SEARCH_AUTO || ix.mode == KNN_SEARCH_I8);
    } else if (split_serves(ix, nq, k)) {
        r.route = Route::Split;
        r.plan = make_split_plan(ix.ntotal, nq, split_kc(k), ix.cus);
    } else {
        r.route = Route::Exact;
        r.plan = make_plan(ix.ntotal, nq, k, ix.cus);
    }
    return r;
}

}  // namespace imgrec
