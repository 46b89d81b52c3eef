// knn_search.cpp — the three search arithmetics of one k-NN index and their device-side
// certificate handling (DESIGN.md "Kernels"):
//
//   exact   the fused fp32 MFMA distance + top-k kernel, then the list merge;
//   bf16    bf16 candidate pass (one bf16 MFMA per product) -> candidate merge (top K' = 64 +
//           list floor) -> fp32 rerank + certificate, with a second chance over every per-split
//           list entry for queries the first certificate cannot settle;
//   split   split-bf16 candidate pass (three bf16 MFMAs per product) -> merge -> rerank +
//           certificate (+ second chance).
//
// Queries no certificate settles are re-run exactly inside the certificate tail kernel, planned on
// the device: the count never travels to the host, so knn_search_device enqueues a whole search
// without waiting for the GPU.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "knn_index.h"

namespace imgrec {

// Timing events around the dominant (fused) kernel launch of a chunk.
int timed_begin(knn_index* ix, hipStream_t st, hipEvent_t* e1) {
    *e1 = nullptr;
    if (!ix->timing) return KNN_OK;
    if (ix->ev_used + 2 > ix->ev.size()) {
        for (int i = 0; i < 64; ++i) {
            hipEvent_t e;
            KNN_HIP(hipEventCreate(&e));
            ix->ev.push_back(e);
        }
    }
    KNN_HIP(hipEventRecord(ix->ev[ix->ev_used], st));
    *e1 = ix->ev[ix->ev_used + 1];
    ix->ev_used += 2;
    return KNN_OK;
}

namespace {

// 1 = L2, 0 = inner product (cosine rows are normalised): the kernels' metric argument
int kmetric_of(const knn_index* ix) { return ix->metric == KNN_METRIC_L2 ? 1 : 0; }

// A chunk's dominant launch between the two events of a timing pair (knn_kernel_time: one a chunk).
#define KNN_TIMED(ix, st, launch)                                          \
    do {                                                                   \
        hipEvent_t e1_ = nullptr;                                          \
        if (const int rc_ = timed_begin(ix, st, &e1_)) return rc_;         \
        KNN_HIP(launch);                                                   \
        if (e1_) KNN_HIP(hipEventRecord(e1_, st));                         \
    } while (0)

// Exact fp32 path over nq padded queries (qpad holds p.nq_pad zero-padded rows).
int exact_chunk(knn_index* ix, const Plan& p, const float* qpad, const float* qnorm, int64_t nq, int k,
                float* D, int64_t* I, hipStream_t st) {
    const int kmetric = kmetric_of(ix);
    int rc;
    if (stream_lists_ok(ix, nq)) {
        // <= 4 queries: the corpus streamed once (HBM-bound) into exact lists of 32 per row
        // split, merged — instead of 32-query fp32 MFMA tiles that compute 28-31 padding queries
        // (d = 48 colour-only or d = 1968 exact mode, one query on 1M rows; profiles/r05/stream/)
        const int sp = stream_splits(ix);
        const size_t nc = (size_t)sp * KNN_MAX_K;
        if ((rc = ix->cand_d.reserve((size_t)nq * nc)) != KNN_OK) return rc;
        if ((rc = ix->cand_i.reserve((size_t)nq * nc)) != KNN_OK) return rc;
        KNN_TIMED(ix, st, launch_stream_lists(ix, qpad, qnorm, nq, kmetric, sp, ix->cand_d, ix->cand_i, st));
        KNN_HIP(launch_merge(ix->cand_d, ix->cand_i, nq, sp, KNN_MAX_K, (int64_t)nc, KNN_MAX_K, k,
                             kmetric, 0, D, I, st));
        return KNN_OK;
    }
    if ((rc = ix->cand_d.reserve((size_t)nq * p.ncand)) != KNN_OK) return rc;
    if ((rc = ix->cand_i.reserve((size_t)nq * p.ncand)) != KNN_OK) return rc;
    TileArgs a{};
    a.wr = p.wr; a.wq = p.wq; a.km = p.km;
    a.xb = ix->xb; a.xnorm = ix->xn; a.nrows = (int)ix->ntotal; a.dp = ix->dp;
    a.qp = qpad; a.qnorm = qnorm; a.nq = (int)nq; a.metric = kmetric;
    a.ntiles = p.ntiles; a.nsplit = p.nsplit; a.nqb = p.nqb; a.id_offset = ix->id_offset;
    a.cand_d = ix->cand_d; a.cand_i = ix->cand_i; a.ncand = p.ncand; a.mode = kModeF32;
    KNN_TIMED(ix, st, launch_tile_topk(a, st));
    KNN_HIP(launch_merge(ix->cand_d, ix->cand_i, nq, p.ncand / p.km, p.km, p.ncand, p.km, k,
                         kmetric, 0, D, I, st));
    return KNN_OK;
}

// max |x|^2 (and max bf16 residual) over the stored rows, recomputed after rows change
int refresh_maxima(knn_index* ix, hipStream_t st) {
    if (!ix->xn_max_stale) return KNN_OK;
    int rc;
    if ((rc = ix->xn_max.reserve(1)) != KNN_OK) return rc;
    KNN_HIP(launch_max_norm(ix->xn, ix->ntotal, ix->xn_max, st));
    if (ix->b16_ok) {
        if ((rc = ix->xr_max.reserve(1)) != KNN_OK) return rc;
        KNN_HIP(launch_max_norm(ix->xr, ix->ntotal, ix->xr_max, st));
    }
    if (ix->x8) {
        if ((rc = ix->x8r_max.reserve(1)) != KNN_OK) return rc;
        KNN_HIP(launch_max_norm(ix->x8r, ix->ntotal, ix->x8r_max, st));
    }
    if (ix->xt) {        // the int8 tail copy: R_t, R_h, X_t, X_h
        if ((rc = ix->xt_max.reserve(4)) != KNN_OK) return rc;
        KNN_HIP(launch_i8tail_max(ix->xtm, ix->ntotal, ix->xt_max, st));
    }
    ix->xn_max_stale = false;
    return KNN_OK;
}

// Certificate counters (two chunk parities + per-search totals, zeroed once here; the fallback
// prep kernel folds and re-zeroes them) and the uncertified-query list.
int grow_stats(knn_index* ix, int64_t nq, hipStream_t st) {
    int rc;
    if (!ix->stat) {
        if ((rc = ix->stat.reserve(12)) != KNN_OK) return rc;
        KNN_HIP(hipMemsetAsync(ix->stat, 0, 12 * sizeof(int), st));
        ix->stat_seq = 0;
    }
    if ((rc = ix->fail.reserve((size_t)nq)) != KNN_OK) return rc;
    return ix->chance.reserve((size_t)nq);
}

// The rerank + certificate of a candidate chunk, then its whole tail in ONE launch
// (cert_tail_kernel: second chance, stats fold, and the exact fp32 re-run of the queries neither
// certificate settles — planned on the device, so the host never waits).  With every query
// certified the tail is one near-empty launch.
int certify_chunk(knn_index* ix, RerankArgs& r, const float* qpad, const float* qnorm, int64_t nq,
                  int k, float* D, int64_t* I, hipStream_t st, bool first) {
    const int parity = ix->stat_seq & 1;
    const int km = fallback_km(k);
    const int grid = kTailWGPerCU * ix->cus;
    const int64_t cap_rows = round_up(nq, 32);
    const int bm = 128 * kFallbackWR;
    const int lists_km = 2 * kFallbackWR * km;
    // candidate lists of the exact re-run: nqb query blocks x nsplit = max(1, grid / nqb) row
    // splits, lists_km entries per (query, split).  nqb * nsplit <= grid while nqb <= grid; past
    // that (more than 32 x grid uncertified queries: a device with fewer CUs) nsplit = 1 and the
    // lists need cap_rows x lists_km (sizing by the grid alone overflowed there)
    const size_t ncap = (size_t)std::max<int64_t>(grid, cap_rows / 32) * 32 * lists_km;
    int rc;
    if ((rc = ix->fb_q.reserve((size_t)cap_rows * ix->dp)) != KNN_OK) return rc;
    if ((rc = ix->fb_qn.reserve((size_t)cap_rows)) != KNN_OK) return rc;
    if ((rc = ix->fb_cd.reserve(ncap)) != KNN_OK) return rc;
    if ((rc = ix->fb_ci.reserve(ncap)) != KNN_OK) return rc;
    if ((rc = ix->tail_ctl.reserve((size_t)4 + cap_rows / 32)) != KNN_OK) return rc;
    r.stats = ix->stat + 4 * parity;
    r.fail_list = ix->fail;
    r.chance_list = ix->chance;
    if (r.raw_d) {
        // sliced second chance: up to 64 slices per item (profiles/r03/second_chance/)
        static const int kSlices = [] {           // IMGREC_SC_SLICES overrides (measurements)
            const char* e = std::getenv("IMGREC_SC_SLICES");
            const int v = e ? std::atoi(e) : 0;
            return v > 0 ? v : 64;
        }();
        // (<= 64: the last slice's merge reads the slice heads from the lanes of one wave;
        // S k <= 1024 = kWideCap, knn_certify.h: it stages the S lists of k in LDS)
        r.sc_slices = std::max(1, std::min({kSlices, 64, r.raw_lists, 1024 / k}));
        const size_t ns = (size_t)nq * r.sc_slices * k;
        if ((rc = ix->sc_key.reserve(ns)) != KNN_OK) return rc;
        if ((rc = ix->sc_lab.reserve(ns)) != KNN_OK) return rc;
        if ((rc = ix->sc_meta.reserve((size_t)nq * r.sc_slices * 4)) != KNN_OK) return rc;
        const size_t c0 = ix->sc_done.cap();
        if ((rc = ix->sc_done.reserve((size_t)nq)) != KNN_OK) return rc;
        if (ix->sc_done.cap() != c0)      // (re)allocated: the self-resetting counters start at 0
            KNN_HIP(hipMemsetAsync(ix->sc_done, 0, ix->sc_done.cap() * sizeof(int), st));
        r.sc_key = ix->sc_key; r.sc_lab = ix->sc_lab; r.sc_meta = ix->sc_meta; r.sc_done = ix->sc_done;
    }
    r.tail_ctl = ix->tail_ctl;
    // (small batches only: a large batch's rerank is throughput-bound and its second chances
    // queue up in the tail; at 1024 queries the A/B was within the +-15 us noise of the step,
    // profiles/r04/chance_skip/ab_env_nq1024*.txt, so large batches keep the round-3 route)
    r.chance_skip = ix->chance_skip && r.raw_d && nq <= ix->cus ? 1 : 0;
    // first rerank phase of k rows for batches past one rerank workgroup per CU
    // (IMGREC_RERANK_P1: 0 keeps 16 everywhere, for A/B)
    r.p1 = ix->rerank_p1k && nq > ix->cus ? k : 0;
    // 4-wave rerank workgroups past one per CU (four resident per CU, one round for 1024 queries):
    // opt-in (IMGREC_RERANK_NW4=1) — measured 3-4 us slower per 125k-row step than 8 waves, the
    // rerank is not residency-bound (profiles/r05/rerank_nw4_ab/)
    r.nw = ix->rerank_nw4 && nq > ix->cus && r.l1_G == 0 && r.s_lists == 0 && !r.chance_skip ? 4 : 0;
    if (!r.direct) KNN_HIP(launch_rerank_certify(r, st));
    TailArgs t{};
    t.r = r;
    t.parity = parity;
    t.first = first ? 1 : 0;
    t.stat = ix->stat;
    t.qpad = qpad;
    t.qnorm = qnorm;
    t.dp = ix->dp;
    t.nrows = (int)ix->ntotal;
    t.ntiles = (int)((ix->ntotal + bm - 1) / bm);
    t.metric = kmetric_of(ix);
    t.xb = ix->xb;
    t.xn = ix->xn;
    t.id_offset = ix->id_offset;
    t.fq = ix->fb_q;
    t.fqn = ix->fb_qn;
    t.fcd = ix->fb_cd;
    t.fci = ix->fb_ci;
    t.ticket = ix->tail_ctl + 4;
    t.km = km;
    t.lists_km = lists_km;
    const hipError_t e = launch_cert_tail(t, grid, st);
    if (e != hipSuccess) {        // the parities may hold this chunk's counts: start clean
        (void)hipMemsetAsync(ix->stat, 0, 12 * sizeof(int), st);
        ix->stat_seq = 0;
        KNN_FAIL(KNN_EHIP, "certificate tail launch failed: %s", hipGetErrorString(e));
    }
    ++ix->stat_seq;
    ix->stat_valid = true;
    ix->last_split_queries += nq;
    return KNN_OK;
}

// The candidate merge's second level inside the rerank kernel (one launch fewer: ~10 us at
// nq = 1, where it is one wave's select behind a kernel boundary) while the batch leaves the rerank
// at most one workgroup per CU; larger batches keep the separate level-2 launch (its 4-wave blocks
// do not idle seven waves of each rerank workgroup behind the select).  IMGREC_MERGE_FUSE=0 at
// index creation: off.
bool fuse_merge_level2(const knn_index* ix, int64_t nq) {
    return ix->merge_fuse && nq <= ix->cus;
}

// Both merge levels inside the rerank (RerankArgs::l0_lists): small batches whose merge would
// take two levels of 16-entry lists with at most one group of 64 lists per rerank wave — no merge
// launch at all (the level-1 launch was ~9 us of a one-query search).
bool fuse_merge_level1(const knn_index* ix, int64_t nq, int nlists, int km) {
    return fuse_merge_level2(ix, nq) && ix->merge_fuse1 && km == 16 && nlists > 64 &&
           nlists <= 64 * kRerankWavesHost;
}

// A single-level merge (<= 64 per-split lists of <= 16: the 256 x 256 kernel's 64 lists of 8 / 10)
// inside the rerank workgroup (RerankArgs::s_lists): no merge launch and no round trip of the K'
// candidates through global memory.  Measured at 1024 queries it saves nothing — the 10.8-us
// launch comes back as rerank workgroups that hold their CU longer (125k rows 0.4815 vs 0.4846 ms
// per step, cfg3 3.181 vs 3.189, two runs each on one box: profiles/r05/merge_rerank_ab/) — so it
// is opt-in: IMGREC_MERGE_SINGLE=1 at index creation.
bool fuse_merge_single(const knn_index* ix, int nlists, int km) {
    return ix->merge_single && nlists <= 64 && km <= 16;
}

// A candidate chunk's buffers: the per-split lists (nq x ncand), the merged K' = kc candidates
// and, for the chains that merge with launch_merge_candidates, the merge floor.
int grow_cand(knn_index* ix, int64_t nq, int ncand, int kc, bool floor) {
    int rc;
    if ((rc = ix->cand_d.reserve((size_t)nq * ncand)) != KNN_OK) return rc;
    if ((rc = ix->cand_i.reserve((size_t)nq * ncand)) != KNN_OK) return rc;
    if ((rc = ix->cand2_d.reserve((size_t)nq * kc)) != KNN_OK) return rc;
    if ((rc = ix->cand2_i.reserve((size_t)nq * kc)) != KNN_OK) return rc;
    return floor ? ix->floor.reserve((size_t)nq) : KNN_OK;
}

// The RerankArgs fields every candidate chain sets alike.  The caller adds its arithmetic's bound
// (c_split, c_trunc, q_resid, xr_max), the merged candidates and the raw per-split lists.
RerankArgs rerank_args(const knn_index* ix, int mode, const float* qpad, const float* qnorm,
                       int64_t nq, int k, int kc, float* D, int64_t* I) {
    RerankArgs r{};
    r.mode = mode;
    r.qp = qpad; r.qnorm = qnorm; r.dp = ix->dp; r.xb = ix->xb; r.xn = ix->xn;
    r.xn_max = ix->xn_max; r.id_offset = ix->id_offset; r.kc = kc; r.nq = nq; r.k = k;
    r.metric = kmetric_of(ix); r.c_fp = rerank_coef(ix->dp); r.D = D; r.I = I;
    return r;
}

// The chunk's nlists per-split lists of km (ix->cand_d / cand_i, query stride ncand) become the
// rerank's r->kc candidates and their floor: merged by the rerank itself — in one level (`single`:
// fuse_merge_single) or in two (fuse_merge_level1) — or by a merge launch, whose second level the
// rerank may take (fuse_merge_level2).
int merge_for_rerank(knn_index* ix, int64_t nq, int nlists, int km, int ncand, bool single,
                     RerankArgs* r, hipStream_t st) {
    const int kc = r->kc, ngrp = (nlists + 63) / 64;
    int rc;
    if (ngrp > 1) {
        if ((rc = ix->mws_d.reserve((size_t)nq * ngrp * kc)) != KNN_OK) return rc;
        if ((rc = ix->mws_i.reserve((size_t)nq * ngrp * kc)) != KNN_OK) return rc;
        if ((rc = ix->mws_f.reserve((size_t)nq * ngrp)) != KNN_OK) return rc;
    }
    int l1G = 0;
    const bool l0 = !single && fuse_merge_level1(ix, nq, nlists, km);
    if (l0) l1G = ngrp;
    else if (!single)
        KNN_HIP(launch_merge_candidates(ix->cand_d, ix->cand_i, nq, nlists, km, ncand, km, kc,
                                        ix->id_offset, ix->cand2_d, ix->cand2_i, ix->floor,
                                        ix->mws_d, ix->mws_i, ix->mws_f, st,
                                        fuse_merge_level2(ix, nq) ? &l1G : nullptr));
    r->cd = ix->cand2_d; r->ci = ix->cand2_i; r->floor = ix->floor;
    if (single) r->s_lists = nlists;
    if (l1G > 0) { r->l1_d = ix->mws_d; r->l1_i = ix->mws_i; r->l1_floor = ix->mws_f; r->l1_G = l1G; }
    if (l0) r->l0_lists = nlists;
    return KNN_OK;
}

// The shared screen bound of a chunk that runs the 256 x 256 kernel (knn_b16w.hip): grows
// the index's per-query records and fills what the query prep kernel needs to reset them (sb->rec
// stays NULL for every other plan, and with IMGREC_B16W_SHARED_BOUND=0).  The prep reads the corpus
// maxima, so they are refreshed here, ahead of it.
int shared_bound_prep(knn_index* ix, const Plan& p, const float* qnorm, hipStream_t st,
                      SharedBoundPrep* sb) {
    *sb = SharedBoundPrep{};
    if (!ix->shared_bound || !p.big) return KNN_OK;
    int rc;
    if ((rc = refresh_maxima(ix, st)) != KNN_OK) return rc;
    if ((rc = ix->sbound.reserve((size_t)p.nq_pad * kSBWords)) != KNN_OK) return rc;
    sb->rec = ix->sbound;
    sb->qnorm = qnorm;
    sb->xn_max = ix->xn_max;
    sb->xr_max = ix->xr_max;
    sb->c_acc = b16_acc_coef(ix->dpb);
    sb->c_fp = rerank_coef(ix->dp);
    sb->c_trunc = p.ib > 0 ? (float)std::ldexp(1.0, p.ib - 23) : 0.f;
    sb->metric = kmetric_of(ix);
    sb->km = p.km;
    return KNN_OK;
}

bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &s) != hipSuccess) { (void)hipGetLastError(); return false; }
    return s != hipStreamCaptureStatusNone;
}

// The int8 tail of a chunk that takes the route (search_locked, ahead of the fused query prep):
// the copy is built if this is its first search, the maxima the prep reads are refreshed, the
// query-side buffers grown.  tp->codes stays NULL when the chunk stays on the pure bf16 pass.
int i8tail_prep(knn_index* ix, const RoutePlan& rp, hipStream_t st, I8TailPrep* tp) {
    *tp = I8TailPrep{};
    if (!rp.tail_ok) return KNN_OK;
    const Plan& p = rp.plan;
    // building the copy waits on the host, which a capturing stream does not allow: such a search
    // runs the bf16 pass and leaves the build to the next search outside a capture
    if (ix->xt_state == TailCopy::Undecided && stream_capturing(st)) return KNN_OK;
    int rc;
    if ((rc = ensure_i8tail(ix, st)) != KNN_OK || ix->xt_state != TailCopy::Built) return rc;
    if ((rc = refresh_maxima(ix, st)) != KNN_OK) return rc;
    if ((rc = ix->qt.reserve((size_t)p.nq_pad * ix->xt_row)) != KNN_OK) return rc;
    if ((rc = ix->qts.reserve((size_t)p.nq_pad)) != KNN_OK) return rc;
    if ((rc = ix->q_eip.reserve((size_t)p.nq_pad)) != KNN_OK) return rc;
    tp->codes = ix->qt; tp->scale = ix->qts; tp->e_ip = ix->q_eip;
    tp->xt_max = ix->xt_max; tp->xn_max = ix->xn_max;
    tp->head = ix->xt_head; tp->dpt = ix->xt_dpt; tp->row = ix->xt_row;
    tp->c_acc = i8t_acc_coef(ix->xt_head);
    return KNN_OK;
}

// The first search on a fresh int8 tail copy is a trial (one more host wait on top of the build's):
// whether the int8 band of a corpus fits K' = 64 depends on how its keys are spread, which no
// statistic of the rows tells (bench config 2, 768 homogeneous columns with every in-cluster key
// inside the band: all 1024 queries went to the exact re-run, 35 ms a step against the bf16 pass's
// 1.4).  The route saves about 1 us per query and an exact re-run costs about 35, so re-runs of
// more than 1/32 of the batch eat the gain: past that share the index drops the copy and stays on
// the bf16 pass until reset.  (The second chance is not counted: its cost per query is far below a
// re-run's and unmeasured.)
int i8tail_trial(knn_index* ix, int64_t nq, hipStream_t st) {
    if (stream_capturing(st)) return KNN_OK;           // (no host wait inside a capture: judged later)
    int acc[4] = {0, 0, 0, 0};
    KNN_HIP(hipMemcpyAsync(acc, ix->stat + 8, sizeof(acc), hipMemcpyDeviceToHost, st));
    KNN_HIP(hipStreamSynchronize(st));
    ix->xt_tried = true;
    const int64_t reruns = acc[0];
    if (reruns * 32 <= nq) return KNN_OK;
    drop_i8tail(ix, TailCopy::Ineligible);                  // (st is drained: nothing reads the copy)
    return KNN_OK;
}

// bf16 candidates (one bf16 MFMA per product) + exact fp32 rerank of K' = 64 + certificate.
// i8t: the 256 x 256 kernel's int8-tail sibling (the prep wrote the query's tail codes and e_ip).
int b16_chunk(knn_index* ix, const Plan& p, const float* qpad, const float* qnorm, int64_t nq, int k,
              float* D, int64_t* I, hipStream_t st, bool q_ready, bool first, bool i8t) {
    const int kmetric = kmetric_of(ix);
    const int kc = kB16Cand;
    const int km = p.km;
    int rc;
    if ((rc = refresh_maxima(ix, st)) != KNN_OK) return rc;
    if ((rc = ix->qb16.reserve((size_t)p.nq_pad * ix->dpb)) != KNN_OK) return rc;
    if ((rc = ix->q_resid.reserve((size_t)p.nq_pad)) != KNN_OK) return rc;
    if ((rc = grow_cand(ix, nq, p.ncand, kc, true)) != KNN_OK) return rc;
    if ((rc = grow_stats(ix, nq, st)) != KNN_OK) return rc;
    // (the prep — here or search_locked's — also resets the shared screen bound's records)
    SharedBoundPrep sb;
    if ((rc = shared_bound_prep(ix, p, qnorm, st, &sb)) != KNN_OK) return rc;
    if (!q_ready)   // else search_locked's fused query prep already wrote qb16 / q_resid
        KNN_HIP(launch_bf16_rows(qpad, p.nq_pad, ix->dp, ix->dpb, ix->qb16, ix->q_resid, st, &sb));
    TileArgs a{};
    a.wr = p.wr; a.wq = p.wq; a.km = km; a.wb = kB16WB; a.mode = kModeBF16;
    a.xb = reinterpret_cast<const float*>(ix->xh.get()); a.xnorm = ix->xn; a.nrows = (int)ix->ntotal;
    a.dp = ix->dpb / 2; a.qp = reinterpret_cast<const float*>(ix->qb16.get()); a.qnorm = qnorm;
    a.nq = (int)nq; a.metric = kmetric; a.ntiles = p.ntiles; a.nsplit = p.nsplit; a.nqb = p.nqb;
    a.id_offset = ix->id_offset; a.cand_d = ix->cand_d; a.cand_i = ix->cand_i; a.ncand = p.ncand;
    a.ib = p.big ? p.ib : 0;
    a.sbound = sb.rec;
    if (i8t) {
        if (!p.big || !q_ready || ix->xt_state != TailCopy::Built)
            KNN_FAIL(KNN_EINVAL, "int8 tail without its query prep");
        a.xt = ix->xt; a.xts = ix->xts; a.qt = ix->qt; a.qts = ix->qts;
        a.t_head = ix->xt_head; a.t_dpt = ix->xt_dpt;
    }
    KNN_TIMED(ix, st, p.big ? launch_b16_big(a, st) : launch_tile_topk(a, st));
    const int nlists = p.ncand / km;
    RerankArgs r = rerank_args(ix, kModeBF16, qpad, qnorm, nq, k, kc, D, I);
    r.c_split = b16_acc_coef(ix->dpb);
    r.c_trunc = a.ib > 0 ? (float)std::ldexp(1.0, a.ib - 23) : 0.f;
    r.q_resid = ix->q_resid; r.xr_max = ix->xr_max;
    if (i8t) r.e_ip = ix->q_eip;
    r.sbound = a.sbound;
    if ((rc = merge_for_rerank(ix, nq, nlists, km, p.ncand, fuse_merge_single(ix, nlists, km), &r,
                               st)) != KNN_OK)
        return rc;
    r.raw_d = ix->cand_d; r.raw_i = ix->cand_i; r.raw_lists = nlists; r.raw_km = km;
    r.raw_stride_q = p.ncand;
    return certify_chunk(ix, r, qpad, qnorm, nq, k, D, I, st, first);
}

// Block-scaled int8 candidates (int8 dot4 products, batches of <= kI8MaxQ queries) + exact fp32
// rerank of K' = 64 + certificate: the bf16 path's chain with the int8 copy's bound.
int i8_chunk(knn_index* ix, const Plan& p, const float* qraw, const float* qpad, const float* qnorm,
             int64_t nq, int k, float* D, int64_t* I, hipStream_t st, bool first) {
    const int kmetric = kmetric_of(ix);
    const int kc = kB16Cand;
    // direct: no merge, no rerank launch — the certificate tail reranks every query's list entries
    // under its prefix limit (RerankArgs::direct); the scan zeroes the tail's claim counters and
    // (raw: <= 4 queries) writes its 16 lane lists per split unfolded
    const bool direct = ix->chance_direct_max > 0 && nq <= ix->chance_direct_max && k <= 64;
    // (unfolded while they make <= 4096 lists per query, i.e. <= 1024 entries per second-chance
    // slice: config 3's 256 splits 2 us faster, config 2's 512 splits 1 us slower than folded,
    // profiles/r05/nq1/direct_raw/; IMGREC_DIRECT_RAW=2: unfolded at any split count)
    const bool raw = direct && nq <= 4 &&
                     (ix->direct_raw == 2 || (ix->direct_raw == 1 && 16 * p.nsplit <= 4096));
    const int ncand = raw ? p.nsplit * 16 * p.km : p.ncand;
    int rc;
    if ((rc = ensure_i8(ix, st)) != KNN_OK) return rc;
    if ((rc = refresh_maxima(ix, st)) != KNN_OK) return rc;
    if ((rc = grow_cand(ix, nq, ncand, kc, true)) != KNN_OK) return rc;
    if ((rc = grow_stats(ix, nq, st)) != KNN_OK) return rc;
    // qraw non-NULL: the scan quantises the raw query rows itself and writes qpad / qnorm /
    // q8r (I8Args::qsrc); otherwise the codes ix->q8 / q8s / q8r came with qpad from
    // launch_i8_query_prep
    I8Args a{};
    a.codes = ix->x8; a.scales = ix->x8s; a.xnorm = ix->xn; a.nrows = (int)ix->ntotal;
    a.nblk = ix->nblk8; a.nq = (int)nq;
    if (qraw) {
        a.qsrc = qraw; a.d = ix->d; a.dp = ix->dp;
        a.normalize = ix->metric == KNN_METRIC_COSINE ? 1 : 0;
        a.qpad = const_cast<float*>(qpad); a.qnorm_out = const_cast<float*>(qnorm); a.qresid = ix->q8r;
    } else {
        a.qcodes = ix->q8; a.qscales = ix->q8s; a.qnorm = qnorm;
    }
    a.km = p.km;
    a.nsplit = p.nsplit; a.l2 = kmetric; a.id_offset = ix->id_offset; a.cand_d = ix->cand_d;
    a.cand_i = ix->cand_i; a.ncand = ncand; a.raw16 = raw ? 1 : 0;
    if (p.nsplit == 2 * ix->cus) a.half_k = ix->i8_half_k;     // two workgroups per CU
    if (ix->i8_pool64 > 0 && nq <= 2 && p.km == 16 &&
        (ix->i8_pool_forced || (nq == 1 && p.nsplit == ix->cus))) {
        // run-time pool of the last row groups (I8Args::pool): replaces the half_k shift
        if (!ix->i8_dyn) {
            if ((rc = ix->i8_dyn.reserve(2)) != KNN_OK) return rc;
            KNN_HIP(hipMemsetAsync(ix->i8_dyn, 0, 2 * sizeof(int), st));
        }
        a.dyn = ix->i8_dyn;
        a.pool = (int)((ix->ntotal + 7) / 8 * ix->i8_pool64 / 64);
        a.pool_ch = ix->i8_pool_ch;
        a.half_k = 0;
    }
    if (direct) {
        if ((rc = ix->tail_ctl.reserve((size_t)4 + round_up(nq, 32) / 32)) != KNN_OK)
            return rc;
        a.zero_ctl = ix->tail_ctl;
        if ((rc = ix->heads.reserve((size_t)nq * p.nsplit)) != KNN_OK) return rc;
        a.heads = ix->heads;
    }
    KNN_TIMED(ix, st, launch_i8_scan(a, st));
    const int nlists = p.nsplit;
    RerankArgs r = rerank_args(ix, kModeI8, qpad, qnorm, nq, k, kc, D, I);
    r.c_split = i8_acc_coef(ix->nblk8);
    r.q_resid = ix->q8r; r.xr_max = ix->x8r_max;
    r.raw_d = ix->cand_d; r.raw_i = ix->cand_i; r.raw_lists = raw ? 16 * nlists : nlists;
    r.raw_km = p.km;
    r.raw_stride_q = ncand;
    if (direct) {
        r.direct = 1;
        r.heads = ix->heads;
        r.heads_n = nlists;
    } else if ((rc = merge_for_rerank(ix, nq, nlists, p.km, ncand, false, &r, st)) != KNN_OK) {
        return rc;
    }
    return certify_chunk(ix, r, qpad, qnorm, nq, k, D, I, st, first);
}

// Split-bf16 candidates + exact rerank + certificate.
int split_chunk(knn_index* ix, const Plan& p, const float* qpad, const float* qnorm, int64_t nq, int k,
                float* D, int64_t* I, hipStream_t st, bool first) {
    const int kmetric = kmetric_of(ix);
    const int kc = p.km;                     // split_kc(k)
    int rc;
    if ((rc = ensure_split(ix, st)) != KNN_OK) return rc;
    if ((rc = refresh_maxima(ix, st)) != KNN_OK) return rc;
    if ((rc = ix->qsplit.reserve((size_t)p.nq_pad * ix->dp)) != KNN_OK) return rc;
    if ((rc = grow_cand(ix, nq, p.ncand, kc, false)) != KNN_OK) return rc;   // (launch_merge: no floor)
    if ((rc = grow_stats(ix, nq, st)) != KNN_OK) return rc;
    KNN_HIP(launch_split_rows(qpad, p.nq_pad, ix->dp, kSplitBK, ix->qsplit, st));
    TileArgs a{};
    a.wr = p.wr; a.wq = p.wq; a.km = kc;
    a.xb = reinterpret_cast<const float*>(ix->xs.get()); a.xnorm = ix->xn; a.nrows = (int)ix->ntotal;
    a.dp = ix->dp; a.qp = reinterpret_cast<const float*>(ix->qsplit.get()); a.qnorm = qnorm;
    a.nq = (int)nq; a.metric = kmetric; a.ntiles = p.ntiles; a.nsplit = p.nsplit; a.nqb = p.nqb;
    a.id_offset = ix->id_offset; a.cand_d = ix->cand_d; a.cand_i = ix->cand_i;
    a.ncand = p.ncand; a.mode = kModeSplit;
    a.wb = kSplitWB; a.sbk = kSplitBK;
    KNN_TIMED(ix, st, launch_tile_topk(a, st));
    // global top-K' approximate candidates, raw ascending keys (merge in its L2 convention)
    KNN_HIP(launch_merge(ix->cand_d, ix->cand_i, nq, p.ncand / kc, kc, p.ncand, kc, kc, 1, 0,
                         ix->cand2_d, ix->cand2_i, st));
    RerankArgs r = rerank_args(ix, kModeSplit, qpad, qnorm, nq, k, kc, D, I);
    r.cd = ix->cand2_d; r.ci = ix->cand2_i;
    r.c_split = split_coef(ix->dp);
    r.raw_d = ix->cand_d; r.raw_i = ix->cand_i; r.raw_lists = p.ncand / kc; r.raw_km = kc;
    r.raw_stride_q = p.ncand;
    return certify_chunk(ix, r, qpad, qnorm, nq, k, D, I, st, first);
}

}  // namespace

int search_locked(knn_index* ix, const float* q, int64_t nq, int k, float* D, int64_t* I,
                  hipStream_t st) {
    const int normalize = ix->metric == KNN_METRIC_COSINE;
    const int kmetric = kmetric_of(ix);
    ix->last_split_queries = 0;
    ix->stat_valid = false;
    if (k > KNN_MAX_K) {               // register top-k lists end at 32: faiss's GEMM + select form
        ix->last_path = 0;
        return k > KNN_MAX_K_LARGE ? hugek_search(ix, q, nq, k, D, I, st)
                                   : largek_search(ix, q, nq, k, D, I, st);
    }
    if (ix->ntotal == 0) {
        KNN_HIP(launch_fill_empty(D, I, nq * (int64_t)k, kmetric, st));
        return KNN_OK;
    }
    bool first_cand = true, any_i8t = false;
    for (int64_t c0 = 0; c0 < nq; c0 += kQueryChunk) {
        const int64_t cn = std::min(kQueryChunk, nq - c0);
        // the chunk's one decision; padding: the query tile of its plan (and the exact re-run's 32)
        const RoutePlan rp = choose_route(*ix, cn, k);
        const Plan& p = rp.plan;
        const bool i8 = rp.route == Route::I8, b16 = rp.route == Route::B16;
        const int64_t nq_pad = p.nq_pad;
        int rc;
        if (c0 == 0) ix->last_path = (int)rp.route;
        if ((rc = ix->qpad.reserve((size_t)nq_pad * ix->dp)) != KNN_OK) return rc;
        if ((rc = ix->qnorm.reserve((size_t)nq_pad)) != KNN_OK) return rc;
        bool i8t = false;
        // fused query prep: fp32 padded rows + norms + bf16 + residuals, or for the int8 path
        // the same rows and norms + the two-level int8 codes (one short pass instead of
        // rows_ingest's latency-bound row loop and a second launch)
        // (the int8 path's prep runs inside its scan unless IMGREC_I8_FUSED_PREP=0: nq_pad = cn)
        const bool i8_fused = i8 && ix->i8_fused_prep && nq_pad == cn && cn <= 4;
        const bool q_ready = b16 && ix->dpb <= 4096;     // b16_chunk: the prep here wrote qb16 / q_resid
        if (i8 && (rc = ix->q8r.reserve((size_t)cn)) != KNN_OK) return rc;
        if (i8 && !i8_fused) {
            if ((rc = ix->q8.reserve((size_t)cn * ix->nblk8 * 128)) != KNN_OK) return rc;
            if ((rc = ix->q8s.reserve((size_t)cn * ix->nblk8 * 2)) != KNN_OK) return rc;
            KNN_HIP(launch_i8_query_prep(q + c0 * ix->d, cn, ix->d, ix->dp, nq_pad, normalize,
                                         ix->nblk8, ix->qpad, ix->qnorm, ix->q8, ix->q8s, ix->q8r, st));
        } else if (q_ready) {
            if ((rc = ix->qb16.reserve((size_t)nq_pad * ix->dpb)) != KNN_OK) return rc;
            if ((rc = ix->q_resid.reserve((size_t)nq_pad)) != KNN_OK) return rc;
            I8TailPrep tp;
            if ((rc = i8tail_prep(ix, rp, st, &tp)) != KNN_OK) return rc;
            i8t = tp.codes != nullptr;
            SharedBoundPrep sb;
            if ((rc = shared_bound_prep(ix, p, ix->qnorm, st, &sb)) != KNN_OK) return rc;
            KNN_HIP(launch_query_prep_b16(q + c0 * ix->d, cn, ix->d, ix->dp, ix->dpb, nq_pad,
                                          normalize, ix->qpad, ix->qnorm, ix->qb16, ix->q_resid, st,
                                          &sb, &tp));
        } else if (!i8) {
            KNN_HIP(launch_rows_ingest(q + c0 * ix->d, cn, ix->d, ix->dp, nq_pad, normalize,
                                       ix->qpad, ix->qnorm, st));
        }
        float* Dc = D + c0 * k;
        int64_t* Ic = I + c0 * k;
        const float *qp = ix->qpad, *qn = ix->qnorm;
        rc = i8 ? i8_chunk(ix, p, i8_fused ? q + c0 * ix->d : nullptr, qp, qn, cn, k, Dc, Ic, st, first_cand)
           : b16 ? b16_chunk(ix, p, qp, qn, cn, k, Dc, Ic, st, q_ready, first_cand, i8t)
           : rp.route == Route::Split ? split_chunk(ix, p, qp, qn, cn, k, Dc, Ic, st, first_cand)
                                      : exact_chunk(ix, p, qp, qn, cn, k, Dc, Ic, st);
        first_cand = first_cand && rp.route == Route::Exact;
        if (rc != KNN_OK) return rc;
        any_i8t = any_i8t || i8t;
    }
    return any_i8t && !ix->xt_tried && !ix->xt_no_trial ? i8tail_trial(ix, nq, st) : KNN_OK;
}

// Totals of the last search's candidate chunks (read on the index's own stream, which it
// synchronises: while stat_valid the caller holds a begun host scope).
int read_search_stats(knn_index* ix, int64_t* split_q, int64_t* fallback_q, int64_t* first_fail,
                      float* ratio) {
    *split_q = ix->last_split_queries;
    *fallback_q = 0;
    if (first_fail) *first_fail = 0;
    if (ratio) *ratio = 0.f;
    if (!ix->stat_valid) return KNN_OK;
    int acc[4] = {0, 0, 0, 0};
    KNN_HIP(hipMemcpyAsync(acc, ix->stat + 8, sizeof(acc), hipMemcpyDeviceToHost, ix->stream));
    KNN_HIP(hipStreamSynchronize(ix->stream));
    if (acc[3] != 0) {        // cert_tail_kernel's bounded wait for its planner ran out
        // reported once: clear the bit so later clean searches read their stats again
        const int zero = 0;
        KNN_HIP(hipMemcpyAsync(ix->stat + 11, &zero, sizeof(int), hipMemcpyHostToDevice, ix->stream));
        KNN_HIP(hipStreamSynchronize(ix->stream));
        KNN_FAIL(KNN_EHIP, "certificate tail: a workgroup gave up waiting for the re-run plan "
                           "(error bits 0x%x); results of that search are not certified", acc[3]);
    }
    *fallback_q = acc[0];
    if (first_fail) *first_fail = acc[2];
    if (ratio) std::memcpy(ratio, &acc[1], sizeof(float));
    return KNN_OK;
}

}  // namespace imgrec
