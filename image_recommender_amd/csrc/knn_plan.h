// knn_plan.h — which route a chunk of queries takes and with what launch geometry (knn_plan.cpp;
// DESIGN.md "Launch plan").  Integer arithmetic on the few fields of IndexShape: no HIP header, so
// the whole decision is checked on a machine with no GPU (tests/fuzz/route_check.cpp).
#pragma once

#include <cstdint>

#include "../../include/imgrec_knn.h"
#include "knn_consts.h"

namespace imgrec {

struct Plan {
    int wr, wq, km, bm, bq;
    int nqb, nq_pad, ntiles, nsplit, ncand, wgs;
    bool big;                    // bf16 path: the 256 x 256-tile kernel (knn_b16w.hip)
    int ib;                      // > 0: its packed-list form with ib split-local index bits
};
constexpr int64_t kQueryChunk = 8192;
Plan make_plan(int64_t ntotal, int64_t nq, int k, int cus);
Plan make_split_plan(int64_t ntotal, int64_t nq, int kc, int cus);
Plan make_b16_plan(int64_t ntotal, int64_t nq, int k, int cus, int dpb);
// The exact re-run of uncertified queries (inside the certificate tail kernel): the (2,1) tile
// of make_plan (256 rows x 32 queries), planned on device for whatever count the certificate
// leaves.
constexpr int kFallbackWR = 2;                 // lists per row split = 2 * kFallbackWR
int fallback_km(int k);
int split_kc(int k);
float split_coef(int dp);
float rerank_coef(int dp);
float b16_acc_coef(int dpb);
// int8 tail of the 256 x 256 kernel (knn_b16w_tile_kernel_i8t): the accumulation coefficient of a
// pass with `head` bf16 columns (knn_certify.h i8tail_e_ip), and the split column from the corpus's
// per-block max |x| (nblk = dpb / 64 blocks): a multiple of 64, or -1 = the route is off
float i8t_acc_coef(int head);
int i8t_pick_head(const float* blkmax, int nblk);
constexpr int kI8TMinTail = 512;               // tail columns below which the route is off
// The copy's joint row (and a padded query's): dpt tail codes, then the first `head` columns as
// bf16 — one array and one stride for both operands of a tile, so the kernel stages 128 B of a row
// per stage whichever kind the stage is.  dpt % 128 == 0 and head % 64 == 0: the row is whole
// stages, i8t_tail_stages of codes first, then head / 64 of bf16.  (-1: not such a pair.)
int i8t_joint_row_bytes(int head, int dpt);
int i8t_tail_stages(int dpt);
int i8t_row_stages(int head, int dpt);
constexpr int kI8TStageBytes = 128;
// int8 small-batch pass (knn_i8.hip): batches of at most kI8MaxQ queries, K' = kB16Cand
constexpr int kI8MaxQ = 8;
float i8_acc_coef(int nblk);
// wgpcu: int8 scan workgroups per CU (the split count is CUs x wgpcu); 0 = by batch size
Plan make_i8_plan(int64_t ntotal, int64_t nq, int k, int cus, int wgpcu, int nblk);
constexpr int kI8WGPCUDefault = 0;
constexpr int kB16Cand = 64;                   // K': candidates the bf16 pass hands to the rerank
int b16_km(int k);

// The int8 tail copy of an index (knn_index.h xt / xts / xtm): not decided yet (until reset), built,
// or the index is not eligible.  Changed only by ensure_i8tail and drop_i8tail.
enum class TailCopy { Undecided, Built, Ineligible };

// What the route decision reads of an index.  knn_index inherits it: nothing is copied per search.
struct IndexShape {
    int d = 0, dp = 0, metric = KNN_METRIC_L2, cus = 256, mode = KNN_SEARCH_AUTO;
    int dpb = 0;             // bf16 row stride (elements)
    int nblk8 = 0;           // 64-element blocks per row (d <= 4096)
    int i8_wgpcu = kI8WGPCUDefault;      // IMGREC_I8_WGPCU at creation (A/B and tests)
    bool split_ok = false, b16_ok = false;
    // IMGREC_B16W_I8TAIL=0: AUTO / i8 large batches stay on the pure bf16 256 x 256 kernel
    bool i8tail = true;
    TailCopy xt_state = TailCopy::Undecided;
    int64_t ntotal = 0;
};

enum class Route { Exact = 0, Split = 1, B16 = 2, I8 = 3 };     // the values knn_last_path reports
struct RoutePlan {
    Route route;
    Plan plan;
    // B16 on the 256 x 256 kernel: the int8 tail's conditions that need no build hold (mode, knob,
    // plan); the chunk runs the tail kernel once the copy is Built
    bool tail_ok;
    int i8_inst;             // I8: the scan's query instance (1, 2, 4 or 8); otherwise 0
};
// The route of one chunk of nq <= kQueryChunk queries: the only place one is chosen.  (Searches
// with k > KNN_MAX_K never ask: for them it answers the exact plan, which is what knn_plan reports.)
RoutePlan choose_route(const IndexShape& ix, int64_t nq, int k);

}  // namespace imgrec
