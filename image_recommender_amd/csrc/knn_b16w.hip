// knn_b16w.hip — the 256 x 256-tile bf16 candidate kernel of the k-NN search, on
// v_mfma_f32_16x16x32_bf16 (gfx950 / MI355X).
//
// Contract: score every corpus row of the workgroup's row split against a block of 256 queries
// with one bf16 MFMA per product (fp32 accumulation) and keep, per (query, row split), the KM best
// approximate keys in registers; knn_refine.hip reranks and certifies the merged candidates.  It
// replaces the arithmetic of faiss IndexFlat.search reached from main/search_from_image.py:247.
//
// Why a kernel of its own: the 128 x 128 tile of the generic kernel (knn_kernels.hip) stages
// 2 bytes of LDS-DMA per MFMA; at one workgroup per CU a 256 x 256 tile halves the staged bytes
// (2 N D Q (1/BM + 1/BQ)).  Why the 16 x 16 MFMA form: in a power-limited MFMA loop the chip holds
// a higher clock on v_mfma_f32_16x16x32_bf16 than on v_mfma_f32_32x32x16_bf16 at equal cycles per
// flop (MI355X_MICROARCH.md, DVFS give-back item 7).
//
// Geometry: 8 waves along the queries; wave w owns queries 32w .. 32w + 31 of the block (two
// 16-query MFMA blocks) against all 256 rows of the tile (sixteen 16-row blocks): 32 MFMAs per
// 32-deep k-step, 128 accumulator registers per lane.  With the 16 x 16 accumulator map (col =
// lane & 15 -> query, row = 4 (lane >> 4) + reg) each lane owns two queries and 64 rows of each,
// so the top-k keeps two register lists per lane and needs no data movement; the four lanes of
// a query (one per lane quarter) hold its four lists, so the screen's shared bound and the final
// fold are wave-local shuffles (no LDS share region, no cross-wave fold).
//
// LDS image: a stage = 64 bf16 of depth per row (128 B, two 32-deep k-steps) for 256 rows (A) +
// 256 queries (B) = 64 KiB, in a two-slot ring (128 KiB), then a four-tile ring of row norms, the
// waves' shared-bound records and the per-query screen state (150 KiB in all).  Row r of a stage
// keeps its 16-B chunk c at chunk c ^ ((r >> 1) & 7) (two 128-B rows per 256-B bank row); the XOR
// is applied on the DMA's per-lane global source offset.  k-step c of lane quarter lq reads
// logical chunk 4c + lq of row (lane & 15) of a 16-row block, so every ds_read_b128 lane group of
// 16 hits 16 distinct bank slots.
//
// Row splits: the corpus is cut into groups of kRPP = 8 rows (one DMA piece each); split s owns
// the global groups s, s + nsplit, s + 2 nsplit, ... and a tile holds kGPT consecutive groups of
// its split.  The splits are interleaved because a stored order that keeps similar rows together
// (the reference stores images folder by folder) is thereby spread over every split, so no
// split's short list has to hold most of a query's neighbours — with contiguous splits the merge
// floor bound on such corpora and sent a quarter of the queries to the exact re-run.
//
// DMA: each wave moves 8 one-KiB pieces per stage (waves 0-3 the corpus tile, 4-7 the query tile)
// with global_load_lds_dwordx4 in the saddr form (lds_dma.h): one per-piece 32-bit lane offset
// fixed for the whole launch, one scalar base per stage, one M0 write per four pieces (the
// instruction offset j KiB moves both the global source and the LDS destination, so the lane
// offsets are pre-reduced by j KiB).  A tile's corpus pieces sit nsplit * kRPP rows apart: the
// lane offsets stay fixed and the scalar base moves by kGPT groups per tile.  Pieces are kPS bytes
// apart and the swizzle of a piece's rows depends only on the piece's parity, so a lane keeps two
// bases and piece j's offset is vpar[j & 1] + (j & ~1) kPS - 1024 (j & 3).
//
// Schedule: a stage's 64 MFMAs run as 8 quads (4 row blocks x 2 query blocks each); the next
// quad's fragments are read under the current quad's MFMAs, one read per MFMA gap.  One barrier
// per stage, before its last quad: by then every wave has read the whole stage (its slot is
// refilled with stage g + 2 right after) and waited for its own DMA of stage g + 1, so the next
// stage's first fragments are read after the barrier while the last quad's MFMAs run and the MFMA
// pipe does not drain.  The corpus-tile waves issue the DMA of stage g + 2 right after the
// barrier, the query-tile waves (static priority 1: the younger half loses issue arbitration
// otherwise) kDeferQ quads later, so each SIMD's MFMA pipe has a feeder during either wave's DMA
// issue.  After a tile's last stage the top-k epilogue runs without barriers (it touches no stage
// memory).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <type_traits>

#include "knn_kernels.h"
#include "knn_plan.h"
#include "lds_dma.h"
#include "wave_ops.h"

namespace imgrec {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kNW = 8;                    // waves, all along the queries
constexpr int kBM = kB16BigRows;          // 256 corpus rows per tile
constexpr int kBQ = kB16BigQueries;       // 256 queries per workgroup
constexpr int kQW = kBQ / kNW;            // 32 queries per wave
constexpr int kRB = kBM / 16;             // 16-row blocks per tile
constexpr int kBKW = 32;                  // 32-bit words (2 bf16) per staged row
constexpr int kNS = 2;                    // stages in the LDS ring
constexpr int kRowB = kBKW * 4;           // bytes per staged row
constexpr int kCPR = kBKW / 4;            // 16-B chunks per staged row
constexpr int kRPP = 64 / kCPR;           // rows per one-KiB DMA piece
constexpr int kRPB = 64 / kBKW;           // rows per 256-B bank row
constexpr int kGPT = kBM / kRPP;          // row groups (= A pieces) per tile
constexpr int kSA = kBM * kRowB;          // A (corpus) stage bytes
constexpr int kSB = kBQ * kRowB;          // B (query) stage bytes
constexpr int kStage = kSA + kSB;
constexpr int kLPW = (kBM + kBQ) / kRPP / kNW;   // DMA pieces per wave per stage
constexpr int kNormSlots = 4;             // row-norm ring (tiles)
constexpr int kNormOff = kNS * kStage;
// shared screen bound: per wave its kQW query records (kSBWords words each: 2 KiB, two LDS-DMA
// pieces), then per query (lu, last published value)
constexpr int kRecOff = kNormOff + kNormSlots * kBM * 4;
constexpr int kLuOff = kRecOff + kNW * kQW * kSBWords * 4;
constexpr int kLDS = kLuOff + kBQ * 2 * 4;
static_assert(kQW * kSBWords * 4 == 2048 && kSBWords == 16, "a wave's records: one dma2_agent of 2 KiB");
static_assert(kLDS == 153600, "LDS image");
// int8-tail sibling (knn_b16w_tile_kernel_i8t): a ring of the tiles' row scales next to the image
// and the queries' scales (one float per query of the block, written and read by the query's wave)
constexpr int kScaleOff = kLDS;
constexpr int kQScaleOff = kScaleOff + kNormSlots * kBM * 4;
constexpr int kQNormOff = kQScaleOff + kBQ * 4;     // and their |q|^2 (registers in the bf16 instances)
constexpr int kLDST = kQNormOff + kBQ * 4;
static_assert(kLDST <= 160 * 1024, "LDS budget (int8 tail)");
constexpr int kQuads = 8;                 // MFMA quads per stage (2 k-steps x 4)
// the query-tile waves issue their DMA after this quad of the next stage (the corpus-tile waves
// issue theirs right after the barrier), so each SIMD's other wave feeds the MFMA pipe meanwhile
#ifndef IMGREC_B16W_DEFER_Q
#define IMGREC_B16W_DEFER_Q 3
#endif
constexpr int kDeferQ = IMGREC_B16W_DEFER_Q;
static_assert(kBKW == 32 && kCPR == 8, "stage depth: two 32-deep k-steps per stage");
static_assert(kLDS <= 160 * 1024, "LDS budget");
static_assert(kLPW % 4 == 0, "pieces go out in dma4x groups of four");
static_assert(kDeferQ >= 0 && kDeferQ < kQuads - 1, "deferred DMA inside the stage's first quads");
// Insertion: a passing row's accumulator and norm are picked from the registers of its two row
// blocks by a 3-level v_cndmask tree (sel8; the norms stay in the registers the screen loaded
// them into), with no trip through LDS.
// Measurement builds only (tools/b16w_epi_split.sh; the lists they return are wrong):
// 1 = no per-tile epilogue (the stage loop alone), 2 = the screen without the insertions, 3 = the
// int8-tail sibling without its fold (the bf16 kernels as 0).  1 and 2
// hand every accumulator (and 2 the screen's masks) to an empty asm at each tile end, so the
// MFMAs and the screen stay live (round 6: without it the compiler dropped every MFMA — PMC
// SQ_INSTS_MFMA = 0, profiles/r06/epi_split/pmc_invalid_variants/).
#ifndef IMGREC_B16W_EPI_EXP
#define IMGREC_B16W_EPI_EXP 0
#endif

// Ascending register list, labels arriving in increasing order per lane: slot p's key is the
// median of (kd[p-1], d, kd[p]); selects stay v_cndmask (no branches); d = +inf is a no-op.
template <int K>
__device__ __forceinline__ void insert_mono(float (&kd)[K], int (&ki)[K], float d, int id) {
    bool c[K];
#pragma unroll
    for (int p = 0; p < K; ++p) c[p] = d < kd[p];
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
        kd[p] = __builtin_amdgcn_fmed3f(kd[p - 1], d, kd[p]);
        const int nx = __builtin_unpredictable(c[p]) ? id : ki[p];
        ki[p] = __builtin_unpredictable(c[p - 1]) ? ki[p - 1] : nx;
    }
    kd[0] = __builtin_unpredictable(c[0]) ? d : kd[0];
    ki[0] = __builtin_unpredictable(c[0]) ? id : ki[0];
}

__device__ __forceinline__ bool rank_lt(float d1, int i1, float d2, int i2) {
    return i2 < 0 || d1 < d2 || (d1 == d2 && i1 < i2);
}

template <int K>
__device__ __forceinline__ void insert_any(float (&kd)[K], int (&ki)[K], float d, int id) {
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
        const bool shift = rank_lt(d, id, kd[p - 1], ki[p - 1]);
        const bool here = !shift && rank_lt(d, id, kd[p], ki[p]);
        kd[p] = shift ? kd[p - 1] : (here ? d : kd[p]);
        ki[p] = shift ? ki[p - 1] : (here ? id : ki[p]);
    }
    const bool here0 = rank_lt(d, id, kd[0], ki[0]);
    kd[0] = here0 ? d : kd[0];
    ki[0] = here0 ? id : ki[0];
}

// min / max over the four lane quarters of a column (lanes l, l ^ 16, l ^ 32, l ^ 48): a
// v_permlane16_swap then a v_permlane32_swap of the value with itself hands every lane its row
// partner's value in the other output register (no LDS crossbar round trip, unlike ds_bpermute)
__device__ __forceinline__ float quarter_min(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fminf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fminf(__uint_as_float(s[0]), __uint_as_float(s[1]));
}
__device__ __forceinline__ float quarter_max(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1]));
}

__device__ __forceinline__ uint32_t quarter_min_u(uint32_t x) {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    x = min(r[0], r[1]);
    const auto s = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return min(s[0], s[1]);
}
__device__ __forceinline__ uint32_t quarter_max_u(uint32_t x) {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    x = max(r[0], r[1]);
    const auto s = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return max(s[0], s[1]);
}

// Packed list entries (PACK): the order-preserving bits of the key (ascending floats ->
// ascending u32) with the low ib bits replaced by the split-local row index, so one u32 compare
// orders entries by (key truncated toward -inf, row) and an insertion is one v_med3_u32 per slot.
__device__ __forceinline__ uint32_t ord_bits(float k) {
    const uint32_t u = __float_as_uint(k);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_float(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
// x[r] of eight register values, r in [0, 8) (lane-varying): three levels of v_cndmask
__device__ __forceinline__ float sel8(int r, float x0, float x1, float x2, float x3, float x4, float x5,
                                      float x6, float x7) {
    const bool b0 = r & 1, b1 = r & 2, b2 = r & 4;
    const float a0 = b0 ? x1 : x0, a1 = b0 ? x3 : x2, a2 = b0 ? x5 : x4, a3 = b0 ? x7 : x6;
    const float c0 = b1 ? a1 : a0, c1 = b1 ? a3 : a2;
    return b2 ? c1 : c0;
}
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    return max(min(a, b), min(max(a, b), c));          // -> v_med3_u32
}
// ascending packed list, any arrival order (entries are distinct; ~0u = empty, and inserting it
// or anything at or above the last entry changes nothing)
template <int K>
__device__ __forceinline__ void insert_packed(uint32_t (&kp)[K], uint32_t u) {
#pragma unroll
    for (int p = K - 1; p > 0; --p) kp[p] = umed3(kp[p - 1], u, kp[p]);
    kp[0] = min(kp[0], u);
}
// smallest key of the bucket after u's (every key that truncates to u's bucket or below is
// smaller): the screen threshold a packed list entry stands for
__device__ __forceinline__ float bucket_end(uint32_t u, uint32_t lowmask) {
    return u == ~0u ? INFINITY : ord_float((u | lowmask) + 1u);
}

}  // namespace

#ifdef IMGREC_B16_STAMPS
// diagnostic build only (tools/b16_stamps.py): s_memtime per wave at fixed points of one tile
__device__ unsigned long long g_b16w_stamps[8 * 256];
// per workgroup (blockIdx.x < 1024): s_memrealtime (100 MHz) at entry and after its last tile
__device__ unsigned long long g_b16w_wg[2 * 1024];
#define B16W_STAMP(slot) do { if (stamp_on && lane == 0) { \
    unsigned long long v_ = __builtin_amdgcn_s_memtime(); g_b16w_stamps[wave * 256 + (slot)] = v_; } } while (0)
// per workgroup (blockIdx.x < 1024), wave 0's sums over its tiles' stage loops, (shader cycles,
// 100 MHz ticks, stages) for the int8 tail stages, then for the bf16 stages: one s_memtime and one
// s_memrealtime before and after each loop (tools/i8joint_stamps.py: cycles per stage, clock)
__device__ unsigned long long g_b16w_loop[6 * 1024];
#define B16W_LOOP_BEGIN() const unsigned long long lc0_ = __builtin_amdgcn_s_memtime(), \
                                                   lr0_ = __builtin_amdgcn_s_memrealtime()
#define B16W_LOOP_END(kind, n) do { lp_cyc[kind] += __builtin_amdgcn_s_memtime() - lc0_; \
    lp_rt[kind] += __builtin_amdgcn_s_memrealtime() - lr0_; lp_n[kind] += (unsigned long long)(n); } while (0)
#else
#define B16W_STAMP(slot) do {} while (0)
#define B16W_LOOP_BEGIN() do {} while (0)
#define B16W_LOOP_END(kind, n) do {} while (0)
#endif

// PACK: one u32 per list entry (see ord_bits), ib = index bits (host: every split-local row index
// t * 256 + tile row fits); otherwise separate key / label lists (any corpus size).
//
// I8T (knn_b16w_tile_kernel_i8t, DESIGN.md "int8 tail"): xh, qh and dw carry the joint rows of the
// tail copy — a row is its tail codes, then its bf16 head, dw words in all — so a tile's stage s
// reads bytes [128 s, 128 s + 128) of every row and query, exactly as the bf16 kernel does.  The
// first ta.nst_t stages are 128 int8 deep (the same 128 B per row, the same two k-steps of four
// 16-B chunks and the same fragment addresses, on v_mfma_i32_16x16x64_i8 into the accumulator
// registers as int32), then the registers are folded in place to fp32 (x row scale x query scale)
// and the remaining bf16 stages of the rows' head columns accumulate on top.
struct I8TailArgs {
    const float* xts = nullptr;      // per-row scale
    const float* qts = nullptr;      // per-query scale
    int nst_t = 0;                   // tail stages of a joint row
};

template <int KM, int L2, bool PACK>
__global__ void __launch_bounds__(512, 2)
knn_b16w_tile_kernel(const uint32_t* __restrict__ xh, const float* __restrict__ xnorm, int nrows,
                     int dw, const uint32_t* __restrict__ qh, const float* __restrict__ qnorm, int nq,
                     int nsplit, int nqb, int64_t id_offset, float* __restrict__ cand_d,
                     int64_t* __restrict__ cand_i, int ncand, int ib, uint32_t* sbound) {
    __shared__ __attribute__((aligned(16))) char smem[kLDS];
#define B16W_I8T 0
#include "knn_b16w_body.inc"
#undef B16W_I8T
}

// The int8-tail sibling: the same tile, ring, epilogue and lists (knn_b16w_body.inc with I8T = true).
template <int KM, int L2, bool PACK>
__global__ void __launch_bounds__(512, 2)
knn_b16w_tile_kernel_i8t(const uint32_t* __restrict__ xh, const float* __restrict__ xnorm, int nrows,
                         int dw, const uint32_t* __restrict__ qh, const float* __restrict__ qnorm, int nq,
                         int nsplit, int nqb, int64_t id_offset, float* __restrict__ cand_d,
                         int64_t* __restrict__ cand_i, int ncand, int ib, uint32_t* sbound,
                         const I8TailArgs ta) {
    __shared__ __attribute__((aligned(16))) char smem[kLDST];
#define B16W_I8T 1
    constexpr bool I8T = true;
#include "knn_b16w_body.inc"
#undef B16W_I8T
}

hipError_t launch_b16_big(const TileArgs& a, hipStream_t st) {
    if (a.wr != 2 || a.wq != 4 || a.dp % kBKW != 0 || a.nsplit < 1) return hipErrorInvalidValue;
    // the lane offsets are 32-bit: a tile's last group sits (kGPT - 1) * nsplit groups past its first
    const auto off_ok = [&](int64_t row_bytes) {
        return ((int64_t)(kGPT - 1) * a.nsplit * kRPP + kBQ) * row_bytes + 8192 < ((int64_t)1 << 32);
    };
    if (!off_ok((int64_t)a.dp * 4)) return hipErrorInvalidValue;
    const bool i8t = a.xt != nullptr;
    I8TailArgs ta;
    const dim3 grid((unsigned)(a.nqb * a.nsplit)), block(kNW * 64);
    const uint32_t* xh = reinterpret_cast<const uint32_t*>(a.xb);
    const uint32_t* qh = reinterpret_cast<const uint32_t*>(a.qp);
    int dw = a.dp;
    if (i8t) {
        // the head is whole 64-column stages inside the bf16 rows, the tail whole 128-column stages;
        // the kernel reads both from the joint rows (i8t_joint_row_bytes) at one stride
        if (a.t_head < 0 || a.t_head % 64 != 0 || a.t_head > 2 * a.dp || a.t_dpt < 128 || a.t_dpt % 128 != 0 ||
            !a.xts || !a.qt || !a.qts || !off_ok(i8t_joint_row_bytes(a.t_head, a.t_dpt)))
            return hipErrorInvalidValue;
        xh = reinterpret_cast<const uint32_t*>(a.xt);
        qh = reinterpret_cast<const uint32_t*>(a.qt);
        dw = i8t_joint_row_bytes(a.t_head, a.t_dpt) / 4;
        ta.xts = a.xts;
        ta.qts = a.qts;
        ta.nst_t = i8t_tail_stages(a.t_dpt);
    }
    if (a.ib < 0 || a.ib > kB16PackMaxIB) return hipErrorInvalidValue;
#define IMGREC_LAUNCH_B16W(KMV, L2V, PK)                                                             \
    do {                                                                                             \
        if (i8t)                                                                                     \
            hipLaunchKernelGGL((knn_b16w_tile_kernel_i8t<KMV, L2V, PK>), grid, block, 0, st, xh,    \
                               a.xnorm, a.nrows, dw, qh, a.qnorm, a.nq, a.nsplit, a.nqb,             \
                               a.id_offset, a.cand_d, a.cand_i, a.ncand, a.ib, a.sbound, ta);        \
        else                                                                                         \
            hipLaunchKernelGGL((knn_b16w_tile_kernel<KMV, L2V, PK>), grid, block, 0, st, xh,        \
                               a.xnorm, a.nrows, a.dp, qh, a.qnorm, a.nq, a.nsplit, a.nqb,           \
                               a.id_offset, a.cand_d, a.cand_i, a.ncand, a.ib, a.sbound);            \
    } while (0)
#define IMGREC_LAUNCH_B16W_K(KMV, PK)                                                               \
    do { if (a.metric == 1) IMGREC_LAUNCH_B16W(KMV, 1, PK); else IMGREC_LAUNCH_B16W(KMV, 0, PK); } while (0)
    if (a.km == 8) {
        if (a.ib > 0) IMGREC_LAUNCH_B16W_K(8, true); else IMGREC_LAUNCH_B16W_K(8, false);
    } else if (a.km == 10) {
        if (a.ib > 0) IMGREC_LAUNCH_B16W_K(10, true); else IMGREC_LAUNCH_B16W_K(10, false);
    } else {
        return hipErrorInvalidValue;
    }
#undef IMGREC_LAUNCH_B16W_K
#undef IMGREC_LAUNCH_B16W
    return hipGetLastError();
}

}  // namespace imgrec


#ifdef IMGREC_B16_STAMPS
extern "C" int knn_b16w_stamps_read(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(imgrec::g_b16w_stamps), sizeof(imgrec::g_b16w_stamps));
}
extern "C" int knn_b16w_wg_read(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(imgrec::g_b16w_wg), sizeof(imgrec::g_b16w_wg));
}
extern "C" int knn_b16w_loop_read(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(imgrec::g_b16w_loop), sizeof(imgrec::g_b16w_loop));
}
#endif
