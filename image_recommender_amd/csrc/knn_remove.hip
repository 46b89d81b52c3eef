// knn_remove.hip — remove_ids (faiss Index::remove_ids): delete rows of a flat index in place.
//
// Every per-row array of a knn_index (xb, xn, the bf16 copy xh / xr, and the split copy xs and the
// int8 copy x8 / x8s / x8r where they have been materialised) is row-major with a fixed row stride
// (knn_kernels.h: the int8 copy's group interleave lives inside a row of i8_row_bytes(nblk) bytes),
// and every derived copy is a pure function of its own fp32 row.  Moving a row's bytes in every array
// therefore leaves the bits a re-derivation would give: no conversion kernel runs again.
//
// Pipeline of one call (remove_rows_locked):
//   1. knn_filter.hip's compaction on the inverted bitmap (compact_rows): the ascending uint32 list
//      src[j] of the surviving rows and their count m, in device memory.
//   2. remove_first_kernel: f = the first j with src[j] != j, the first removed row (src[j] - j never
//      decreases, so a binary search finds it).  Rows before f never move.  m and f reach the host.
//   3. per array, per chunk [j0, j1) of destination rows starting at f: rows_gather_kernel copies
//      the rows src[j0 .. j1) into a bounce buffer, and a device-to-device hipMemcpyAsync puts the
//      bounce buffer at rows [j0, j1), both on the same stream.
//   4. rows [m, old ntotal) of every array are zeroed (the state reserve_rows leaves), ntotal = m, and
//      the maxima are marked stale.
//
// Why in place is safe: src[j] >= j, so the destination rows [j0, j1) of a chunk can overlap only the
// chunk's own source rows src[j0 .. j1) — every later chunk reads rows src[j] >= src[j1] >= j1 only,
// and every earlier chunk's sources are done (stream order).  The bounce buffer covers the overlap
// inside a chunk: the gather finishes before the copy starts.  Nothing depends on the order in which
// workgroups are dispatched.
//
// Memory: the bounce buffer is the index's host-path staging buffer (hq, the 64 MB of knn_add): a
// chunk holds 64 MB / row bytes rows of the array being moved, whatever ntotal is.
// IMGREC_REMOVE_CHUNK=<rows> (tests) fixes the chunk's rows for every array instead.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "knn_index.h"

namespace imgrec {
namespace {

constexpr int kGatherThreads = 256;
constexpr size_t kBounceBytes = size_t(64) << 20;

// dst[(j - j0) * units + c] = base[src[j] * units + c] for j in [j0, j0 + n), c in [0, units): rows
// of `units` elements of V (uint4: 16 B, uint32_t: 4 B).  n * units < 2^32 (a chunk fits the bounce
// buffer).
template <typename V>
__global__ void __launch_bounds__(kGatherThreads)
rows_gather_kernel(const V* __restrict__ base, uint32_t units, const uint32_t* __restrict__ src,
                   uint32_t total, V* __restrict__ dst) {
    const uint32_t u = blockIdx.x * (uint32_t)kGatherThreads + threadIdx.x;
    if (u >= total) return;
    const uint32_t row = u / units, c = u - row * units;
    dst[u] = base[(size_t)src[row] * units + c];
}

// out[1] = the first j < m with list[j] != j, or m (m = out[0], the compaction's count)
__global__ void remove_first_kernel(const uint32_t* __restrict__ list, uint32_t* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t lo = 0, hi = out[0];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list[mid] == mid) lo = mid + 1;
        else hi = mid;
    }
    out[1] = lo;
}

// label -> label - (removed labels below it): word w of `words` holds the removal bits of the labels
// [32 w, 32 w + 32) (0 at and past nbits), pref[w] the set bits of the words before it
__global__ void __launch_bounds__(256)
renumber_labels_kernel(int64_t* __restrict__ lab, int64_t n, const uint32_t* __restrict__ words,
                       const uint32_t* __restrict__ pref, int64_t nbits, int64_t removed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t g = lab[i];
    if (g < 0) return;
    int64_t below = removed;
    if (g < nbits) {
        const int64_t w = g >> 5;
        below = (int64_t)pref[w] + __popc(words[w] & ((1u << (int)(g & 31)) - 1u));
    }
    lab[i] = g - below;
}

// rows src[j0 .. j0 + n) of one array -> its rows [j0, j0 + n), through the bounce buffer
hipError_t move_chunk(char* base, size_t row_bytes, const uint32_t* list, int64_t j0, int64_t n,
                      void* bounce, hipStream_t st) {
    const bool wide = row_bytes % 16 == 0 && (uintptr_t)base % 16 == 0 && (uintptr_t)bounce % 16 == 0;
    const uint32_t units = (uint32_t)(row_bytes / (wide ? 16 : 4));
    const uint32_t total = (uint32_t)n * units;
    const dim3 grid((total + kGatherThreads - 1) / kGatherThreads);
    if (wide)
        hipLaunchKernelGGL(rows_gather_kernel<uint4>, grid, dim3(kGatherThreads), 0, st,
                           reinterpret_cast<const uint4*>(base), units, list + j0, total,
                           reinterpret_cast<uint4*>(bounce));
    else
        hipLaunchKernelGGL(rows_gather_kernel<uint32_t>, grid, dim3(kGatherThreads), 0, st,
                           reinterpret_cast<const uint32_t*>(base), units, list + j0, total,
                           reinterpret_cast<uint32_t*>(bounce));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(base + (size_t)j0 * row_bytes, bounce, (size_t)n * row_bytes,
                          hipMemcpyDeviceToDevice, st);
}

}  // namespace

// The rows of `ix` whose bit is set in the device bitmap leave the index (bit lmap[r] for local row
// r when lmap is given); `extra`, when given, is one more per-row array of 8-byte rows compacted
// with them (a shard's label map).  Waits once on `st` for the survivor count; the moves may still
// run when it returns.
int remove_rows_locked(knn_index* ix, const uint8_t* bits, int64_t nbits, const int64_t* lmap,
                       int64_t* extra, hipStream_t st, int64_t* nremoved) {
    *nremoved = 0;
    if (ix->ntotal == 0 || nbits == 0) return KNN_OK;
    if (ix->ntotal >= (int64_t(1) << 32))
        KNN_FAIL(KNN_EINVAL, "remove_ids: %lld rows in one shard (limit 2^32 - 1)", (long long)ix->ntotal);
    int rc;
    // the count and the first moved row sit side by side: one copy brings both to the host
    if ((rc = ix->ft_m.reserve((size_t)2)) != KNN_OK) return rc;
    if ((rc = ix->rm_h.reserve(2)) != KNN_OK) return rc;
    if ((rc = compact_rows(ix, bits, nbits, lmap, true, st)) != KNN_OK) return rc;
    hipLaunchKernelGGL(remove_first_kernel, dim3(1), dim3(64), 0, st, ix->ft_list, ix->ft_m);
    KNN_HIP(hipGetLastError());
    KNN_HIP(hipMemcpyAsync(ix->rm_h, ix->ft_m, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KNN_HIP(hipStreamSynchronize(st));
    const int64_t old = ix->ntotal, m = (int64_t)ix->rm_h[0], first = (int64_t)ix->rm_h[1];
    if (m > old || first > m) KNN_FAIL(KNN_EHIP, "remove_ids: inconsistent survivor list");
    if (m == old) return KNN_OK;

    // every live corpus column, and the caller's extra array
    struct Arr { char* p; size_t row_bytes; };
    Arr arrs[kCorpusColumns + 1];
    int narr = 0;
    Column<DeviceSpace> cols[kCorpusColumns];
    const int ncols = corpus_columns(ix, cols);
    for (int i = 0; i < ncols; ++i) arrs[narr++] = {(char*)cols[i].buf->data(), cols[i].stride};
    if (extra) arrs[narr++] = {(char*)extra, sizeof(int64_t)};
    size_t max_row = 0;
    for (int i = 0; i < narr; ++i) max_row = std::max(max_row, arrs[i].row_bytes);
    // the knob can only lower a chunk's rows: the buffer never exceeds the staging size
    size_t bounce_bytes = kBounceBytes;
    if (ix->remove_chunk > 0 && (size_t)ix->remove_chunk < kBounceBytes / max_row)
        bounce_bytes = (size_t)ix->remove_chunk * max_row;
    bounce_bytes = std::max(bounce_bytes, max_row);
    if (first < m)
        if ((rc = ix->hq.reserve((bounce_bytes + 3) / 4)) != KNN_OK) return rc;
    for (int i = 0; i < narr; ++i) {
        const Arr& a = arrs[i];
        int64_t chunk = (int64_t)(bounce_bytes / a.row_bytes);
        if (ix->remove_chunk > 0) chunk = std::min(chunk, ix->remove_chunk);
        for (int64_t j0 = first; j0 < m; j0 += chunk)
            KNN_HIP(move_chunk(a.p, a.row_bytes, ix->ft_list, j0, std::min(chunk, m - j0), ix->hq, st));
        KNN_HIP(hipMemsetAsync(a.p + (size_t)m * a.row_bytes, 0, (size_t)(old - m) * a.row_bytes, st));
    }
    ix->ntotal = m;
    ix->xn_max_stale = true;
    *nremoved = old - m;
    return KNN_OK;
}

hipError_t launch_renumber_labels(int64_t* lab, int64_t n, const uint32_t* words, const uint32_t* pref,
                                  int64_t nbits, int64_t removed, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(renumber_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, lab, n,
                       words, pref, nbits, removed);
    return hipGetLastError();
}

}  // namespace imgrec
