// resize.hip — Pillow's 8-bit LANCZOS resize on gfx950 (include/imgrec_resize.h; the PIL branch
// of the reference's load_image, vector_scripts/create_vector_base.py: Image.resize(size, LANCZOS)).
//
// The arithmetic is integer but for the weight tables, which are built on the HOST in double with
// libm's sin exactly as Pillow builds them (axis_table): a device sin differs in the last bits and
// a rounded weight can flip with it.  One table per distinct (in, out) pair of a call.
//
// Two launches on the caller's stream, none of which waits ("LANCZOS resize"):
//   1. resize_h_kernel<C>  a workgroup per (image, block of <= 8 input rows), across ALL output
//                          columns.  The rows are brought into LDS with 16-byte loads from the
//                          16-byte boundary at or below each row's first byte (any alignment of the
//                          image works, and every input byte leaves HBM once); a thread owns an
//                          output column and keeps rows x channels int32 accumulators, so the
//                          column's weights are fetched once per block (four taps per 16-byte
//                          load) and each meets every row of the block.  The taps come out of LDS
//                          as dwords, realigned by v_alignbyte to the window's first byte.  The tap
//                          loop runs over the column's own count; nothing is sized by ksize.  A row
//                          too long for the LDS budget is read from global memory, a byte at a time.
//                          Writes the uint8 intermediate, or, when the vertical pass is skipped,
//                          the result.
//   2. resize_v_kernel<C>  a workgroup per (image, block of 8 output rows); a thread owns four
//                          consecutive bytes of an output row and walks the row's taps down the
//                          intermediate, eight taps a step (dword loads; L2-resident: the
//                          intermediate of an image is out_w x C bytes wide).  Reads the image itself when the horizontal
//                          pass is skipped, and with both skipped only copies.
// A skipped pass launches no blocks for that image.  No atomics; an output element has one owner
// and a fixed tap order, so results do not depend on the batch.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <map>
#include <utility>
#include <vector>

#include "../../include/imgrec_resize.h"
#include "dev_workspace.h"

namespace imgrec {
namespace {

constexpr int kRNT = 256;
constexpr int kHRows = 8;                 // input rows of a horizontal block (accumulators per channel)
constexpr int kVRows = 8;                 // output rows of a vertical block
constexpr int kVTaps = 8;                 // taps of a vertical step: a table row is a multiple of it
constexpr int kHLds = 48 * 1024;          // LDS budget of a horizontal block
constexpr int kHSlack = 16;               // bytes behind an LDS row that the last step's zero-weight taps may read
constexpr int kPrec = 22;                 // Pillow's PRECISION_BITS = 32 - 8 - 2

// ---- the weight table of one axis (host) ----------------------------------------------------------
// Layout, int32: bounds[out][2] = (xmin, n), padded to a multiple of 4, then k[out][kstride] with
// kstride = ksize rounded up to a multiple of 8 (kVTaps) and zeros behind the n weights: rows start on
// 16 bytes, and a step of 4 (horizontal) or 8 (vertical) taps never leaves its row.
struct AxisShape {
    int ksize, kstride;
    size_t bounds, total;                 // int32 counts
};

double axis_support(int in, int out) {
    const double scale = (double)in / (double)out;
    return 3.0 * (scale < 1.0 ? 1.0 : scale);
}

bool axis_shape(int in, int out, AxisShape* s) {
    const double kd = std::ceil(axis_support(in, out)) * 2.0 + 1.0;
    if (kd > (double)(1 << 28)) return false;
    s->ksize = (int)std::ceil(axis_support(in, out)) * 2 + 1;
    s->kstride = (s->ksize + kVTaps - 1) & ~(kVTaps - 1);
    s->bounds = ((size_t)out * 2 + 3) & ~(size_t)3;
    s->total = s->bounds + (size_t)out * s->kstride;
    return true;
}

inline double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
inline double lanczos_filter(double x) {
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc, statement for statement (no contraction: each
// product and sum rounds on its own).  False when a weight does not fit the kernels' 24-bit multiply.
#pragma clang fp contract(off)
bool axis_table(int in, int out, const AxisShape& s, int32_t* t) {
    const double scale = (double)in / (double)out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> pre((size_t)s.ksize);
    int32_t* const k = t + s.bounds;
    bool fits = true;
    for (size_t i = (size_t)out * 2; i < s.bounds; ++i) t[i] = 0;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = lanczos_filter((x + xmin - center + 0.5) * ss);
            pre[x] = w;
            ww += w;
        }
        int32_t* const row = k + (size_t)xx * s.kstride;
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) pre[x] /= ww;
            const double v = pre[x] * (double)(1 << kPrec);
            row[x] = pre[x] < 0 ? (int32_t)(-0.5 + v) : (int32_t)(0.5 + v);
            if (row[x] >= (1 << 23) || row[x] < -(1 << 23)) fits = false;
        }
        for (int x = xmax; x < s.kstride; ++x) row[x] = 0;
        t[2 * xx] = xmin;
        t[2 * xx + 1] = xmax;
    }
    return fits;
}

inline uint8_t clip8(int32_t acc) {
    const int32_t v = acc >> kPrec;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- device side ----------------------------------------------------------------------------------

struct ImgDesc {                          // 48 bytes, built on the host
    int64_t src;                          // the image's byte offset in the pixel buffer
    int64_t mid;                          // its intermediate's byte offset (both passes run)
    int32_t h, w;
    int32_t htab, vtab;                   // table offsets in int32s; -1: the pass is skipped
    int32_t hks, vks;                     // the tables' kstride
    int32_t hrows;                        // input rows per horizontal block; 0: rows read from global memory
    int32_t lds_stride;                   // bytes between the block's rows in LDS
};
static_assert(sizeof(ImgDesc) == 48, "the staging layout counts on it");

struct ResizeParams {
    const uint8_t* pix;
    const ImgDesc* img;
    const int32_t* hblk;                  // n + 1: first horizontal block of image i (prefix sum)
    const int32_t* vblk;                  // n + 1: first vertical block
    const int32_t* tab;
    uint8_t* mid;
    void* out;
    int n, out_h, out_w, fmt, mid_pitch;
};

// the image whose blocks include b: the last i with first[i] <= b (images without blocks repeat
// their successor's value and are passed over)
__device__ __forceinline__ int find_image(const int32_t* __restrict__ first, int n, int b) {
    int lo = 0, hi = n;                   // first[lo] <= b < first[hi]
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (first[m] <= b) lo = m; else hi = m;
    }
    return lo;
}

__device__ __forceinline__ int clip8_dev(int acc) { return min(max(acc >> kPrec, 0), 255); }

// one result byte of image i at (y, x, c)
template <int C>
__device__ __forceinline__ void store_px(const ResizeParams& p, int i, int y, int x, int c, int v) {
    if (p.fmt == RESIZE_U8_HWC) {
        static_cast<uint8_t*>(p.out)[(((int64_t)i * p.out_h + y) * p.out_w + x) * C + c] = (uint8_t)v;
    } else {
        static_cast<float*>(p.out)[(((int64_t)i * C + c) * p.out_h + y) * p.out_w + x] = __fdiv_rn((float)v, 255.0f);
    }
}

// The taps of one output column over the block's rows, a byte at a time (rows read from global
// memory): row(r) is the address of row r's byte xmin * C.  FULL: all kHRows rows exist; otherwise
// rows >= nr are left alone.
template <int C, bool FULL, class Row>
__device__ __forceinline__ void h_taps(int (&acc)[kHRows][C], Row row, int n, const int4* __restrict__ kv, int nr) {
    for (int j = 0; j < n; j += 4) {
        const int4 w4 = kv[j >> 2];
        const int wq[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (j + q < n) {
#pragma unroll
                for (int r = 0; r < kHRows; ++r) {
                    if (FULL || r < nr) {
                        const uint8_t* s = row(r) + (j + q) * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) acc[r][c] += __mul24(wq[q], (int)s[c]);
                    }
                }
            }
        }
    }
}

// The same taps out of the LDS tile, read as dwords: row r's taps are the byte stream that starts at
// byte s_r = (row's first byte mod 16) + xmin * C of its LDS row; the stream's dwords come from
// consecutive LDS dwords by v_alignbyte (shift s_r & 3), four taps = C stream dwords per step, one
// bit-field extract and one 24-bit multiply-add per byte.  Taps n .. 4 ceil(n / 4) - 1 carry the
// table's zero weights; their bytes lie in the row's slack (kHSlack) and count for nothing.
template <int C, bool FULL>
__device__ __forceinline__ void h_taps_lds(int (&acc)[kHRows][C], const uint32_t* tile32, int ls4, int a0, int rb16,
                                           int xb, int n, const int4* __restrict__ kv, int nr) {
    int idx[kHRows];
    uint32_t sh[kHRows], lo[kHRows];
#pragma unroll
    for (int r = 0; r < kHRows; ++r) {
        const int s = ((a0 + r * rb16) & 15) + xb;
        idx[r] = r * ls4 + (s >> 2);
        sh[r] = (uint32_t)(s & 3);
        lo[r] = (FULL || r < nr) ? tile32[idx[r]] : 0u;
    }
    int4 wn = kv[0];
    for (int j = 0; j < n; j += 4) {
        const int4 w4 = wn;
        wn = kv[(j >> 2) + (j + 4 < n ? 1 : 0)];       // the next step's weights, under this step's work
        const int wq[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int r = 0; r < kHRows; ++r) {
            if (FULL || r < nr) {
                uint32_t st[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const uint32_t hi = tile32[idx[r] + 1 + c];
                    st[c] = __builtin_amdgcn_alignbyte(hi, lo[r], sh[r]);
                    lo[r] = hi;
                }
                idx[r] += C;
#pragma unroll
                for (int m = 0; m < 4 * C; ++m)
                    acc[r][m % C] += __mul24(wq[m / C], (int)((st[m >> 2] >> (8 * (m & 3))) & 0xffu));
            }
        }
    }
}

template <int C>
__global__ void __launch_bounds__(kRNT)
resize_h_kernel(const ResizeParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = find_image(p.hblk, p.n, (int)blockIdx.x);
    const ImgDesc d = p.img[i];
    const bool direct = d.hrows == 0;
    const int R = direct ? kHRows : d.hrows;
    const int y0 = ((int)blockIdx.x - p.hblk[i]) * R;
    const int nr = min(R, d.h - y0);
    const int64_t rowb = (int64_t)d.w * C;
    const uint8_t* const src = p.pix + d.src + (int64_t)y0 * rowb;
    if (!direct) {
        // a wave per row: 16-byte loads from the 16-byte boundary at or below the row's first byte
        // to the one at or above its last (both vectors hold a byte of the image)
        for (int r = wave; r < nr; r += kRNT / 64) {
            const uint8_t* g = src + r * rowb;
            const int al = (int)((uintptr_t)g & 15);
            const uint4* gv = reinterpret_cast<const uint4*>(g - al);
            const int nv = (int)((al + rowb + 15) >> 4);
            uint4* lv = reinterpret_cast<uint4*>(tile + (size_t)r * d.lds_stride);
            for (int v = lane; v < nv; v += 64) lv[v] = gv[v];
        }
        __syncthreads();
    }
    const int32_t* const bounds = p.tab + d.htab;
    const int32_t* const kk = bounds + ((2 * p.out_w + 3) & ~3);
    const bool to_mid = d.vtab >= 0;
    for (int ox = tid; ox < p.out_w; ox += kRNT) {
        const int xmin = bounds[2 * ox], n = bounds[2 * ox + 1];
        const int4* kv = reinterpret_cast<const int4*>(kk + (int64_t)ox * d.hks);
        int acc[kHRows][C];
#pragma unroll
        for (int r = 0; r < kHRows; ++r)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[r][c] = 1 << (kPrec - 1);
        if (direct) {
            const uint8_t* g0 = src + (int64_t)xmin * C;
            auto row = [&](int r) __attribute__((always_inline)) { return g0 + r * rowb; };
            if (nr == kHRows) h_taps<C, true>(acc, row, n, kv, nr);
            else h_taps<C, false>(acc, row, n, kv, nr);
        } else {
            // row r starts (address of its first byte) mod 16 into its LDS row
            const uint32_t* tile32 = reinterpret_cast<const uint32_t*>(tile);
            const int a0 = (int)((uintptr_t)src & 15);
            const int rb16 = (int)(rowb & 15);
            const int ls4 = d.lds_stride >> 2;
            if (nr == kHRows) h_taps_lds<C, true>(acc, tile32, ls4, a0, rb16, xmin * C, n, kv, nr);
            else h_taps_lds<C, false>(acc, tile32, ls4, a0, rb16, xmin * C, n, kv, nr);
        }
#pragma unroll
        for (int r = 0; r < kHRows; ++r) {
            if (r < nr) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int v = clip8_dev(acc[r][c]);
                    if (to_mid) p.mid[d.mid + (int64_t)(y0 + r) * p.mid_pitch + ox * C + c] = (uint8_t)v;
                    else store_px<C>(p, i, y0 + r, ox, c, v);
                }
            }
        }
    }
}

// four bytes at s (nb of them inside the row): one dword when the rows are dword-aligned (the
// dword then holds a byte of the buffer), single bytes otherwise
__device__ __forceinline__ uint32_t load4(const uint8_t* s, bool aligned, int nb) {
    if (aligned) return *reinterpret_cast<const uint32_t*>(s);
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < nb) v |= (uint32_t)s[q] << (8 * q);
    return v;
}

template <int C>
__global__ void __launch_bounds__(kRNT)
resize_v_kernel(const ResizeParams p) {
    const int tid = threadIdx.x;
    const int i = find_image(p.vblk, p.n, (int)blockIdx.x);
    const ImgDesc d = p.img[i];
    const int y0 = ((int)blockIdx.x - p.vblk[i]) * kVRows;
    const int ny = min(kVRows, p.out_h - y0);
    const int rowb = p.out_w * C;
    const int ndw = (rowb + 3) >> 2;
    // the source rows: the intermediate (16-byte pitch) or, with the horizontal pass skipped, the image
    const bool from_mid = d.htab >= 0;
    const uint8_t* const base = from_mid ? p.mid + d.mid : p.pix + d.src;
    const int64_t pitch = from_mid ? p.mid_pitch : rowb;
    const bool aligned = from_mid || ((((uintptr_t)base) | (uintptr_t)pitch) & 3) == 0;
    const bool out_dw = p.fmt == RESIZE_U8_HWC && ((((uintptr_t)p.out) | (uintptr_t)rowb) & 3) == 0;
    const int32_t* const bounds = p.tab + (d.vtab >= 0 ? d.vtab : 0);
    const int32_t* const kk = bounds + ((2 * p.out_h + 3) & ~3);
    for (int item = tid; item < ny * ndw; item += kRNT) {
        const int yy = y0 + item / ndw;
        const int b = 4 * (item % ndw);
        const int nb = min(4, rowb - b);
        int v[4];
        if (d.vtab < 0) {                 // both passes skipped: a copy
            const uint32_t px = load4(base + (int64_t)yy * pitch + b, aligned, nb);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = (int)((px >> (8 * q)) & 0xffu);
        } else {
            const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
            const int32_t* kr = kk + (int64_t)yy * d.vks;
            const uint8_t* s = base + (int64_t)ymin * pitch + b;
            int acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = 1 << (kPrec - 1);
            // kVTaps taps a step, their loads in flight together: taps >= n re-read the last row
            // under the table's zero weights
            for (int j = 0; j < n; j += kVTaps) {
                const int4* kv = reinterpret_cast<const int4*>(kr + j);
                const int4 wa = kv[0], wb = kv[1];
                const int wq[kVTaps] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
                uint32_t px[kVTaps];
#pragma unroll
                for (int u = 0; u < kVTaps; ++u) px[u] = load4(s + (int64_t)min(j + u, n - 1) * pitch, aligned, nb);
#pragma unroll
                for (int u = 0; u < kVTaps; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] += __mul24(wq[u], (int)((px[u] >> (8 * q)) & 0xffu));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = clip8_dev(acc[q]);
        }
        if (out_dw && nb == 4) {
            uint8_t* o = static_cast<uint8_t*>(p.out) + ((int64_t)i * p.out_h + yy) * rowb + b;
            *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nb) store_px<C>(p, i, yy, (b + q) / C, (b + q) % C, v[q]);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------

// what a call's launches share (dev_workspace.h: one per device).  `stage` is the page-locked
// image of `meta` (descriptors, block prefixes, tables); `uploaded` marks the end of the last copy
// out of it, and the next call waits for that event on the host before it rewrites the staging.
struct Workspace : StreamHandoff {
    PinBuf<int32_t> stage;
    DevBuf<int32_t> meta;
    DevBuf<uint8_t> mid;
    hipEvent_t uploaded = nullptr;
    bool pending = false;
};

// `missing`: one of the call's pointers is null
int check_args(bool missing, int64_t n, int channels, int out_h, int out_w, const char* who) {
    if (channels != 1 && channels != 3) KNN_FAIL(KNN_EINVAL, "%s: channels must be 1 or 3, got %d", who, channels);
    if (out_h <= 0 || out_w <= 0) KNN_FAIL(KNN_EINVAL, "%s: output size %d x %d must be positive", who, out_h, out_w);
    if (n < 0) KNN_FAIL(KNN_EINVAL, "%s: n = %lld is negative", who, (long long)n);
    if (n > 0 && missing) KNN_FAIL(KNN_EINVAL, "%s: NULL pointer", who);
    if ((int64_t)out_w * channels > (1 << 28) || (int64_t)out_h > (1 << 28))
        KNN_FAIL(KNN_EINVAL, "%s: output size %d x %d is too large", who, out_h, out_w);
    return KNN_OK;
}

int resize_locked(Workspace* w, const uint8_t* pix, const int64_t* offs, const int32_t* hs, const int32_t* ws,
                  int64_t n, int C, int out_h, int out_w, int fmt, void* out, hipStream_t st) {
    // pass 1: the distinct axes and the staging layout (int32s): descriptors | hblk | vblk | tables
    std::map<std::pair<int, int>, size_t> axes;          // (in, out) -> table offset
    const size_t ndesc = (size_t)n * (sizeof(ImgDesc) / 4);
    const size_t hblk_at = (ndesc + 3) & ~(size_t)3, vblk_at = hblk_at + (((size_t)n + 1 + 3) & ~(size_t)3);
    size_t total = vblk_at + (((size_t)n + 1 + 3) & ~(size_t)3);
    auto axis = [&](int in, int o) -> int64_t {
        if (in == o) return -1;
        const auto key = std::make_pair(in, o);
        auto it = axes.find(key);
        if (it != axes.end()) return (int64_t)it->second;
        AxisShape s;
        if (!axis_shape(in, o, &s) || total + s.total > (size_t)INT32_MAX) return -2;
        axes.emplace(key, total);
        total += s.total;
        return (int64_t)(total - s.total);
    };
    std::vector<ImgDesc> desc((size_t)n);
    std::vector<int32_t> hblk((size_t)n + 1), vblk((size_t)n + 1);
    const int mid_pitch = (out_w * C + 15) & ~15;
    int64_t nh = 0, nv = 0, mid_bytes = 0;
    int lds = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (hs[i] <= 0 || ws[i] <= 0 || offs[i] < 0)
            KNN_FAIL(KNN_EINVAL, "resize_lanczos_device: image %lld has size %d x %d at offset %lld", (long long)i,
                     hs[i], ws[i], (long long)offs[i]);
        if ((int64_t)ws[i] * C > (1 << 30)) KNN_FAIL(KNN_EINVAL, "resize_lanczos_device: image %lld is too wide", (long long)i);
        ImgDesc& d = desc[(size_t)i];
        d = ImgDesc{};
        d.src = offs[i];
        d.h = hs[i];
        d.w = ws[i];
        const int64_t ht = axis(ws[i], out_w), vt = axis(hs[i], out_h);
        if (ht == -2 || vt == -2) KNN_FAIL(KNN_EINVAL, "resize_lanczos_device: the batch's weight tables are too large");
        d.htab = (int32_t)ht;
        d.vtab = (int32_t)vt;
        hblk[(size_t)i] = (int32_t)nh;
        vblk[(size_t)i] = (int32_t)nv;
        if (ht >= 0) {
            const int64_t stride = ((int64_t)ws[i] * C + 15 + kHSlack + 15) & ~(int64_t)15;
            const int rows = (int)std::min<int64_t>(kHRows, kHLds / stride);
            d.hrows = rows;
            d.lds_stride = rows ? (int32_t)stride : 0;
            lds = std::max(lds, rows * (int)d.lds_stride);
            const int per = rows ? rows : kHRows;
            nh += (hs[i] + per - 1) / per;
            if (vt >= 0) {
                d.mid = mid_bytes;
                mid_bytes += (int64_t)hs[i] * mid_pitch;
            }
        }
        if (vt >= 0 || ht < 0) nv += (out_h + kVRows - 1) / kVRows;
        if (nh > INT32_MAX || nv > INT32_MAX) KNN_FAIL(KNN_EINVAL, "resize_lanczos_device: too many blocks");
    }
    hblk[(size_t)n] = (int32_t)nh;
    vblk[(size_t)n] = (int32_t)nv;

    // the staging may still feed the previous call's copy
    if (!w->uploaded) KNN_HIP(hipEventCreateWithFlags(&w->uploaded, hipEventDisableTiming));
    if (w->pending) {
        KNN_HIP(hipEventSynchronize(w->uploaded));
        w->pending = false;
    }
    int rc;
    if ((rc = w->stage.reserve(total)) != KNN_OK) return rc;
    if ((rc = w->meta.reserve(total)) != KNN_OK) return rc;
    if ((rc = w->mid.reserve((size_t)std::max<int64_t>(mid_bytes, 16))) != KNN_OK) return rc;
    int32_t* const sp = w->stage.get();
    for (size_t k = ndesc; k < hblk_at; ++k) sp[k] = 0;
    std::copy(hblk.begin(), hblk.end(), sp + hblk_at);
    std::copy(vblk.begin(), vblk.end(), sp + vblk_at);
    for (const auto& a : axes) {
        AxisShape s;
        axis_shape(a.first.first, a.first.second, &s);
        if (!axis_table(a.first.first, a.first.second, s, sp + a.second))
            KNN_FAIL(KNN_EINVAL, "resize_lanczos_device: a weight of the %d -> %d axis exceeds 24 bits", a.first.first,
                     a.first.second);
    }
    for (int64_t i = 0; i < n; ++i) {
        ImgDesc& d = desc[(size_t)i];
        AxisShape s;
        if (d.htab >= 0) axis_shape(d.w, out_w, &s), d.hks = s.kstride;
        if (d.vtab >= 0) axis_shape(d.h, out_h, &s), d.vks = s.kstride;
    }
    std::copy(reinterpret_cast<const int32_t*>(desc.data()), reinterpret_cast<const int32_t*>(desc.data()) + ndesc, sp);
    KNN_HIP(hipMemcpyAsync(w->meta.get(), sp, total * sizeof(int32_t), hipMemcpyHostToDevice, st));
    w->pending = true;                     // (a failed record below leaves the wait to the next call's event sync)
    KNN_HIP(hipEventRecord(w->uploaded, st));

    ResizeParams p;
    p.pix = pix;
    p.img = reinterpret_cast<const ImgDesc*>(w->meta.get());
    p.hblk = w->meta.get() + hblk_at;
    p.vblk = w->meta.get() + vblk_at;
    p.tab = w->meta.get();
    p.mid = w->mid.get();
    p.out = out;
    p.n = (int)n;
    p.out_h = out_h;
    p.out_w = out_w;
    p.fmt = fmt;
    p.mid_pitch = mid_pitch;
    if (nh > 0) {
        if (C == 3) hipLaunchKernelGGL(resize_h_kernel<3>, dim3((unsigned)nh), dim3(kRNT), (size_t)lds, st, p);
        else hipLaunchKernelGGL(resize_h_kernel<1>, dim3((unsigned)nh), dim3(kRNT), (size_t)lds, st, p);
        KNN_HIP(hipGetLastError());
    }
    if (nv > 0) {
        if (C == 3) hipLaunchKernelGGL(resize_v_kernel<3>, dim3((unsigned)nv), dim3(kRNT), 0, st, p);
        else hipLaunchKernelGGL(resize_v_kernel<1>, dim3((unsigned)nv), dim3(kRNT), 0, st, p);
        KNN_HIP(hipGetLastError());
    }
    return KNN_OK;
}

// one pass of the host statement: `lines` lines of `in` pixels (pixel stride ps, line stride ls) ->
// `out` pixels each
void host_pass(const uint8_t* src, int64_t ps, int64_t ls, uint8_t* dst, int64_t dps, int64_t dls, int lines, int in,
               int out, int C) {
    AxisShape s;
    axis_shape(in, out, &s);
    std::vector<int32_t> t(s.total);
    axis_table(in, out, s, t.data());
    const int32_t* k = t.data() + s.bounds;
    for (int l = 0; l < lines; ++l)
        for (int xx = 0; xx < out; ++xx) {
            const int xmin = t[2 * xx], n = t[2 * xx + 1];
            for (int c = 0; c < C; ++c) {
                int32_t acc = 1 << (kPrec - 1);
                for (int j = 0; j < n; ++j) acc += (int32_t)src[l * ls + (xmin + j) * ps + c] * k[(size_t)xx * s.kstride + j];
                dst[l * dls + xx * dps + c] = clip8(acc);
            }
        }
}

}  // namespace
}  // namespace imgrec

using namespace imgrec;

extern "C" {

const char* resize_last_error(void) { return knn_last_error(); }

int resize_lanczos_host(const uint8_t* pixels, int h, int w, int channels, int out_h, int out_w, uint8_t* out_u8) {
    const int rc = check_args(!pixels || !out_u8, 1, channels, out_h, out_w, "resize_lanczos_host");
    if (rc != KNN_OK) return rc;
    if (h <= 0 || w <= 0) KNN_FAIL(KNN_EINVAL, "resize_lanczos_host: input size %d x %d must be positive", h, w);
    AxisShape s;
    if (!axis_shape(w, out_w, &s) || !axis_shape(h, out_h, &s))
        KNN_FAIL(KNN_EINVAL, "resize_lanczos_host: %d x %d -> %d x %d needs too many taps", h, w, out_h, out_w);
    const int C = channels;
    const uint8_t* cur = pixels;
    std::vector<uint8_t> mid;
    if (w != out_w) {                      // horizontal first, over every input row, rounded to uint8
        uint8_t* dst = out_u8;
        if (h != out_h) {
            mid.resize((size_t)h * out_w * C);
            dst = mid.data();
        }
        host_pass(cur, C, (int64_t)w * C, dst, C, (int64_t)out_w * C, h, w, out_w, C);
        cur = dst;
    }
    if (h != out_h) {                      // vertical: a "line" is a column
        host_pass(cur, (int64_t)out_w * C, C, out_u8, (int64_t)out_w * C, C, out_w, h, out_h, C);
    } else if (w == out_w) {
        std::copy(pixels, pixels + (size_t)h * w * C, out_u8);
    }
    return KNN_OK;
}

int resize_lanczos_device(const uint8_t* dev_pixels, const int64_t* host_offsets, const int32_t* host_heights,
                          const int32_t* host_widths, int64_t n, int channels, int out_h, int out_w, int format,
                          void* dev_out, void* stream) {
    int rc = check_args(!dev_pixels || !host_offsets || !host_heights || !host_widths || !dev_out, n, channels, out_h,
                        out_w, "resize_lanczos_device");
    if (rc != KNN_OK) return rc;
    if (format != RESIZE_U8_HWC && format != RESIZE_F32_CHW)
        KNN_FAIL(KNN_EINVAL, "resize_lanczos_device: unknown format %d", format);
    if (n > (1 << 24)) KNN_FAIL(KNN_EINVAL, "resize_lanczos_device: n = %lld is too large", (long long)n);
    if (n == 0) return KNN_OK;
    if ((rc = have_device()) != KNN_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    return on_workspace<Workspace>(st, [&](Workspace* w) {
        return resize_locked(w, dev_pixels, host_offsets, host_heights, host_widths, n, channels, out_h, out_w, format,
                             dev_out, st);
    });
}

}  // extern "C"
