// vladenc_args_check.cpp — host check of csrc/vladenc_args.h: the argument checks, the depth split
// rule and the chunk rule that the entry points of include/imgrec_vladenc.h run before any GPU call
// (tests/test_vladenc_cpu.py builds it with -fsanitize=address,undefined and runs it).  The width
// and pointer arrays live in heap blocks of exactly the documented size, so a read past either end
// is an AddressSanitizer report; the arguments reach the integer extremes, so an overflow in the
// rules' own arithmetic is a UBSan report.  CPU only.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../image_recommender_amd/csrc/vladenc_args.h"

using namespace imgrec;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #cond);                  \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static const float* const P = reinterpret_cast<const float*>(4096);     // never dereferenced

// vladenc_check_create over exactly-sized heap arrays: widths[nw], W/b[np], gamma/beta[ng]
static int create(int nlayers, const std::vector<int>& widths, int np, int ng, float eps, const char* word,
                  int null_w = -1, int null_g = -1) {
    int* w = static_cast<int*>(std::malloc(widths.size() * sizeof(int) + 1));
    std::memcpy(w, widths.data(), widths.size() * sizeof(int));
    auto ptrs = [](int n, int null_at) {
        const float** p = static_cast<const float**>(std::malloc((size_t)n * sizeof(float*) + 1));
        for (int i = 0; i < n; ++i) p[i] = i == null_at ? nullptr : P;
        return p;
    };
    const float** W = ptrs(np, null_w);
    const float** b = ptrs(np, -1);
    const float** g = ptrs(ng, null_g);
    const float** be = ptrs(ng, -1);
    char msg[96];                      // a short buffer: the message is cut, never overrun
    std::memset(msg, 0, sizeof msg);
    const int rc = vladenc_check_create(nlayers, w, W, b, g, be, eps, P, "t", msg, sizeof msg);
    std::free(w); std::free(W); std::free(b); std::free(g); std::free(be);
    if (rc != 0 && word && !std::strstr(msg, word)) {
        std::printf("message '%s' lacks '%s'\n", msg, word);
        ++failures;
    }
    return rc;
}

static int forward(const void* h, const void* x, int64_t n, int flags, const void* out, const char* word) {
    char msg[256];
    std::memset(msg, 0, sizeof msg);
    const int rc = vladenc_check_forward(h, x, n, flags, out, "t", msg, sizeof msg);
    if (rc != 0 && word && !std::strstr(msg, word)) {
        std::printf("message '%s' lacks '%s'\n", msg, word);
        ++failures;
    }
    return rc;
}

// every stage of every split, exactly once, in order; the grid and the workspace within their bounds
static void check_split(int K, int N) {
    const EncSplit s = vladenc_split(K, N);
    const EncSplit again = vladenc_split(K, N);
    EXPECT(s.tiles == again.tiles && s.stages == again.stages && s.per == again.per && s.nsplit == again.nsplit);
    EXPECT(s.tiles >= 1 && (int64_t)s.tiles * kBN >= N && (int64_t)(s.tiles - 1) * kBN < N);
    EXPECT(s.stages >= 1 && (int64_t)s.stages * kBK >= K && (int64_t)(s.stages - 1) * kBK < K);
    EXPECT(s.per >= 1 && s.nsplit >= 1 && s.nsplit <= 65535);
    int64_t next = 0;                                    // the first depth column not yet covered
    for (int i = 0; i < s.nsplit; ++i) {
        const int64_t s0 = (int64_t)i * s.per, s1 = s0 + s.per < s.stages ? s0 + s.per : s.stages;
        EXPECT(s0 < s1);                                 // no empty split
        EXPECT(s0 * kBK == next);
        next = s1 * kBK;
    }
    EXPECT(next >= K && next - kBK < K);
    EXPECT((int64_t)s.tiles * s.nsplit <= kEncTargetWgs || s.nsplit == 1);
    // the workspace bound, for every chunk the knob can ask for, whatever n: a layer's rows per
    // launch are whole row tiles (or the chunk) and their partial sums fit
    for (long long knob : {0LL, 1LL, 64LL, 100LL, 128LL, 129LL, -5LL, 1LL << 40}) {
        const int chunk = vladenc_chunk_rows(knob);
        EXPECT(vladenc_knob_set(knob) == (knob >= 1 && knob <= VLADENC_CHUNK_ROWS));
        EXPECT(chunk == (vladenc_knob_set(knob) ? (int)knob : VLADENC_SUPER_ROWS));
        for (int c : {chunk, 1, 129, chunk / 2 + 1}) {       // (a batch smaller than the chunk caps it)
            const int rows = vladenc_layer_rows(K, N, c);
            EXPECT(rows >= 1 && rows <= c && (rows == c || rows % VLADENC_CHUNK_ROWS == 0));
            if (N <= VLADENC_MAX_WIDTH) EXPECT(vladenc_part_floats(K, N, rows) <= kEncMaxPartFloats);
        }
    }
}

int main() {
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    const int64_t i64max = std::numeric_limits<int64_t>::max(), i64min = std::numeric_limits<int64_t>::min();
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    EXPECT(create(3, {32768, 669, 317, 128}, 3, 2, 1e-5f, nullptr) == 0);
    EXPECT(create(1, {70, 3}, 1, 0, 1e-5f, nullptr) == 0);
    EXPECT(create(8, {VLADENC_MAX_IN, 4096, 1, 2, 3, 4, 5, 6, 4096}, 8, 7, 0.f, nullptr) == 0);
    for (int nl : {0, -1, 9, imax, imin}) EXPECT(create(nl, {4, 4}, 1, 0, 1e-5f, "nlayers") == -1);
    EXPECT(create(2, {4, 0, 4}, 2, 1, 1e-5f, "widths[1]") == -1);
    EXPECT(create(2, {0, 4, 4}, 2, 1, 1e-5f, "widths[0]") == -1);
    EXPECT(create(2, {4, 4, imin}, 2, 1, 1e-5f, "widths[2]") == -1);
    EXPECT(create(2, {4, 4097, 4}, 2, 1, 1e-5f, "widths[1]") == -1);
    EXPECT(create(2, {4, 4, 4097}, 2, 1, 1e-5f, "widths[2]") == -1);
    EXPECT(create(2, {VLADENC_MAX_IN + 1, 4, 4}, 2, 1, 1e-5f, "widths[0]") == -1);
    EXPECT(create(2, {4097, 4, 4}, 2, 1, 1e-5f, nullptr) == 0);            // the input may be wider
    EXPECT(create(2, {4, 4, 4}, 2, 1, 1e-5f, "NULL", 1) == -1);
    EXPECT(create(3, {4, 4, 4, 4}, 3, 2, 1e-5f, "NULL", -1, 1) == -1);
    for (float e : {-1e-9f, -1.f, inf, -inf, nan, 1e30f}) EXPECT(create(1, {4, 4}, 1, 0, e, "ln_eps") == -1);
    {
        char msg[128];
        const int w[2] = {4, 4};
        const float* one[1] = {P};
        EXPECT(vladenc_check_create(1, nullptr, one, one, nullptr, nullptr, 1e-5f, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladenc_check_create(1, w, nullptr, one, nullptr, nullptr, 1e-5f, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladenc_check_create(1, w, one, nullptr, nullptr, nullptr, 1e-5f, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladenc_check_create(1, w, one, one, nullptr, nullptr, 1e-5f, nullptr, "t", msg, sizeof msg) == -1);
        EXPECT(vladenc_check_create(1, w, one, one, nullptr, nullptr, 1e-5f, P, "t", msg, sizeof msg) == 0);
        const int w3[3] = {4, 4, 4};
        const float* two[2] = {P, P};
        EXPECT(vladenc_check_create(2, w3, two, two, nullptr, one, 1e-5f, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladenc_check_create(2, w3, two, two, one, nullptr, 1e-5f, P, "t", msg, sizeof msg) == -1);
    }

    EXPECT(forward(P, P, 10, 0, P, nullptr) == 0);
    EXPECT(forward(P, P, 10, VLADENC_MODEL_OUTPUT, P, nullptr) == 0);
    EXPECT(forward(P, nullptr, 0, 0, nullptr, nullptr) == 0);
    EXPECT(forward(nullptr, P, 10, 0, P, "NULL handle") == -1);
    EXPECT(forward(P, nullptr, 10, 0, P, "NULL x") == -1);
    EXPECT(forward(P, P, 10, 0, nullptr, "NULL x") == -1);
    for (int f : {2, 3, -1, imin, imax}) EXPECT(forward(P, P, 10, f, P, "flags") == -1);
    for (int64_t n : {(int64_t)-1, (int64_t)1 << 31, i64max, i64min}) EXPECT(forward(P, P, n, 0, P, "2^31") == -1);
    EXPECT(forward(P, P, ((int64_t)1 << 31) - 1, 0, P, nullptr) == 0);

    // the split rule: the reference's layers, the edges, then samples of the whole range
    {
        const EncSplit s = vladenc_split(32768, 669);
        EXPECT(s.tiles == 3 && s.stages == 1024 && s.per == 7 && s.nsplit == 147);
        const EncSplit t = vladenc_split(669, 317);
        EXPECT(t.tiles == 2 && t.stages == 21 && t.per == 5 && t.nsplit == 5);
        const EncSplit u = vladenc_split(1, 1);
        EXPECT(u.tiles == 1 && u.stages == 1 && u.per == 1 && u.nsplit == 1);
    }
    const int edgesK[] = {1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1023, 1024, 1025,
                          32767, 32768, 32769, VLADENC_MAX_IN - 33, VLADENC_MAX_IN - 1, VLADENC_MAX_IN};
    const int edgesN[] = {1, 2, 31, 32, 33, 255, 256, 257, 317, 511, 512, 513, 669, 4095, 4096};
    for (int K : edgesK)
        for (int N : edgesN) check_split(K, N);
    for (int K = 1; K <= 4200; ++K) check_split(K, 1 + K % 700);
    std::mt19937_64 rng(20250);
    for (int it = 0; it < 200000; ++it) {
        const int K = 1 + (int)(rng() % (uint64_t)VLADENC_MAX_IN), N = 1 + (int)(rng() % (uint64_t)VLADENC_MAX_WIDTH);
        check_split(K, N);
    }
    // the chunks of any n, and a layer's launches inside a chunk, cover the rows exactly once
    for (long long knob : {0LL, 1LL, 64LL, 100LL, 128LL}) {
        const int chunk = vladenc_chunk_rows(knob);
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)127, (int64_t)128, (int64_t)129, (int64_t)1000, (int64_t)5000}) {
            int64_t covered = 0;
            for (int64_t c0 = 0; c0 < n; c0 += chunk) {
                const int M = (int)(chunk < n - c0 ? chunk : n - c0), rows = vladenc_layer_rows(32768, 669, M);
                for (int r0 = 0; r0 < M; r0 += rows) covered += (rows < M - r0 ? rows : M - r0);
            }
            EXPECT(covered == n);
        }
    }
    EXPECT(vladenc_layer_rows(32768, 669, VLADENC_SUPER_ROWS) == 128 && vladenc_layer_rows(669, 317, VLADENC_SUPER_ROWS) == VLADENC_SUPER_ROWS);

    if (failures) {
        std::printf("vladenc_args_check: %d failures\n", failures);
        return 1;
    }
    std::puts("vladenc_args_check: ok");
    return 0;
}
