// vlad_args_check.cpp — host check of csrc/vlad_args.h, the argument, offsets and tiling checks
// that vlad_encode / vlad_encode_device (include/imgrec_vlad.h) run before any GPU call
// (tests/test_vlad_cpu.py builds it with -fsanitize=address,undefined and runs it).  Every offsets
// array lives in a heap block of exactly nimg + 1 entries, so a read past either end is an
// AddressSanitizer report; the random arguments reach the integer extremes, so an overflow in the
// checks' own arithmetic is a UBSan report.  CPU only.

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../image_recommender_amd/csrc/vlad_args.h"

using namespace imgrec;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #cond);                  \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static const void* const P = reinterpret_cast<const void*>(4096);     // never dereferenced

static VladArgs good() { return VladArgs{P, 10, P, 2, 128, P, 256, 4, 125.0f, 0, P}; }

static int args(const VladArgs& a, const char* word) {
    char msg[256];
    std::memset(msg, 0, sizeof msg);
    const int rc = vlad_check_args(a, "t", msg, sizeof msg);
    if (rc != 0 && word && !std::strstr(msg, word)) {
        std::printf("message '%s' lacks '%s'\n", msg, word);
        ++failures;
    }
    return rc;
}

// offsets in an exactly-sized heap block
static int offsets(const std::vector<int64_t>& v, int64_t N, const char* word) {
    int64_t* p = static_cast<int64_t*>(std::malloc(v.size() * sizeof(int64_t)));
    std::memcpy(p, v.data(), v.size() * sizeof(int64_t));
    char msg[64];                      // a short buffer: the message is cut, never overrun
    std::memset(msg, 0, sizeof msg);
    const int rc = vlad_check_offsets(p, (int64_t)v.size() - 1, N, "t", msg, sizeof msg);
    std::free(p);
    if (rc != 0 && word && !std::strstr(msg, word)) {
        std::printf("message '%s' lacks '%s'\n", msg, word);
        ++failures;
    }
    return rc;
}

int main() {
    const int64_t i64max = std::numeric_limits<int64_t>::max(), i64min = std::numeric_limits<int64_t>::min();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    VladArgs a = good();
    EXPECT(args(a, nullptr) == 0);
    a = good(); a.x = nullptr; EXPECT(args(a, "NULL") == -1);
    a = good(); a.x = nullptr; a.N = 0; EXPECT(args(a, nullptr) == 0);
    a = good(); a.offsets = nullptr; EXPECT(args(a, "NULL") == -1);
    a = good(); a.codebook = nullptr; EXPECT(args(a, "NULL") == -1);
    a = good(); a.vlad = nullptr; EXPECT(args(a, "NULL") == -1);
    a = good(); a.vlad = nullptr; a.nimg = 0; EXPECT(args(a, nullptr) == 0);
    for (int nn : {0, -1, 9, imax, imin}) { a = good(); a.nn = nn; EXPECT(args(a, "nn must be") == -1); }
    for (int nn = 1; nn <= VLAD_MAX_NN; ++nn) { a = good(); a.nn = nn; EXPECT(args(a, nullptr) == 0); }
    a = good(); a.k = 3; EXPECT(args(a, "exceeds") == -1);
    a = good(); a.k = 4; EXPECT(args(a, nullptr) == 0);
    for (int k : {0, -5, imin}) { a = good(); a.k = k; EXPECT(args(a, "k must be") == -1); }
    a = good(); a.k = imax; EXPECT(args(a, nullptr) == 0);
    a = good(); a.k = imax; a.d = VLAD_MAX_D; EXPECT(args(a, "too large") == -1);
    for (int d : {0, -1, VLAD_MAX_D + 1, imax, imin}) { a = good(); a.d = d; EXPECT(args(a, "d must be") == -1); }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float s : {0.f, -0.f, -1.f, inf, -inf, nan, 1e30f}) { a = good(); a.sigma = s; EXPECT(args(a, "sigma") == -1); }
    for (float s : {1e-30f, 0.5f, 125.f, 1e18f}) { a = good(); a.sigma = s; EXPECT(args(a, nullptr) == 0); }
    for (int f : {2, 3, -1, imin}) { a = good(); a.flags = f; EXPECT(args(a, "flags") == -1); }
    a = good(); a.flags = VLAD_RAW; EXPECT(args(a, nullptr) == 0);
    for (int64_t n : {(int64_t)-1, (int64_t)1 << 31, i64max, i64min}) {
        a = good(); a.N = n; EXPECT(args(a, "2^31") == -1);
        a = good(); a.nimg = n; EXPECT(args(a, "2^31") == -1);
    }
    a = good(); a.N = ((int64_t)1 << 31) - 1; a.nimg = a.N; EXPECT(args(a, nullptr) == 0);

    EXPECT(offsets({0}, 0, nullptr) == 0);
    EXPECT(offsets({0, 0, 0}, 0, nullptr) == 0);
    EXPECT(offsets({0, 1, 4, 4, 10}, 10, nullptr) == 0);
    EXPECT(offsets({1, 4, 10}, 10, "offsets[0]") == -1);
    EXPECT(offsets({-1, 4, 10}, 10, "offsets[0]") == -1);
    EXPECT(offsets({0, 5, 4, 10}, 10, "decrease") == -1);
    EXPECT(offsets({0, 11, 10}, 10, "decrease") == -1);
    EXPECT(offsets({0, i64max, i64min, 10}, 10, "decrease") == -1);
    EXPECT(offsets({0, 4, 9}, 10, "offsets[nimg]") == -1);
    EXPECT(offsets({0, 4, i64max}, 10, "offsets[nimg]") == -1);
    EXPECT(offsets({0}, 3, "offsets[nimg]") == -1);

    char msg[256];
    int ct = 0;
    int64_t nt = 0;
    EXPECT(vlad_cluster_tile(256, 128, kVladAccFloats, 512, &ct, &nt, "t", msg, sizeof msg) == 0 && ct == 256 && nt == 1);
    EXPECT(vlad_cluster_tile(300, 48, kVladAccFloats, 1, &ct, &nt, "t", msg, sizeof msg) == 0 && ct == 300 && nt == 1);
    EXPECT(vlad_cluster_tile(256, 128, 1000, 1, &ct, &nt, "t", msg, sizeof msg) == 0 && ct == 7 && nt == 37);
    EXPECT(vlad_cluster_tile(5, VLAD_MAX_D, 1, 1, &ct, &nt, "t", msg, sizeof msg) == 0 && ct == 1 && nt == 5);
    EXPECT(vlad_cluster_tile(imax, VLAD_MAX_D, kVladAccFloats, 1, &ct, &nt, "t", msg, sizeof msg) == 0 && ct == 2);
    EXPECT(vlad_cluster_tile(imax, VLAD_MAX_D, kVladAccFloats, ((int64_t)1 << 31) - 1, &ct, &nt, "t", msg, sizeof msg) == -1);

    // random arguments, the extremes included: a verdict is reached without UB, an accepted set is
    // within the documented limits, and the tile of an accepted set fits the accumulator
    std::mt19937_64 rng(20240);
    auto pick_int = [&](std::initializer_list<int> edge) {
        const uint64_t r = rng();
        if (r % 3 == 0) return *(edge.begin() + (r >> 8) % edge.size());
        return (int)((r >> 8) % 40000) - 100;
    };
    int accepted = 0;
    for (int it = 0; it < 200000; ++it) {
        VladArgs r = good();
        r.d = pick_int({0, 1, VLAD_MAX_D, VLAD_MAX_D + 1, imax, imin});
        r.k = pick_int({0, 1, 8, imax, imin});
        r.nn = pick_int({0, 1, 8, 9, imax, imin}) % 16;
        r.flags = (int)(rng() % 4) - 1;
        r.N = (rng() % 4 == 0) ? (int64_t)rng() : (int64_t)(rng() % 5000) - 3;
        r.nimg = (rng() % 4 == 0) ? (int64_t)rng() : (int64_t)(rng() % 5000) - 3;
        const float sig[] = {0.f, -1.f, 0.5f, 125.f, inf, nan};
        r.sigma = sig[rng() % 6];
        if (vlad_check_args(r, "t", msg, sizeof msg) != 0) continue;
        ++accepted;
        EXPECT(r.d >= 1 && r.d <= VLAD_MAX_D && r.k >= 1 && r.nn >= 1 && r.nn <= VLAD_MAX_NN && r.nn <= r.k);
        EXPECT(r.N >= 0 && r.N < ((int64_t)1 << 31) && r.nimg >= 0 && r.nimg < ((int64_t)1 << 31));
        EXPECT(r.sigma > 0.f && (r.flags & ~VLAD_RAW) == 0);
        const int64_t budget = 1 + (int64_t)(rng() % (uint64_t)kVladAccFloats);
        if (vlad_cluster_tile(r.k, r.d, budget, r.nimg, &ct, &nt, "t", msg, sizeof msg) != 0) continue;
        EXPECT(ct >= 1 && ct <= r.k && nt * ct >= r.k && (nt - 1) * ct < r.k);
        EXPECT(ct == 1 || (int64_t)ct * r.d <= budget);
        EXPECT(r.nimg * nt < ((int64_t)1 << 31));
    }
    EXPECT(accepted > 1000);

    // random offsets: a sorted array passes, one inversion anywhere is found
    for (int it = 0; it < 2000; ++it) {
        const int nimg = (int)(rng() % 40);
        std::vector<int64_t> off(nimg + 1, 0);
        for (int i = 1; i <= nimg; ++i) off[i] = off[i - 1] + (int64_t)(rng() % 4 == 0 ? 0 : rng() % 1000);
        EXPECT(offsets(off, off[nimg], nullptr) == 0);
        if (nimg >= 2) {
            const int i = 1 + (int)(rng() % (nimg - 1));
            std::vector<int64_t> bad = off;
            bad[i] = bad[i + 1] + 1;
            EXPECT(offsets(bad, off[nimg], nullptr) == -1);
        }
    }

    if (failures) {
        std::printf("vlad_args_check: %d failures\n", failures);
        return 1;
    }
    std::puts("vlad_args_check: ok");
    return 0;
}
