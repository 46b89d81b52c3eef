// vladtrain_args_check.cpp — host check of csrc/vladtrain_args.h: the argument checks, the split rule
// of the backward products, the parameter layout and the workspace bound that the entry points of
// include/imgrec_vladtrain.h run before any GPU call (tests/test_vladtrain_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  The index and scratch arrays live in heap blocks of
// exactly the documented size, so a read or write past either end is an AddressSanitizer report; the
// arguments reach the integer extremes, so an overflow in the rules' own arithmetic is a UBSan
// report.  CPU only.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../image_recommender_amd/csrc/vladtrain_args.h"

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

static vladtrain_config good() { return vladtrain_config{0.1, 1e-3, 0.9, 0.999, 1e-8, 1e-5, 2.0, 0.25, 1.5, 1e-5, 0}; }

static int config(const vladtrain_config& c, const char* word) {
    char msg[96];
    std::memset(msg, 0, sizeof msg);
    const int rc = vladtrain_check_config(&c, "t", msg, sizeof msg);
    if (rc != 0 && word && !std::strstr(msg, word)) {
        std::printf("message '%s' lacks '%s'\n", msg, word);
        ++failures;
    }
    return rc;
}

// vladtrain_check_call, then vladtrain_check_sample, as the entry points run them: sample_idx in a
// heap block of exactly k ints and the scratch of exactly n bytes; on success the marks must be the
// sampled rows
static int batch(const void* h, int width, const void* x, int64_t n, const std::vector<int32_t>* idx, int64_t k,
                 const void* losses, const char* word) {
    int32_t* s = nullptr;
    if (idx) {
        s = static_cast<int32_t*>(std::malloc(idx->size() * sizeof(int32_t) + 1));
        std::memcpy(s, idx->data(), idx->size() * sizeof(int32_t));
    }
    char msg[256];
    std::memset(msg, 0, sizeof msg);
    int kout = -1;
    int rc = vladtrain_check_call(h, x, n, s, k, losses, "t", msg, sizeof msg);
    unsigned char* seen = nullptr;
    if (rc == 0) {
        seen = static_cast<unsigned char*>(std::malloc((size_t)n));
        std::memset(seen, 7, (size_t)n);
        rc = vladtrain_check_sample(width, n, s, k, seen, &kout, "t", msg, sizeof msg);
    }
    if (rc == 0) {
        int count = 0;
        for (int64_t i = 0; i < n; ++i) {
            EXPECT(seen[i] == 0 || seen[i] == 1);
            count += seen[i];
        }
        EXPECT(count == kout && kout == (idx ? (int)k : (int)n));
        if (idx)
            for (int64_t q = 0; q < k; ++q) EXPECT(seen[(*idx)[q]] == 1);
    } else if (word && !std::strstr(msg, word)) {
        std::printf("message '%s' lacks '%s'\n", msg, word);
        ++failures;
    }
    std::free(s);
    std::free(seen);
    return rc;
}

// every stage of every split exactly once; the grid and the partial sums within their bounds
static void check_split(int I, int J, int K) {
    const ProdSplit p = vladtrain_split(I, J, K);
    EXPECT(p.ti >= 1 && (int64_t)p.ti * kBN >= I && (int64_t)(p.ti - 1) * kBN < I);
    EXPECT(p.tj >= 1 && (int64_t)p.tj * kBM >= J && (int64_t)(p.tj - 1) * kBM < J);
    EXPECT(p.sp.tiles == p.ti && p.tj <= 65535);
    EXPECT(p.sp.stages >= 1 && (int64_t)p.sp.stages * kBK >= K && (int64_t)(p.sp.stages - 1) * kBK < K);
    EXPECT(p.sp.per >= 1 && p.sp.nsplit >= 1 && p.sp.nsplit <= kEncTargetWgs);
    int64_t next = 0;
    for (int i = 0; i < p.sp.nsplit; ++i) {
        const int64_t s0 = (int64_t)i * p.sp.per, s1 = s0 + p.sp.per < p.sp.stages ? s0 + p.sp.per : p.sp.stages;
        EXPECT(s0 < s1 && s0 * kBK == next);
        next = s1 * kBK;
    }
    EXPECT(next >= K && next - kBK < K);
    EXPECT((int64_t)p.ti * p.tj * p.sp.nsplit <= kEncTargetWgs || p.sp.nsplit == 1);
    EXPECT(vladtrain_part_floats(I, J, K) <= kEncMaxPartFloats);
    EXPECT((vladtrain_part_floats(I, J, K) == 0) == (p.sp.nsplit == 1));
}

// the layout's slots are disjoint, aligned and in order; the workspace total is the sum of its parts
// and within the documented bound
static void check_model(const std::vector<int>& widths, int64_t n) {
    const int nl = (int)widths.size() - 1;
    int64_t off[4 * VLADENC_MAX_LAYERS];
    const int64_t total = vladtrain_layout(nl, widths.data(), off);
    EXPECT(vladtrain_layout(nl, widths.data(), nullptr) == total);
    int64_t at = 0;
    for (int l = 0; l < nl; ++l) {
        const int64_t K = widths[l], N = widths[l + 1];
        const int64_t count[4] = {N * K, N, l < nl - 1 ? N : 0, l < nl - 1 ? N : 0};
        for (int q = 0; q < 4; ++q) {
            EXPECT(off[4 * l + q] == at && at % 4 == 0);
            at += (count[q] + 3) / 4 * 4;
        }
    }
    EXPECT(at == total);
    const TrainSizes s = vladtrain_sizes(nl, widths.data(), n);
    int64_t wmax = 1, hsum = 0;
    for (int l = 1; l <= nl; ++l) {
        if (widths[l] > wmax) wmax = widths[l];
        if (l < nl) hsum += widths[l];
    }
    EXPECT(s.part >= 0 && s.part <= kEncMaxPartFloats);
    EXPECT(s.xt == n * widths[0] && s.xt <= (int64_t)VLADTRAIN_MAX_BATCH_FLOATS);
    EXPECT(s.gram == n * n && s.wide == n * wmax && s.keep == n * (2 * hsum + widths[nl] + 1));
    EXPECT(s.wt <= (int64_t)VLADENC_MAX_WIDTH * VLADENC_MAX_WIDTH);
    EXPECT(s.doubles == n * (2 * nl + 8) + 16);
    const int64_t total_bytes = vladtrain_workspace_total(nl, widths.data(), n);
    // the header's bound: 1 GiB transposed batch, 64 MiB each of G, partial sums and W^T, and per
    // layer at most five n x 4096 float arrays, plus the statistics
    const int64_t bound = 4 * ((int64_t)VLADTRAIN_MAX_BATCH_FLOATS + 3 * kEncMaxPartFloats +
                               (int64_t)VLADTRAIN_MAX_BATCH * VLADENC_MAX_WIDTH * (2 * VLADENC_MAX_LAYERS + 5)) + (1 << 20);
    EXPECT(total_bytes > 0 && total_bytes <= bound);
}

int main() {
    const int imax = std::numeric_limits<int>::max();
    const int64_t i64max = std::numeric_limits<int64_t>::max(), i64min = std::numeric_limits<int64_t>::min();
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    EXPECT(config(good(), nullptr) == 0);
    {
        char msg[64];
        EXPECT(vladtrain_check_config(nullptr, "t", msg, sizeof msg) == -1);
    }
    for (double v : {-0.1, 1.0, 2.0, inf, nan}) { auto c = good(); c.dropout = v; EXPECT(config(c, "dropout") == -1); }
    { auto c = good(); c.dropout = 0.0; EXPECT(config(c, nullptr) == 0); }
    for (double v : {-1e-9, inf, -inf, nan}) { auto c = good(); c.lr = v; EXPECT(config(c, "lr") == -1); }
    for (double v : {-0.1, 1.0, inf, nan}) {
        auto c = good(); c.beta1 = v; EXPECT(config(c, "betas") == -1);
        c = good(); c.beta2 = v; EXPECT(config(c, "betas") == -1);
    }
    for (double v : {0.0, -1.0, inf, nan}) { auto c = good(); c.adam_eps = v; EXPECT(config(c, "adam_eps") == -1); }
    for (double v : {-1e-9, inf, nan}) { auto c = good(); c.weight_decay = v; EXPECT(config(c, "weight_decay") == -1); }
    for (double v : {inf, -inf, nan}) {
        auto c = good(); c.corr_weight = v; EXPECT(config(c, "loss weights") == -1);
        c = good(); c.umap_weight = v; EXPECT(config(c, "loss weights") == -1);
    }
    for (double v : {0.0, -1.5, inf, nan}) { auto c = good(); c.temperature = v; EXPECT(config(c, "temperature") == -1); }
    for (double v : {-1e-9, inf, nan}) { auto c = good(); c.ln_eps = v; EXPECT(config(c, "ln_eps") == -1); }
    {
        char msg[128];
        const int w[4] = {32768, 669, 317, 128};
        const float* three[3] = {P, P, P};
        const float* two[2] = {P, P};
        const vladtrain_config c = good();
        EXPECT(vladtrain_check_create(3, w, three, three, two, two, &c, P, "t", msg, sizeof msg) == 0);
        EXPECT(vladtrain_check_create(3, w, three, three, two, two, nullptr, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladtrain_check_create(0, w, three, three, two, two, &c, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladtrain_check_create(3, w, three, three, nullptr, two, &c, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladtrain_check_create(3, w, three, three, two, two, &c, nullptr, "t", msg, sizeof msg) == -1);
        for (int which : {-1, 4, imax}) EXPECT(vladtrain_check_which(which, false, "t", msg, sizeof msg) == -1);
        for (int which : {0, 1, 2, 3}) EXPECT(vladtrain_check_which(which, false, "t", msg, sizeof msg) == 0);
        EXPECT(vladtrain_check_which(VLADTRAIN_GRADS, true, "t", msg, sizeof msg) == -1);
        EXPECT(vladtrain_check_which(VLADTRAIN_ADAM_V, true, "t", msg, sizeof msg) == 0);
    }

    {
        char msg[128];
        EXPECT(vladtrain_check_product(P, 669, P, 32768, 1024, P, "t", msg, sizeof msg) == 0);
        EXPECT(vladtrain_check_product(P, VLADENC_MAX_WIDTH, P, VLADENC_MAX_IN, VLADENC_MAX_IN, P, "t", msg, sizeof msg) == 0);
        EXPECT(vladtrain_check_product(nullptr, 4, P, 4, 4, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladtrain_check_product(P, 4, nullptr, 4, 4, P, "t", msg, sizeof msg) == -1);
        EXPECT(vladtrain_check_product(P, 4, P, 4, 4, nullptr, "t", msg, sizeof msg) == -1);
        for (int64_t v : {(int64_t)0, (int64_t)-1, (int64_t)VLADENC_MAX_IN + 1, i64max, i64min}) {
            EXPECT(vladtrain_check_product(P, v, P, 4, 4, P, "t", msg, sizeof msg) == -1);
            EXPECT(vladtrain_check_product(P, 4, P, v, 4, P, "t", msg, sizeof msg) == -1);
            EXPECT(vladtrain_check_product(P, 4, P, 4, v, P, "t", msg, sizeof msg) == -1);
        }
        EXPECT(vladtrain_check_product(P, VLADENC_MAX_WIDTH + 1, P, 4, 4, P, "t", msg, sizeof msg) == -1);
    }

    EXPECT(batch(P, 32768, P, 1024, nullptr, 0, P, nullptr) == 0);
    EXPECT(batch(P, 32768, P, 2, nullptr, 0, P, nullptr) == 0);
    EXPECT(batch(P, 32768, P, VLADTRAIN_MAX_BATCH, nullptr, 0, P, nullptr) == 0);
    EXPECT(batch(nullptr, 32768, P, 8, nullptr, 0, P, "NULL handle") == -1);
    EXPECT(batch(P, 32768, nullptr, 8, nullptr, 0, P, "NULL x") == -1);
    EXPECT(batch(P, 32768, P, 8, nullptr, 0, nullptr, "NULL x") == -1);
    for (int64_t n : {(int64_t)1, (int64_t)0, (int64_t)-1, (int64_t)VLADTRAIN_MAX_BATCH + 1, i64max, i64min})
        EXPECT(batch(P, 4, P, n, nullptr, 0, P, "n must be") == -1);
    EXPECT(batch(P, VLADENC_MAX_IN, P, 256, nullptr, 0, P, nullptr) == 0);
    EXPECT(batch(P, VLADENC_MAX_IN, P, 257, nullptr, 0, P, "exceeds") == -1);
    EXPECT(batch(P, imax, P, VLADTRAIN_MAX_BATCH, nullptr, 0, P, "exceeds") == -1);
    {
        const std::vector<int32_t> ok = {5, 0, 7, 2}, twice = {5, 0, 5, 2}, low = {5, -1, 7, 2}, high = {5, 8, 7, 2};
        EXPECT(batch(P, 16, P, 8, &ok, 4, P, nullptr) == 0);
        EXPECT(batch(P, 16, P, 8, &twice, 4, P, "twice") == -1);
        EXPECT(batch(P, 16, P, 8, &low, 4, P, "not a row") == -1);
        EXPECT(batch(P, 16, P, 8, &high, 4, P, "not a row") == -1);
        for (int64_t k : {(int64_t)1, (int64_t)0, (int64_t)-1, (int64_t)9, i64max, i64min})
            EXPECT(batch(P, 16, P, 8, &ok, k, P, "k must be") == -1);
        std::vector<int32_t> all(VLADTRAIN_MAX_BATCH);
        for (int i = 0; i < VLADTRAIN_MAX_BATCH; ++i) all[i] = VLADTRAIN_MAX_BATCH - 1 - i;
        EXPECT(batch(P, 16, P, VLADTRAIN_MAX_BATCH, &all, VLADTRAIN_MAX_BATCH, P, nullptr) == 0);
        const std::vector<int32_t> edge = {std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
        EXPECT(batch(P, 16, P, 8, &edge, 2, P, "not a row") == -1);
    }

    // the split rule: the reference's products, the edges, then samples of the whole range
    {
        const ProdSplit dw0 = vladtrain_split(669, 32768, 1024);          // dW_0 at B = 1024: no depth split
        EXPECT(dw0.ti == 3 && dw0.tj == 256 && dw0.sp.nsplit == 1 && dw0.sp.per == 32);
        EXPECT(vladtrain_split(669, 32768, 32).sp.nsplit == 1);
        const ProdSplit gram = vladtrain_split(1024, 1024, 32768);
        EXPECT(gram.ti == 4 && gram.tj == 8 && gram.sp.nsplit == 16 && gram.sp.per == 64);
        const ProdSplit one = vladtrain_split(1, 1, 1);
        EXPECT(one.ti == 1 && one.tj == 1 && one.sp.nsplit == 1 && one.sp.stages == 1);
    }
    const int edgesIJ[] = {1, 2, 127, 128, 129, 255, 256, 257, 669, 4095, 4096, 32768, VLADENC_MAX_IN};
    const int edgesK[] = {1, 2, 3, 31, 32, 33, 127, 128, 129, 1000, 4095, 4096, 32768, VLADENC_MAX_IN};
    for (int I : edgesIJ)
        for (int J : edgesIJ)
            for (int K : edgesK)
                if (I <= 4096 || J <= 4096) check_split(I, J, K);
    std::mt19937_64 rng(20251);
    for (int it = 0; it < 200000; ++it) {
        const int I = 1 + (int)(rng() % 4096), J = 1 + (int)(rng() % (uint64_t)VLADENC_MAX_IN),
                  K = 1 + (int)(rng() % (uint64_t)VLADENC_MAX_IN);
        check_split(I, J, K);
        check_split(J % 4096 + 1, I, K % 4096 + 1);
    }

    // the layout and the workspace over the argument range
    check_model({32768, 669, 317, 128}, 1024);
    check_model({32768, 669, 317, 128}, VLADTRAIN_MAX_BATCH);
    check_model({70, 3}, 2);
    check_model({VLADENC_MAX_IN, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096}, 256);
    check_model({65536, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096}, VLADTRAIN_MAX_BATCH);
    check_model({1, 1, 1}, 2);
    for (int it = 0; it < 20000; ++it) {
        const int nl = 1 + (int)(rng() % VLADENC_MAX_LAYERS);
        std::vector<int> w(nl + 1);
        w[0] = 1 + (int)(rng() % (uint64_t)VLADENC_MAX_IN);
        for (int l = 1; l <= nl; ++l) w[l] = 1 + (int)(rng() % VLADENC_MAX_WIDTH);
        int64_t nmax = (int64_t)VLADTRAIN_MAX_BATCH_FLOATS / w[0];
        if (nmax > VLADTRAIN_MAX_BATCH) nmax = VLADTRAIN_MAX_BATCH;
        check_model(w, 2 + (int64_t)(rng() % (uint64_t)(nmax - 1)));
    }

    if (failures) {
        std::printf("vladtrain_args_check: %d failures\n", failures);
        return 1;
    }
    std::puts("vladtrain_args_check: ok");
    return 0;
}
