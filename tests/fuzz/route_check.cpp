// route_check.cpp — host check of csrc/knn_plan.h choose_route (tests/test_route_cpu.py builds it with
// knn_plan.cpp under -fsanitize=address,undefined and runs it on tests/golden/route_table.bin).
// Every output of choose_route — route, tail_ok, i8_inst and the Plan — over a grid that crosses
// every threshold of the decision must equal the recorded table, which was taken from the former
// use_i8 -> use_b16 -> use_split ladder (tools/route_table_gen.py: format and provenance), not from
// choose_route.  No tolerance: any difference names its slice (or row) and fails the run.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../image_recommender_amd/csrc/knn_plan.h"

using namespace imgrec;

namespace {

using Words = std::vector<int32_t>;

// (448 / 512 and 1088 / 1408: 7 / 8 and 17 / 22 blocks of 64, next to kI8MinBlocks and i8_wins_8q's ends)
const Words kD = {48,  63,   64,   128,  255,  256,  448,  512,  768,  832,  896,
                  1024, 1088, 1280, 1408, 1472, 1536, 1968, 4096, 4160, 16448};
const Words kNtotal = {0, 1, 255, 1000, 16383, 16384, 131072, 1000000, 10000000};
const Words kNq = {1, 2, 3, 4, 5, 8, 9, 32, 33, 128, 129, kB16BigMinQ - 1, kB16BigMinQ, 1024, 8192};
const Words kK = {1, 8, 9, 10, 11, 16, 17, 32};
const Words kModes = {KNN_SEARCH_AUTO, KNN_SEARCH_EXACT, KNN_SEARCH_SPLIT, KNN_SEARCH_BF16, KNN_SEARCH_I8};
const Words kCus = {256, 32, 8}, kWgpcu = {0, 1}, kKnob = {1, 0}, kState = {0, 1, 2}, kFullD = {768, 1968};
const TailCopy kTailCopy[] = {TailCopy::Undecided, TailCopy::Built, TailCopy::Ineligible};

constexpr int kValues = 16;
constexpr int32_t kMagic = 0x31425452;      // "RTB1"

uint64_t fnv(uint64_t h, int v) {
    for (int i = 0; i < 4; ++i) { h ^= (uint32_t(v) >> (8 * i)) & 0xff; h *= 1099511628211ull; }
    return h;
}

// create_single's shape of a d-column index (knn_capi.cpp)
IndexShape shape_of(int d) {
    IndexShape s;
    const int pad = d >= 256 ? 2 * kDepthPad : kDepthPad;
    s.d = d;
    s.dp = (d + pad - 1) / pad * pad;
    s.split_ok = s.dp % 32 == 0 && d >= 256;
    s.b16_ok = d >= 64;
    s.dpb = (d + kB16Pad - 1) / kB16Pad * kB16Pad;
    s.nblk8 = d >= 64 && d <= 4096 ? (d + 63) / 64 : 0;
    return s;
}

std::string text(const Words& w) {
    std::string s;
    for (int32_t x : w) s += (s.empty() ? "" : " ") + std::to_string(x);
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: route_check <route_table.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    Words w(bytes.size() / 4);
    std::memcpy(w.data(), bytes.data(), w.size() * 4);
    // header: magic, the revision (12 characters), the ten grids' lengths; then the grids, the
    // slices' digests (low, high word) and the spelled-out rows' values, both in the loops' order
    const Words* grid[] = {&kD, &kModes, &kCus, &kWgpcu, &kKnob, &kState, &kNtotal, &kNq, &kK, &kFullD};
    const char* grid_name[] = {"d", "mode", "cus", "wgpcu", "knob", "state", "ntotal", "nq", "k", "spelled-out d"};
    size_t at = 14, want = 14;
    if (w.size() < at || w[0] != kMagic) { std::fprintf(stderr, "route_check: %s is no route table\n", argv[1]); return 2; }
    for (int g = 0; g < 10; ++g) want += grid[g]->size();
    const size_t n_inner = kNtotal.size() * kNq.size() * kK.size();
    const size_t n_slices = kD.size() * kModes.size() * kCus.size() * kWgpcu.size() * kKnob.size() * kState.size();
    const size_t slice0 = want, row0 = slice0 + 2 * n_slices;
    want = row0 + kFullD.size() * n_inner * kValues;
    int bad = 0;
    auto expect = [&](const std::string& what, const std::string& got, const std::string& table) {
        if (got != table && ++bad <= 20)
            std::fprintf(stderr, "route_check: %s: got [%s], table [%s]\n", what.c_str(), got.c_str(), table.c_str());
    };
    // the table covers this program's grid, no other
    for (int g = 0; g < 10 && at < w.size(); ++g) {
        const size_t n = std::min<size_t>(w[4 + g], w.size() - at);
        expect(std::string("grid ") + grid_name[g], text(*grid[g]), text(Words(w.begin() + at, w.begin() + at + n)));
        at += n;
    }
    expect("table size in words", std::to_string(want), std::to_string(w.size()));
    if (bad) return 1;      // (another grid: the digests below would index it wrongly)
    size_t nslices = 0, nrows = 0;
    for (int d : kD) for (int mode : kModes) for (int cus : kCus) for (int wg : kWgpcu) for (int knob : kKnob)
    for (int st : kState) {
        IndexShape ix = shape_of(d);
        ix.mode = mode; ix.cus = cus; ix.i8_wgpcu = wg; ix.i8tail = knob != 0; ix.xt_state = kTailCopy[st];
        const Words key = {d, mode, cus, wg, knob, st};
        // spelled out: the default knobs (each grid's first entry) at the widths of kFullD
        const bool spelled = std::count(kFullD.begin(), kFullD.end(), d) && mode == kModes[0] && cus == kCus[0] &&
                             wg == kWgpcu[0] && knob == kKnob[0] && st == kState[0];
        uint64_t h = 14695981039346656037ull;
        for (int nt : kNtotal) for (int nq : kNq) for (int k : kK) {
            ix.ntotal = nt;
            const RoutePlan r = choose_route(ix, nq, k);
            const Plan& p = r.plan;
            const int32_t v[kValues] = {(int)r.route, r.tail_ok ? 1 : 0, r.i8_inst, p.wr, p.wq, p.km, p.bm, p.bq, p.nqb,
                                        p.nq_pad, p.ntiles, p.nsplit, p.ncand, p.wgs, p.big ? 1 : 0, p.ib};
            for (int x : v) h = fnv(h, x);
            if (!spelled) continue;
            const int32_t* t = &w[row0 + kValues * nrows++];
            if (!std::equal(v, v + kValues, t))
                expect("row (d mode cus wgpcu knob state ntotal nq k) " + text(key) + " " + text({nt, nq, k}),
                       text(Words(v, v + kValues)), text(Words(t, t + kValues)));
        }
        char hex[2][17];
        const uint32_t* t = reinterpret_cast<const uint32_t*>(&w[slice0 + 2 * nslices++]);
        std::snprintf(hex[0], 17, "%016llx", (unsigned long long)h);
        std::snprintf(hex[1], 17, "%016llx", (unsigned long long)(t[0] | (uint64_t)t[1] << 32));
        expect("slice (d mode cus wgpcu knob state) " + text(key), hex[0], hex[1]);
    }
    if (bad) { std::fprintf(stderr, "route_check: %d differences\n", bad); return 1; }
    std::printf("route_check: ok (%zu slices, %zu rows)\n", nslices, nrows);
    return 0;
}
