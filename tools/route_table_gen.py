#!/usr/bin/env python3
"""Record the route table that tests/fuzz/route_check.cpp holds choose_route to.

The table is taken from a revision that still chose routes the old way — the ladder use_i8 ->
use_b16 -> use_split of search_locked, with use_i8tail beside it — and NOT from choose_route:

* ``git show REV:...`` extracts knn_plan.cpp (whole), the use_* / i8_wins_8q block of
  knn_search.cpp, the Plan block of knn_index.h, the tile constants of knn_kernels.h and
  include/imgrec_knn.h;
* they are compiled unchanged, with g++, against a stub ``knn_index`` that has the fields they read,
  filled from d the way create_single fills them;
* a small driver walks the grid below, applies the ladder as search_locked did, and prints the table.

It only has to work for the revision the table was recorded from (the parent of the change that
introduced choose_route): later revisions have no use_* functions to extract.

Table format (tests/golden/route_table.bin, little-endian int32 words; ``--text`` prints the same
content as lines).  A slice is one (d, mode, cus, wgpcu, knob, state); its rows run over ntotal, then
nq, then k, in the order of the grids, and a row is the 16 values

    route tail_ok i8_inst wr wq km bm bq nqb nq_pad ntiles nsplit ncand wgs big ib

Words: the magic "RTB1"; the revision's first 12 characters; the lengths of the ten grids (d, mode,
cus, wgpcu, knob, state, ntotal, nq, k, spelled-out d), then the grids themselves; per slice, in
that nesting order, the low and high word of the FNV-1a 64 digest of its rows (each value as 4
little-endian bytes); then the 16 values of every spelled-out row, in the same order.  Rows are
spelled out for the default knobs (the first mode, cus, wgpcu, knob and state of the grids: AUTO,
all CUs, 0, on, copy undecided) at d = 768 and d = 1968.  state: 0 undecided, 1 built, 2 ineligible.

Usage: python tools/route_table_gen.py REV [-o tests/golden/route_table.bin] [--text]
"""
from __future__ import annotations

import argparse
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = "image_recommender_amd/csrc/"

# (448 / 512 and 1088 / 1408: 7 / 8 and 17 / 22 blocks of 64, next to kI8MinBlocks and i8_wins_8q's ends)
D = [48, 63, 64, 128, 255, 256, 448, 512, 768, 832, 896, 1024, 1088, 1280, 1408, 1472, 1536, 1968, 4096,
     4160, 16448]
NTOTAL = [0, 1, 255, 1000, 16383, 16384, 131072, 1000000, 10000000]
NQ = "1, 2, 3, 4, 5, 8, 9, 32, 33, 128, 129, kB16BigMinQ - 1, kB16BigMinQ, 1024, 8192"
K = [1, 8, 9, 10, 11, 16, 17, 32]
MODES = [0, 1, 2, 3, 4]
CUS = [256, 32, 8]
WGPCU = [0, 1]
KNOB = [1, 0]
STATE = [0, 1, 2]
FULL_D = [768, 1968]


def show(rev: str, path: str) -> str:
    return subprocess.run(["git", "show", f"{rev}:{path}"], cwd=ROOT, check=True, capture_output=True,
                          text=True).stdout


def between(text: str, first: str, last: str, inclusive: bool) -> str:
    a = text.index(first)
    b = text.index(last, a)
    return text[a:b + len(last) if inclusive else b]


def line_with(text: str, needle: str) -> str:
    return next(ln for ln in text.splitlines() if needle in ln)


DRIVER = r"""
#include <cstdio>
#include "knn_index.h"
namespace imgrec {
%(use_block)s
}
using namespace imgrec;
static uint64_t fnv(uint64_t h, int v) {
    for (int i = 0; i < 4; ++i) { h ^= (uint32_t(v) >> (8 * i)) & 0xff; h *= 1099511628211ull; }
    return h;
}
int main() {
    const int Ds[] = {%(d)s}, Ks[] = {%(k)s}, Modes[] = {%(modes)s}, Cus[] = {%(cus)s};
    const int Wg[] = {%(wgpcu)s}, Knob[] = {%(knob)s}, State[] = {%(state)s}, FullD[] = {%(full_d)s};
    const long long Nt[] = {%(ntotal)s}, Nq[] = {%(nq)s};
    std::printf("grid ntotal"); for (long long v : Nt) std::printf(" %%lld", v);
    std::printf("\ngrid nq"); for (long long v : Nq) std::printf(" %%lld", v);
    std::printf("\ngrid k"); for (int v : Ks) std::printf(" %%d", v);
    std::printf("\n");
    for (int d : Ds) for (int mode : Modes) for (int cus : Cus) for (int wg : Wg) for (int knob : Knob)
    for (int state : State) {
        knn_index ix;
        // create_single's shape of a d-column index
        ix.d = d;
        ix.dp = (d + (d >= 256 ? 31 : 15)) / (d >= 256 ? 32 : 16) * (d >= 256 ? 32 : 16);
        ix.split_ok = ix.dp %% 32 == 0 && d >= 256;
        ix.b16_ok = d >= 64;
        ix.dpb = (d + 63) / 64 * 64;
        ix.nblk8 = d >= 64 && d <= 4096 ? (d + 63) / 64 : 0;
        ix.metric = KNN_METRIC_L2; ix.mode = mode; ix.cus = cus; ix.i8_wgpcu = wg; ix.i8tail = knob != 0;
        ix.xt_state = state == 0 ? 0 : state == 1 ? 1 : -1;
        bool full = false;
        for (int fd : FullD) full = full || fd == d;
        full = full && mode == 0 && cus == Cus[0] && wg == 0 && knob == 1 && state == 0;
        uint64_t h = 14695981039346656037ull;
        for (long long nt : Nt) for (long long nq : Nq) for (int k : Ks) {
            ix.ntotal = nt;
            // search_locked's ladder
            const bool i8 = use_i8(&ix, nq, k);
            const bool b16 = !i8 && use_b16(&ix, nq, k);
            const bool split = !i8 && !b16 && use_split(&ix, nq, k);
            const Plan p = i8 ? make_i8_plan(ix.ntotal, nq, k, ix.cus, ix.i8_wgpcu, ix.nblk8)
                         : b16 ? make_b16_plan(ix.ntotal, nq, k, ix.cus, ix.dpb)
                         : split ? make_split_plan(ix.ntotal, nq, split_kc(k), ix.cus)
                                 : make_plan(ix.ntotal, nq, k, ix.cus);
            const int v[16] = {i8 ? 3 : (b16 ? 2 : (split ? 1 : 0)), use_i8tail(&ix, nq, k) ? 1 : 0,
                               i8 ? (nq <= 2 ? (int)nq : (nq <= 4 ? 4 : 8)) : 0,      // knn_plan_kernel
                               p.wr, p.wq, p.km, p.bm, p.bq, p.nqb, p.nq_pad, p.ntiles, p.nsplit, p.ncand,
                               p.wgs, p.big ? 1 : 0, p.ib};
            for (int x : v) h = fnv(h, x);
            if (full) {
                std::printf("row %%d %%d %%d %%d %%d %%d %%lld %%lld %%d", d, mode, cus, wg, knob, state, nt, nq, k);
                for (int x : v) std::printf(" %%d", x);
                std::printf("\n");
            }
        }
        std::printf("slice %%d %%d %%d %%d %%d %%d %%016llx\n", d, mode, cus, wg, knob, state, (unsigned long long)h);
    }
    return 0;
}
"""

STUB = r"""
#pragma once
#include <algorithm>
#include <cstdint>
#include "imgrec_knn.h"
#define __host__
#define __device__
namespace imgrec {
%(consts)s
%(i8_row_bytes)s
%(plan_block)s
}
struct knn_index {
    int d = 0, dp = 0, dpb = 0, nblk8 = 0, cus = 256, i8_wgpcu = 0, metric = 0, mode = 0, xt_state = 0;
    bool split_ok = false, b16_ok = false, i8tail = true;
    int64_t ntotal = 0;
};
"""


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev")
    ap.add_argument("-o", "--out", default=str(ROOT / "tests" / "golden" / "route_table.bin"))
    ap.add_argument("--text", action="store_true", help="print the table as text lines instead")
    a = ap.parse_args()
    sha = subprocess.run(["git", "rev-parse", "--short=12", a.rev], cwd=ROOT, check=True, capture_output=True,
                         text=True).stdout.strip()
    kernels_h = show(a.rev, CSRC + "knn_kernels.h")
    stub = STUB % {
        "consts": between(kernels_h, "constexpr int kTileRowsMax", "// Small-batch candidate pass", False),
        "i8_row_bytes": line_with(kernels_h, "inline int64_t i8_row_bytes("),
        "plan_block": between(show(a.rev, CSRC + "knn_index.h"), "struct Plan {", "int b16_km(int k);", True),
    }
    join = lambda v: ", ".join(str(x) for x in v)
    driver = DRIVER % {
        "use_block": between(show(a.rev, CSRC + "knn_search.cpp"), "// AUTO: the bf16 path at every corpus size.",
                             "int search_locked(", False),
        "d": join(D), "k": join(K), "modes": join(MODES), "cus": join(CUS), "wgpcu": join(WGPCU),
        "knob": join(KNOB), "state": join(STATE), "full_d": join(FULL_D), "ntotal": join(NTOTAL), "nq": NQ,
    }
    with tempfile.TemporaryDirectory() as tmp:
        t = Path(tmp)
        (t / "knn_index.h").write_text(stub)
        (t / "imgrec_knn.h").write_text(show(a.rev, "include/imgrec_knn.h"))
        (t / "knn_plan.cpp").write_text(show(a.rev, CSRC + "knn_plan.cpp"))
        (t / "driver.cpp").write_text(driver)
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", tmp, str(t / "driver.cpp"), str(t / "knn_plan.cpp"),
                        "-o", str(t / "gen")], check=True)
        table = subprocess.run([str(t / "gen")], check=True, capture_output=True, text=True).stdout
    if a.text:
        print(table, end="")
        return
    lines = [ln.split() for ln in table.splitlines()]
    inner = {w[1]: [int(x) for x in w[2:]] for w in lines if w[0] == "grid"}
    grids = [D, MODES, CUS, WGPCU, KNOB, STATE, inner["ntotal"], inner["nq"], inner["k"], FULL_D]
    slices = [[int(w[7], 16) & 0xffffffff, int(w[7], 16) >> 32] for w in lines if w[0] == "slice"]
    rows = [[int(x) for x in w[10:]] for w in lines if w[0] == "row"]
    words = [len(g) for g in grids] + sum(grids, []) + sum(slices, []) + sum(rows, [])
    Path(a.out).write_bytes(b"RTB1" + sha.encode().ljust(12)[:12] + struct.pack(f"<{len(words)}I", *words))
    print(f"{a.out}: {len(slices)} slices, {len(rows)} rows from {sha}", file=sys.stderr)

if __name__ == "__main__":
    main()
