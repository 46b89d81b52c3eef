#!/usr/bin/env python3
"""In-process A/B of the 256 x 256 candidate pass: one index of bench.py's workload, searches
alternating between search_mode = "bf16" (the pure bf16 kernel) and "auto" (the int8-tail sibling
where the index takes it) in rounds.  Reports, per mode, the median and the minimum over the rounds
of the step (wall time of `steps` searches between synchronisations) and of the candidate kernel
(the library's own event pair around its launch, knn_set_timing / knn_kernel_time), and AUTO's
certificate counts: queries that took the second chance, queries re-run exactly.

Usage: python tools/i8tail_ab.py [--config 3] [--rows N] [--nq 1024] [--k 10] [--rounds 7] [--steps 10]
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    import torch
    from image_recommender_amd import _lib
    from image_recommender_amd.faiss_compat import METRIC_L2
    from image_recommender_amd.sharded import ShardedIndex

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    cfg = dict(bench.CONFIGS[a.config])
    if a.rows:
        cfg["rows"] = a.rows
    seed = a.config
    centres = bench.make_centres(torch, cfg, device, seed)
    q = bench.gen_queries(torch, cfg, centres, a.nq, device, seed)
    shard = ShardedIndex(int(sum(cfg["parts"])), cfg["rows"], METRIC_L2, device=0)
    for blk in bench.gen_rows(torch, cfg, centres, shard.row0, shard.row1, device, seed):
        shard.add_local(blk)
    torch.cuda.synchronize()
    lib, h = _lib.load(), shard.index.handle

    def kernel_name():
        name = C.create_string_buffer(128)
        _lib.check(lib.knn_plan_kernel(h, a.nq, a.k, name, 128), "knn_plan_kernel")
        return name.value.decode()

    def region(events):
        if events:
            lib.knn_set_timing(h, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            shard.search(q, a.k)
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) * 1e3 / a.steps
        if not events:
            return el
        tot, n = C.c_double(), C.c_int()
        _lib.check(lib.knn_kernel_time(h, C.byref(tot), C.byref(n)), "knn_kernel_time")
        lib.knn_set_timing(h, 0)
        return tot.value / max(n.value, 1)

    out = {"config": a.config, "rows": cfg["rows"], "nq": a.nq, "k": a.k, "rounds": a.rounds, "steps": a.steps}
    res = {m: {"step_ms": [], "kernel_ms": []} for m in ("bf16", "auto")}
    for m in ("auto", "bf16"):                         # warm-up; AUTO's first search builds and judges the copy
        shard.index.search_mode = m
        for _ in range(3):
            shard.search(q, a.k)
        out[m + "_kernel"] = kernel_name()
    for _ in range(a.rounds):
        for m in ("bf16", "auto"):
            shard.index.search_mode = m
            res[m]["step_ms"].append(region(False))
            res[m]["kernel_ms"].append(region(True))
    shard.index.search_mode = "auto"
    shard.search(q, a.k)
    out["auto_certificate"] = shard.index.certificate_stats()
    for m, r in res.items():
        out[m] = {k_: {"median": round(statistics.median(v), 4), "min": round(min(v), 4)} for k_, v in r.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
