"""Diagnostic: cycles per stage and the in-kernel clock of the 256 x 256 candidate kernels' stage
loops on bench config 3, from a build with -DIMGREC_B16_STAMPS (lib/libimgrec_stamps.so: csrc/
knn_b16w.hip g_b16w_loop — wave 0 of every workgroup sums s_memtime and s_memrealtime around its
tiles' stage loops, the int8 tail stages and the bf16 stages apart).

Per route (AUTO = the int8-tail sibling, then "bf16"): at least SECONDS of back-to-back searches on
the real data, then the last launch's sums; printed per route: the median over workgroups of cycles
per tail stage, cycles per bf16 stage, and the clock each loop held (cycles / ticks x 100 MHz).
The stamped build's wall time means nothing (its stamps forbid overlaps); read its shares."""
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("IMGREC_LIB_NAME", "libimgrec_stamps.so")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from image_recommender_amd import _lib
from image_recommender_amd.faiss_compat import METRIC_L2
from image_recommender_amd.sharded import ShardedIndex

CFG = int(os.environ.get("IMGREC_STAMPS_CFG", "3"))
SECONDS = float(os.environ.get("IMGREC_STAMPS_SECONDS", "2.5"))
cfg = dict(bench.CONFIGS[CFG])
dev = torch.device("cuda", 0)
D = int(sum(cfg["parts"]))
centres = bench.make_centres(torch, cfg, dev, CFG)
q = bench.gen_queries(torch, cfg, centres, 1024, dev, CFG)
shard = ShardedIndex(D, cfg["rows"], METRIC_L2, device=0)
for blk in bench.gen_rows(torch, cfg, centres, shard.row0, shard.row1, dev, CFG):
    shard.add_local(blk)
lib = _lib.load()
out = {}
for mode in ("auto", "bf16"):
    shard.index.search_mode = mode
    for _ in range(4):                                   # (AUTO: the copy's build and its trial)
        shard.search(q, 10)
    torch.cuda.synchronize()
    name = C.create_string_buffer(128)
    lib.knn_plan_kernel(shard.index.handle, 1024, 10, name, 128)
    t0, n = time.time(), 0
    while time.time() - t0 < SECONDS:
        for _ in range(50):
            shard.search(q, 10)
        torch.cuda.synchronize()
        n += 50
    buf = (C.c_ulonglong * (6 * 1024))()
    assert lib.knn_b16w_loop_read(buf) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 2, 3).astype(np.float64)
    a = a[a[:, 1, 2] > 0]                                # workgroups that ran bf16 stages
    rec = {"kernel": name.value.decode(), "launches": n, "workgroups": int(a.shape[0])}
    for i, kind in enumerate(("tail", "bf16")):
        cyc, rt, ns = a[:, i, 0], a[:, i, 1], a[:, i, 2]
        if not (ns > 0).all():
            continue
        rec[kind] = {"stages_per_wg": float(np.median(ns)), "cycles_per_stage": float(np.median(cyc / ns)),
                     "ns_per_stage": float(np.median(rt / ns) * 10.0),
                     "clock_ghz": float(np.median(cyc / rt) * 0.1)}
    out[mode] = rec
    print(mode, json.dumps(rec), file=sys.stderr)
print(json.dumps(out))
