#!/usr/bin/env python
"""Time faiss_compat.Kmeans against the torch k-means of ivfpq.IndexIVFPQ on the same device tensor.

For each shape (default: n = 1 M, d = 128, k = 256 and n = 1 M, d = 768, k = 1024) a fresh child
process, under its own time limit, generates a seeded mixture on the GPU, warms both paths up, and
times `--iters` Lloyd iterations of each `--repeats` times, alternating the two, with device events:

* new: ``Kmeans.train_device`` (csrc/knn_kmeans.hip), with the per-iteration GPU milliseconds of the
  assignment, the sort and the segmented sums (``iteration_stats``);
* old: ``ivfpq.IndexIVFPQ._kmeans`` (k = 1 exact search + ``index_add_``), same tensor, k and niter.

The step's floor is 2 n k d FLOP at the fp32-MFMA rate (155 TF measured) plus two reads of x at
the HBM rate (6.29 TB/s measured), the figures of the chip's microarchitecture notes.  The parent
stops at the first child that fails or runs out of time.  One JSON document goes to --out.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MFMA_F32_FLOPS = 155e12
HBM_BYTES_PER_S = 6.29e12
SHAPES = [(1_000_000, 128, 256), (1_000_000, 768, 1024)]


def worker(n: int, d: int, k: int, iters: int, repeats: int) -> dict:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from image_recommender_amd import faiss_compat as faiss
    from image_recommender_amd.ivfpq import IndexIVFPQ

    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(7)
    centres = torch.randn((64, d), generator=g, device=dev)
    x = centres[torch.randint(0, 64, (n,), generator=g, device=dev)]
    x = (x + 0.5 * torch.randn((n, d), generator=g, device=dev)).contiguous()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream

    m = next(m for m in (8, 4, 2, 1) if d % m == 0 and d // m <= 256)
    old = IndexIVFPQ(d, k, m, device=torch.cuda.current_device())

    def run_new():
        km = faiss.Kmeans(d, k, niter=iters, seed=1234)
        km.train_device(x.data_ptr(), n, st)
        return km

    def run_old():
        return old._kmeans(x, k, iters, 1234)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    faiss.Kmeans(d, k, niter=2).train_device(x.data_ptr(), n, st)      # warm-up of both paths
    old._kmeans(x, k, 2, 1234)
    torch.cuda.synchronize()
    new_ms, old_ms, split = [], [], []
    for _ in range(repeats):
        t, km = timed(run_new)
        new_ms.append(t)
        split.append({key: float(np.mean([s[key] for s in km.iteration_stats]))
                      for key in ("ms_assign", "ms_sort", "ms_update")})
        t, _ = timed(run_old)
        old_ms.append(t)
    flop = 2.0 * n * k * d
    floor_ms = 1e3 * (flop / MFMA_F32_FLOPS + 2.0 * n * d * 4 / HBM_BYTES_PER_S)
    per_iter = {key: float(np.median([s[key] for s in split])) for key in split[0]}
    step_ms = sum(per_iter.values())
    return {
        "n": n, "d": d, "k": k, "iters": iters, "repeats": repeats,
        "new_train_ms": new_ms, "old_kmeans_ms": old_ms,
        "new_train_ms_median": float(np.median(new_ms)), "old_kmeans_ms_median": float(np.median(old_ms)),
        "speedup_old_over_new": float(np.median(old_ms) / np.median(new_ms)),
        "per_iteration_ms": per_iter, "step_ms": step_ms,
        "assign_tflops": flop / (per_iter["ms_assign"] * 1e-3) / 1e12,
        "floor_ms": floor_ms, "step_over_floor": step_ms / floor_ms,
        "final_objective": float(km.obj[-1]), "nsplit_total": int(sum(s["nsplit"] for s in km.iteration_stats)),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="kmeans_bench.json")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("N", "D", "K"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    shapes = [tuple(s) for s in a.shape] if a.shape else SHAPES
    if a.worker:
        print("RESULT " + json.dumps(worker(*shapes[0], a.iters, a.repeats)))
        return 0
    results = []
    rc = 0
    for n, d, k in shapes:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--shape", str(n), str(d), str(k),
               "--iters", str(a.iters), "--repeats", str(a.repeats)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"n={n} d={d} k={k}: no result within {a.timeout} s; stopping", file=sys.stderr)
            rc = 124
            break
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(f"n={n} d={d} k={k}: child exited {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            rc = p.returncode or 1
            break
        r = json.loads(line[len("RESULT "):])
        results.append(r)
        print(f"n={n} d={d} k={k}: new {r['new_train_ms_median']:.1f} ms, old {r['old_kmeans_ms_median']:.1f} ms "
              f"({r['speedup_old_over_new']:.2f}x), step {r['step_ms']:.2f} ms = {r['step_over_floor']:.1f}x its "
              f"floor, assign {r['assign_tflops']:.1f} TF")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({"shapes": results}, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
