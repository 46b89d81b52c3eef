"""Filtered-search cost on the bench corpora (1M x 1968 and 1M x 768, generated on device), beside
the exact top-10 search of the same batches in the same process.  Measurement tool (not bench.py);
prints one JSON line per (corpus, batch, mask) case.

Cases: batches of 1 and 1,024 queries, k = 10; masks selecting 100 %, 10 % and 1 % of the rows at
random and one contiguous 1 % range; a mask selecting nothing (the compaction, an idle tile launch
and the merge: an upper bound of the fixed cost); and k = 100 at the random 1 % mask (the sort
route).  Per case: HIP-event ms of search_filtered_device (queries, bitmap and outputs on the
device) — median, minimum and maximum over the repeats — the gathered tile kernel's own time
(knn_set_timing), and the search_mode="exact" k = 10 search_device of the same batch, timed
alternately with the filtered search so both see the same clock; its max - min is the comparator's
run-to-run spread of this session.

CONFIGS=3,2 picks the corpora (bench.py's configs: 3 = 1M x 1968, 2 = 1M x 768), ROWS=<n> shrinks
them (rehearsal), REPS=<n> sets the timed repeats per case, BATCHES=a,b the batch sizes,
MASKS=<tags> keeps only the named masks.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from image_recommender_amd import _lib  # noqa: E402
from image_recommender_amd import faiss_compat as faiss  # noqa: E402


def kernel_ms(idx):
    t, n = C.c_double(), C.c_int()
    _lib.check(_lib.load().knn_kernel_time(idx.handle, C.byref(t), C.byref(n)), "knn_kernel_time")
    return t.value / max(n.value, 1)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def run_config(c, dev):
    cfg = dict(bench.CONFIGS[c])
    rows = int(os.environ.get("ROWS", cfg["rows"]))
    reps = int(os.environ.get("REPS", 10))
    d = sum(cfg["parts"])
    cent = bench.make_centres(torch, cfg, dev, 3)
    idx = faiss.IndexFlatL2(d, device=0)
    idx.reserve(rows)
    st = torch.cuda.current_stream().cuda_stream
    for blk in bench.gen_rows(torch, cfg, cent, 0, rows, dev, 3):
        idx.add_device(blk.data_ptr(), blk.shape[0], st)
    torch.cuda.synchronize()
    qd = bench.gen_queries(torch, cfg, cent, 1024, dev, 3)
    idx.search_mode = "exact"
    lib = _lib.load()

    rng = np.random.default_rng(11)
    u = rng.random(rows)
    lo = rows // 3
    contiguous = np.zeros(rows, dtype=bool)
    contiguous[lo:lo + rows // 100] = True
    masks = [("100%", np.ones(rows, dtype=bool), 10), ("10% random", u < 0.10, 10),
             ("1% random", u < 0.01, 10), ("1% contiguous", contiguous, 10),
             ("none", np.zeros(rows, dtype=bool), 10), ("1% random", u < 0.01, 100)]
    if os.environ.get("MASKS"):
        masks = [m for m in masks if m[0] in os.environ["MASKS"].split(",")]

    for nq in [int(v) for v in os.environ.get("BATCHES", "1,1024").split(",")]:
        qq = qd[:nq].contiguous()
        D10 = torch.empty((nq, 10), dtype=torch.float32, device=dev)
        I10 = torch.empty((nq, 10), dtype=torch.int64, device=dev)

        def run_search():
            idx.search_device(qq.data_ptr(), nq, 10, D10.data_ptr(), I10.data_ptr(), st)

        for tag, mask, k in masks:
            bm = torch.from_numpy(np.packbits(mask, bitorder="little")).to(dev)
            Dk = torch.empty((nq, k), dtype=torch.float32, device=dev)
            Ik = torch.empty((nq, k), dtype=torch.int64, device=dev)

            def run_filtered():
                idx.search_filtered_device(qq.data_ptr(), nq, k, bm.data_ptr(), rows, Dk.data_ptr(),
                                           Ik.data_ptr(), st)

            for _ in range(3):                         # warm-up: code objects, workspace growth
                run_filtered()
                run_search()
            torch.cuda.synchronize()
            t_f, t_s = [], []
            for _ in range(reps):                      # alternating: the same clock for both
                t_f.append(event_ms(run_filtered))
                t_s.append(event_ms(run_search))
            _lib.check(lib.knn_set_timing(idx.handle, 1), "knn_set_timing")
            for _ in range(reps):
                run_filtered()
            torch.cuda.synchronize()
            k_f = kernel_ms(idx)
            for _ in range(reps):
                run_search()
            torch.cuda.synchronize()
            k_s = kernel_ms(idx)
            _lib.check(lib.knn_set_timing(idx.handle, 0), "knn_set_timing")
            if k == 10 and mask.all():                 # the same rows: the same neighbours
                same = bool((Ik == I10).all().item())
            else:
                same = None
            f, s = stats(t_f), stats(t_s)
            print(json.dumps({
                "rows": rows, "d": d, "nq": nq, "k": k, "mask": tag, "selected": int(mask.sum()),
                "filtered_ms": f, "filtered_tile_kernel_ms": k_f,
                "exact_top10_ms": s, "exact_top10_spread_ms": s["max"] - s["min"],
                "exact_top10_kernel_ms": k_s, "filtered_over_exact": f["median"] / s["median"],
                "labels_equal_exact_top10": same, "reps": reps}), flush=True)
    del idx
    torch.cuda.empty_cache()


def main():
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    for c in [int(v) for v in os.environ.get("CONFIGS", "3,2").split(",")]:
        run_config(c, dev)


if __name__ == "__main__":
    main()
