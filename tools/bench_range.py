"""Range-search cost on the bench corpus (1M x 1968, generated on device), beside the exact top-10
search of the same batches in the same process.  Measurement tool (not bench.py); prints one JSON
line per (batch, radius) case.

Cases: batches of 1,024 queries and of 1 query; one radius that gives about 10 hits per query and
one that gives about 1,000 (the medians of the 10th / 1,000th exact neighbour distance over 64
queries).  Per case: end-to-end ms of range_search_device (queries on the device, result complete
on the device) and of the host form (numpy in, numpy out), the tile kernel's own time (HIP events,
knn_set_timing), hits per query, and the search_mode="exact" k = 10 search_device of the same
batch, timed alternately with the range search so both see the same clock.

ROWS=<n> shrinks the corpus (rehearsal), REPS=<n> sets the timed repeats per case, BATCHES=a,b
the batch sizes (default 1024,1).
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from image_recommender_amd import _lib  # noqa: E402
from image_recommender_amd import faiss_compat as faiss  # noqa: E402


def kernel_ms(idx):
    t, n = C.c_double(), C.c_int()
    _lib.check(_lib.load().knn_kernel_time(idx.handle, C.byref(t), C.byref(n)), "knn_kernel_time")
    return t.value / max(n.value, 1), n.value


def main():
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[3])
    rows = int(os.environ.get("ROWS", cfg["rows"]))
    reps = int(os.environ.get("REPS", 10))
    cent = bench.make_centres(torch, cfg, dev, 3)
    idx = faiss.IndexFlatL2(1968, device=0)
    idx.reserve(rows)
    st = torch.cuda.current_stream().cuda_stream
    for blk in bench.gen_rows(torch, cfg, cent, 0, rows, dev, 3):
        idx.add_device(blk.data_ptr(), blk.shape[0], st)
    torch.cuda.synchronize()
    qd = bench.gen_queries(torch, cfg, cent, 1024, dev, 3)
    qh = qd.cpu().numpy()
    idx.search_mode = "exact"
    lib = _lib.load()

    # radii: medians of the 10th and 1,000th exact neighbour distance
    kk = min(1000, rows)
    Dk, _ = idx.search(qh[:64], kk)
    radii = {"~10": float(np.median(Dk[:, min(10, kk) - 1])), "~1000": float(np.median(Dk[:, kk - 1]))}

    for nq in [int(v) for v in os.environ.get("BATCHES", "1024,1").split(",")]:
        qq = qd[:nq].contiguous()
        x = np.ascontiguousarray(qh[:nq])
        Dd = torch.empty((nq, 10), dtype=torch.float32, device=dev)
        Id = torch.empty((nq, 10), dtype=torch.int64, device=dev)

        def run_search():
            idx.search_device(qq.data_ptr(), nq, 10, Dd.data_ptr(), Id.data_ptr(), st)
            torch.cuda.synchronize()

        for tag, radius in radii.items():
            def run_range():
                res = idx.range_search_device(qq.data_ptr(), nq, radius, st)
                res.device_ptrs()                      # waits for the last kernel
                return res

            for _ in range(3):                         # warm-up: code objects, workspace growth
                run_range()
                run_search()
                idx.range_search(x, radius)
            size = run_range().size
            t_range, t_search, t_host = [], [], []
            for _ in range(reps):                      # alternating: the same clock for both
                t0 = time.perf_counter()
                run_range()
                t1 = time.perf_counter()
                run_search()
                t2 = time.perf_counter()
                idx.range_search(x, radius)
                t3 = time.perf_counter()
                t_range.append(t1 - t0)
                t_search.append(t2 - t1)
                t_host.append(t3 - t2)
            _lib.check(lib.knn_set_timing(idx.handle, 1), "knn_set_timing")
            for _ in range(reps):
                run_range()
            k_range, launches = kernel_ms(idx)
            for _ in range(reps):
                run_search()
            k_search, _ = kernel_ms(idx)
            _lib.check(lib.knn_set_timing(idx.handle, 0), "knn_set_timing")
            med = lambda v: float(np.median(v)) * 1e3  # noqa: E731
            print(json.dumps({
                "rows": rows, "nq": nq, "hits": tag, "radius": radius, "hits_per_query": size / nq,
                "range_device_ms": med(t_range), "range_device_ms_min": min(t_range) * 1e3,
                "range_host_ms": med(t_host),
                "range_tile_kernel_ms": k_range, "tile_launches_per_call": launches / reps,
                "exact_top10_device_ms": med(t_search), "exact_top10_device_ms_min": min(t_search) * 1e3,
                "exact_top10_kernel_ms": k_search,
                "range_over_exact": med(t_range) / med(t_search), "reps": reps}), flush=True)


if __name__ == "__main__":
    main()
