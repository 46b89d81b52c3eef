"""Hashes of search results on a seeded bench corpus, for A/B bit-identity of library variants (run
once per IMGREC_LIB_NAME; equal hashes = identical results).  One line per route:

    auto      the AUTO search, k = 10 (with its certificate statistics)
    exact10   search_mode="exact", k = 10          exact32   the same, k = 32
    range     range_search at the median 100th exact neighbour distance (~100 hits per query)
    filter10  a random 10 % IDSelectorBitmap, k = 10 (register-list route)
    filter100 the same mask, k = 100 (store-everything + segmented-sort route)

Usage: IMGREC_LIB_NAME=libimgrec_x.so python tools/ab_result_hash.py [config] [nq[,nq..]] [rows]"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    import numpy as np
    import torch
    import bench
    from image_recommender_amd import faiss_compat as faiss
    cid = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    nqs = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1024]
    cfg = dict(bench.CONFIGS[cid])
    rows = int(sys.argv[3]) if len(sys.argv) > 3 else cfg["rows"]
    dev = torch.device("cuda", 0)
    cen = bench.make_centres(torch, cfg, dev, cid)
    d = sum(cfg["parts"])
    idx = faiss.IndexFlatL2(d)
    idx.reserve(rows)
    st = torch.cuda.current_stream().cuda_stream
    for blk in bench.gen_rows(torch, cfg, cen, 0, rows, dev, cid):
        idx.add_device(blk.data_ptr(), blk.shape[0], st)
    mask = np.random.default_rng(cid).random(rows) < 0.1
    params = faiss.SearchParameters(sel=faiss.IDSelectorBitmap(np.packbits(mask, bitorder="little")))
    lib = os.environ.get("IMGREC_LIB_NAME", "libimgrec.so")
    for nq in nqs:
        q = bench.gen_queries(torch, cfg, cen, nq, dev, cid)
        x = np.ascontiguousarray(q.cpu().numpy())
        tag = f"{lib} cfg{cid} rows={rows} nq={nq}"
        idx.search_mode = "auto"
        D = torch.empty((nq, 10), dtype=torch.float32, device=dev)
        I = torch.empty((nq, 10), dtype=torch.int64, device=dev)
        idx.search_device(q.data_ptr(), nq, 10, D.data_ptr(), I.data_ptr(), st)
        torch.cuda.synchronize()
        print(f"{tag} auto {digest(D.cpu().numpy(), I.cpu().numpy())} stats={idx.certificate_stats()}")
        idx.search_mode = "exact"
        print(f"{tag} exact10 {digest(*idx.search(x, 10))}")
        print(f"{tag} exact32 {digest(*idx.search(x, 32))}")
        radius = float(np.median(idx.search(x, min(100, rows))[0][:, -1]))
        lims, Dr, Ir = idx.range_search(x, radius)
        print(f"{tag} range {digest(lims, Dr, Ir)} hits/query={lims[-1] / nq:.1f}")
        print(f"{tag} filter10 {digest(*idx.search(x, 10, params=params))}")
        print(f"{tag} filter100 {digest(*idx.search(x, 100, params=params))}", flush=True)


if __name__ == "__main__":
    main()
