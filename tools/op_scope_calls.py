"""A fixed sequence of index operations for counting HIP API calls per library build.

200 one-query search_device calls on one stream with the eager fence, 200 with the lazy fence, 50
host searches and 20 searches that alternate between two streams.  Run it under
``rocprofv3 --hip-trace --stats`` (no counters), one fresh process per library
(``IMGREC_LIB_NAME``): the per-API call counts of two builds that do the same work are equal
(tools/ab_op_scope.sh, profiles/op_scope/README.md).
"""
import numpy as np
import torch

from image_recommender_amd import faiss_compat as faiss

D, N, K = 128, 20000, 10


def main():
    rng = np.random.default_rng(0)
    xb = rng.standard_normal((N, D)).astype(np.float32)
    xq = rng.standard_normal((1, D)).astype(np.float32)
    q = torch.from_numpy(xq).cuda()
    Dd = torch.empty((1, K), dtype=torch.float32, device="cuda")
    Id = torch.empty((1, K), dtype=torch.int64, device="cuda")
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for lazy in (False, True):
        idx = faiss.IndexFlatL2(D)
        idx.set_fence_mode(lazy)
        idx.add(xb)
        for _ in range(200):
            idx.search_device(q.data_ptr(), 1, K, Dd.data_ptr(), Id.data_ptr(), a.cuda_stream)
        for _ in range(50):
            idx.search(xq, K)
        for i in range(20):
            idx.search_device(q.data_ptr(), 1, K, Dd.data_ptr(), Id.data_ptr(), (b if i % 2 == 0 else a).cuda_stream)
        torch.cuda.synchronize()
        print("lazy" if lazy else "eager", Id.cpu().numpy().ravel().tolist())
        del idx


if __name__ == "__main__":
    main()
