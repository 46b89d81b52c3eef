#!/usr/bin/env python
"""Time SoftVLAD.encode_device against what the same work takes without it: the 4-NN by
IndexFlatL2(codebook).search_device plus the aggregation and the three normalisations in PyTorch.

Shape (default: the reference's): nimg images x per descriptors of width d against a k-word
codebook, nn neighbours, everything device-resident.  Seeded RootSIFT-like descriptors (sparse
gamma prototypes, modulated, square-rooted and L2-normalised) are generated on the GPU and the
codebook is 5 Lloyd iterations of faiss_compat.Kmeans on them.  Both paths are warmed up, then timed
`--repeats` times with device events, alternating; medians are reported.

* new: ``SoftVLAD.encode_device`` (csrc/vlad.hip: norms, nn, aggregate, epilogue; the N x nn lists
  go to the library's workspace).
* old, part 1: ``IndexFlatL2.search_device`` of the N descriptors against the k codebook rows.
* old, part 2: PyTorch: w = exp(-D / 2 sigma^2); per slot an ``index_add_`` of w * x into an
  (nimg * k, d) accumulator and of w into (nimg * k); minus sum(w) * C; row norms, signed square
  root, global norm.  (The factored form: the residual form would also gather C[I], N x nn x d.)
  The descriptor-to-image map is built outside the timed window.

Floors: 2 N k d FLOP at the fp32-MFMA rate (155 TF measured) and one read of x plus one write of
the output at the HBM rate (6.29 TB/s measured), the figures tools/kmeans_bench.py uses.  The
whole call's time is held against them (a call's share, not a kernel's).  One JSON document goes
to --out.  A machine without a GPU fails.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MFMA_F32_FLOPS = 155e12
HBM_BYTES_PER_S = 6.29e12


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="vlad_bench.json")
    ap.add_argument("--nimg", type=int, default=512)
    ap.add_argument("--per", type=int, default=1000, help="descriptors per image")
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--nn", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=125.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--new-only", action="store_true", help="only the new path (for a kernel trace)")
    a = ap.parse_args()

    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from image_recommender_amd import faiss_compat as faiss
    from image_recommender_amd.vlad import SoftVLAD

    if not torch.cuda.is_available():
        print("no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda")
    nimg, per, d, k, nn = a.nimg, a.per, a.d, a.k, a.nn
    N = nimg * per
    g = torch.Generator(device=dev).manual_seed(7)

    def gamma(shape, conc, scale):
        return torch._standard_gamma(torch.full(shape, conc, device=dev), generator=g) * scale

    proto = gamma((40, d), 0.6, 1.0) * (torch.rand((40, d), generator=g, device=dev) < 0.35)
    label = torch.randint(0, 40, (N,), generator=g, device=dev)
    x = proto[label] * gamma((N, d), 4.0, 0.25)
    x += 0.05 * gamma((N, d), 0.5, 1.0) * (torch.rand((N, d), generator=g, device=dev) < 0.2)
    x /= x.abs().sum(1, keepdim=True) + 1e-7
    x.sqrt_()
    x /= x.norm(dim=1, keepdim=True) + 1e-7
    x = x.contiguous()
    offsets = torch.arange(nimg + 1, device=dev, dtype=torch.int64) * per
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream

    km = faiss.Kmeans(d, k, niter=5, seed=1234)
    km.train_device(x.data_ptr(), min(N, 256 * k), st)
    enc = SoftVLAD.from_kmeans(km, nn=nn, sigma=a.sigma)
    cb = torch.from_numpy(km.centroids.copy()).to(dev)
    out_new = torch.empty((nimg, k * d), dtype=torch.float32, device=dev)

    def run_new():
        enc.encode_device(x.data_ptr(), offsets.data_ptr(), nimg, N, out_new.data_ptr(), stream=st,
                          codebook_ptr=cb.data_ptr())

    index = faiss.IndexFlatL2(d)
    index.add_device(cb.data_ptr(), k, st)
    D = torch.empty((N, nn), dtype=torch.float32, device=dev)
    I = torch.empty((N, nn), dtype=torch.int64, device=dev)
    img = torch.arange(nimg, device=dev).repeat_interleave(per)
    two_s2 = 2.0 * a.sigma * a.sigma

    def run_search():
        index.search_device(x.data_ptr(), N, nn, D.data_ptr(), I.data_ptr(), st)

    def run_torch(D=D, I=I):
        w = torch.exp(D / -two_s2)
        key = img[:, None] * k + I
        acc = torch.zeros((nimg * k, d), dtype=torch.float32, device=dev)
        sw = torch.zeros((nimg * k,), dtype=torch.float32, device=dev)
        for s in range(nn):
            acc.index_add_(0, key[:, s], x * w[:, s:s + 1])
            sw.index_add_(0, key[:, s], w[:, s])
        v = acc.view(nimg, k, d) - sw.view(nimg, k, 1) * cb[None]
        r = v.norm(dim=2, keepdim=True)
        v = v / torch.where(r == 0, torch.ones_like(r), r)
        v = torch.sign(v) * torch.sqrt(torch.abs(v))
        v = v.reshape(nimg, k * d)
        gn = v.norm(dim=1, keepdim=True)
        return v / torch.where(gn == 0, torch.ones_like(gn), gn)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    for _ in range(3):
        run_new()
        if not a.new_only:
            run_search()
            run_torch()
    torch.cuda.synchronize()
    new_ms, search_ms, torch_ms = [], [], []
    out_old = None
    for _ in range(a.repeats):
        new_ms.append(timed(run_new)[0])
        if not a.new_only:
            search_ms.append(timed(run_search)[0])
            t, out_old = timed(run_torch)
            torch_ms.append(t)
    flop = 2.0 * N * k * d
    nbytes = 4.0 * (N * d + nimg * k * d)
    new = float(np.median(new_ms))
    res = {
        "nimg": nimg, "per_image": per, "N": N, "d": d, "k": k, "nn": nn, "sigma": a.sigma, "repeats": a.repeats,
        "new_ms": new_ms, "new_ms_median": new, "new_ms_min": float(min(new_ms)), "new_ms_max": float(max(new_ms)),
        "descriptors_per_s": N / (new * 1e-3),
        "mfma_floor_ms": 1e3 * flop / MFMA_F32_FLOPS, "hbm_floor_ms": 1e3 * nbytes / HBM_BYTES_PER_S,
        "call_share_of_mfma_limit": (1e3 * flop / MFMA_F32_FLOPS) / new,
        "call_share_of_hbm_limit": (1e3 * nbytes / HBM_BYTES_PER_S) / new,
        "call_tflops": flop / (new * 1e-3) / 1e12,
    }
    if not a.new_only:
        sm, tm = float(np.median(search_ms)), float(np.median(torch_ms))
        diff = (out_new - out_old).abs().max().item()
        # the same aggregation over the new path's own lists: what is left is summation order
        idx_new = torch.empty((N, nn), dtype=torch.int32, device=dev)
        dist_new = torch.empty((N, nn), dtype=torch.float32, device=dev)
        enc.encode_device(x.data_ptr(), offsets.data_ptr(), nimg, N, out_new.data_ptr(), stream=st,
                          codebook_ptr=cb.data_ptr(), nn_idx_ptr=idx_new.data_ptr(), nn_dist_ptr=dist_new.data_ptr())
        torch.cuda.synchronize()
        sets_differ = int((idx_new.long().sort(1).values != I.sort(1).values).any(1).sum().item())
        diff_same_lists = (out_new - run_torch(dist_new, idx_new.long())).abs().max().item()
        res.update({
            "old_search_ms": search_ms, "old_torch_ms": torch_ms, "old_search_ms_median": sm,
            "old_torch_ms_median": tm, "old_total_ms_median": sm + tm, "speedup_old_over_new": (sm + tm) / new,
            "max_abs_difference_new_vs_old": diff, "largest_output_element": out_new.abs().max().item(),
            "descriptors_whose_neighbour_sets_differ": sets_differ,
            "max_abs_difference_new_vs_torch_over_the_new_lists": diff_same_lists,
        })
        print(f"N={N} d={d} k={k} nn={nn}: new {new:.3f} ms ({res['descriptors_per_s'] / 1e6:.1f} M descriptors/s, "
              f"{res['call_tflops']:.1f} TF); old search {sm:.3f} ms + torch {tm:.3f} ms = {sm + tm:.3f} ms "
              f"({res['speedup_old_over_new']:.2f}x); outputs differ by at most {diff:.2e} ({sets_differ} descriptors "
              f"with another neighbour set), by {diff_same_lists:.2e} over the same lists")
    else:
        print(f"N={N} d={d} k={k} nn={nn}: new {new:.3f} ms")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
