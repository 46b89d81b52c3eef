#!/usr/bin/env python
"""Time VladEncoderTrainer's step at the reference's widths (32768, 669, 317, 128), dropout 0.1,
against what a user runs today on the same card: PyTorch's fp32 step of the same module (train
mode, forward, torch.cdist of the batch and of the codes, both losses, backward(), Adam.step()),
TF32 / reduced-precision matmul off.  Everything is device-resident; weights come from a seed.

Without --step this is a driver: every GPU step runs in a child process of its own under a time
limit, one after the other, and the driver stops at the first step that fails; the steps' JSON
documents are collected into --out.  A machine without a GPU fails.

* --step train --batch B: both paths are warmed up, then timed `--repeats` times with device events,
  alternating, `--inner` steps per timing; medians are reported.
* --step products --batch B: the three big products alone, each as a share of the 155 TF fp32-MFMA
  rate: the first layer's forward (an encoder of the one Linear(32768, 669): its linear, reduce and
  finish launches, depth-split 147 ways), its weight gradient dW_0 = dY^T X (669 x 32768, depth B:
  vladtrain_product_device over transposed copies made beforehand, no depth split from B = 32 on)
  and the Gram matrix X X^T (B x B, depth 32768).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MFMA_F32_FLOPS = 155e12
WIDTHS = (32768, 669, 317, 128)


def params(seed=5):
    import numpy as np
    rng = np.random.default_rng(seed)
    W, b, g, be = [], [], [], []
    for l in range(3):
        K, N = WIDTHS[l], WIDTHS[l + 1]
        W.append(rng.standard_normal((N, K), dtype=np.float32) * np.float32((K ** 0.5 if l == 0 else 1.0) / K ** 0.5))
        b.append((0.1 * rng.standard_normal(N)).astype(np.float32))
        if l < 2:
            g.append((1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32))
            be.append((0.1 * rng.standard_normal(N)).astype(np.float32))
    return W, b, g, be


def batch(torch, B):
    """B unit rows of a Gaussian mixture, as VLAD vectors spread."""
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(3)
    centres = torch.randn((8, WIDTHS[0]), generator=gen, device=dev)
    pick = torch.randint(0, 8, (B,), generator=gen, device=dev)
    x = centres[pick] + 0.7 * torch.randn((B, WIDTHS[0]), generator=gen, device=dev)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def timed(torch, fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def step_train(a) -> dict:
    import numpy as np
    import torch
    from torch import nn
    import torch.nn.functional as F
    from image_recommender_amd.vlad_trainer import VladEncoderTrainer
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda")
    B = a.batch
    W, b, g, be = params()
    tr = VladEncoderTrainer(widths=WIDTHS, params=(W, b, g, be), dropout=0.1, seed=1)
    mods = []
    for l in range(3):
        lin = nn.Linear(WIDTHS[l], WIDTHS[l + 1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W[l]))
            lin.bias.copy_(torch.from_numpy(b[l]))
        mods.append(lin)
        if l < 2:
            ln = nn.LayerNorm(WIDTHS[l + 1])
            with torch.no_grad():
                ln.weight.copy_(torch.from_numpy(g[l]))
                ln.bias.copy_(torch.from_numpy(be[l]))
            mods += [ln, nn.Mish(), nn.Dropout(0.1)]
    seq = nn.Sequential(*mods).to(dev).train()
    opt = torch.optim.Adam(seq.parameters(), lr=1e-3, weight_decay=1e-5)
    x = batch(torch, B)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def run_hip():
        tr.step_device(x.data_ptr(), B, stream=st, losses_ptr=losses.data_ptr())

    def run_torch():
        opt.zero_grad()
        z = F.normalize(seq(x), p=2, dim=-1)
        D_x, D_z = torch.cdist(x, x), torch.cdist(z, z)
        af, bf = D_x.triu(1).flatten(), D_z.triu(1).flatten()
        ac, bc = af - af.mean(), bf - bf.mean()
        corr = 1 - (ac * bc).sum() / (ac.pow(2).sum().sqrt() * bc.pow(2).sum().sqrt() + 1e-8)
        umap = F.kl_div(torch.softmax(-D_z / 1.5, dim=1).log(), torch.softmax(-D_x / 1.5, dim=1), reduction="batchmean")
        (2.0 * corr + 0.25 * umap).backward()
        opt.step()

    for _ in range(3):
        run_hip()
        run_torch()
    torch.cuda.synchronize()
    hip_ms, torch_ms = [], []
    for _ in range(a.repeats):
        hip_ms.append(timed(torch, run_hip, a.inner))
        torch_ms.append(timed(torch, run_torch, a.inner))
    hm, tm = float(np.median(hip_ms)), float(np.median(torch_ms))
    flop = 2.0 * B * WIDTHS[0] * WIDTHS[1] * 2 + 2.0 * B * B * WIDTHS[0]
    res = {"step": "train", "batch": B, "repeats": a.repeats, "inner": a.inner, "hip_ms": hip_ms, "torch_ms": torch_ms,
           "hip_ms_median": hm, "torch_ms_median": tm, "hip_over_torch": hm / tm,
           "within_10_percent_of_torch": hm <= 1.1 * tm, "big_products_gflop": flop / 1e9,
           "big_products_mfma_floor_ms": 1e3 * flop / MFMA_F32_FLOPS, "steps_taken": tr.step_count,
           "last_losses": [float(v) for v in losses.cpu().numpy()]}
    print(f"B={B}: hip {hm:.3f} ms, torch {tm:.3f} ms per step (hip / torch = {hm / tm:.2f}); the three big products are "
          f"{flop / 1e9:.0f} GFLOP = {res['big_products_mfma_floor_ms']:.3f} ms at 155 TF")
    return res


def step_products(a) -> dict:
    import numpy as np
    import torch
    from image_recommender_amd import _lib
    from image_recommender_amd.vlad_encoder import VladEncoder
    dev = torch.device("cuda")
    B, K, N = a.batch, WIDTHS[0], WIDTHS[1]
    W, b, _, _ = params()
    first = VladEncoder(W[:1], b[:1], [], [])
    x = batch(torch, B)
    xt = x.t().contiguous()
    gen = torch.Generator(device=dev).manual_seed(4)
    dyt = torch.randn((N, B), generator=gen, device=dev)
    out1 = torch.empty((B, N), dtype=torch.float32, device=dev)
    dw = torch.empty((N, K), dtype=torch.float32, device=dev)
    gram = torch.empty((B, B), dtype=torch.float32, device=dev)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream

    def product(A, I, Bm, J, depth, out):
        _lib.check(lib.vladtrain_product_device(C.c_void_p(A.data_ptr()), I, C.c_void_p(Bm.data_ptr()), J, depth,
                                                C.c_void_p(out.data_ptr()), C.c_void_p(st or None)), "vladtrain_product_device")

    runs = {
        "forward_layer0": (lambda: first.forward_device(x.data_ptr(), B, out1.data_ptr(), stream=st, model_output=True),
                           2.0 * B * K * N),
        "dW0": (lambda: product(dyt, N, xt, K, B, dw), 2.0 * B * K * N),
        "gram": (lambda: product(x, B, x, B, K, gram), 2.0 * B * B * K),
    }
    for fn, _ in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, (fn, _) in runs.items():
            ms[k].append(timed(torch, fn, a.inner))
    res = {"step": "products", "batch": B, "repeats": a.repeats, "inner": a.inner}
    line = []
    for k, (_, flop) in runs.items():
        m = float(np.median(ms[k]))
        res[k] = {"ms": ms[k], "ms_median": m, "gflop": flop / 1e9, "tflops": flop / (m * 1e-3) / 1e12,
                  "share_of_mfma_limit": flop / (m * 1e-3) / MFMA_F32_FLOPS}
        line.append(f"{k} {m:.3f} ms = {res[k]['tflops']:.1f} TF ({100 * res[k]['share_of_mfma_limit']:.0f} %)")
    want = (dyt.double() @ x.double())
    res["dW0_max_abs_difference_vs_float64"] = (dw.double() - want).abs().max().item()
    print(f"B={B}: " + "; ".join(line))
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="vladtrain_bench.json")
    ap.add_argument("--step", choices=("train", "products"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, nargs="*", default=[128, 1024])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3, help="steps per timing")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per child step")
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))

    if a.step:
        import torch
        if not torch.cuda.is_available():
            print("no GPU: nothing is measured", file=sys.stderr)
            return 2
        res = step_train(a) if a.step == "train" else step_products(a)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return 0

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    steps = [["--step", s, "--batch", str(b)] for b in a.batches for s in ("train", "products")]
    docs = []
    for i, extra in enumerate(steps):
        part = out.with_suffix(f".step{i}.json")
        cmd = [sys.executable, str(Path(__file__).resolve()), *extra, "--out", str(part), "--repeats", str(a.repeats),
               "--inner", str(a.inner)]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"step {' '.join(extra)} ran past {a.step_timeout} s: stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"step {' '.join(extra)} ended with {rc}: stopping", file=sys.stderr)
            return rc
        docs.append(json.loads(part.read_text()))
        part.unlink()
        out.write_text(json.dumps(docs, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
