#!/usr/bin/env python
"""Time VladEncoder.forward_device at the reference's widths (32768, 669, 317, 128) against what the
reference itself would run on the same card: PyTorch's fp32 eval forward of the same nn.Sequential
with the same weights, F.normalize and the division by (norm + 1e-7), TF32 / reduced-precision
matmul off.  Everything is device-resident; weights come from a seed.

Without --step this is a driver: every GPU step (a batch size, or the descriptor pipeline) runs in
a child process of its own under a time limit, one after the other, and the driver stops at the first
step that fails; the steps' JSON documents are collected into --out.  A machine without a GPU fails.

* --step forward --batch B: both paths are warmed up, then timed `--repeats` times with device
  events, alternating, `--inner` calls per timing; medians are reported.  Also timed: the first
  layer alone (an encoder of the one Linear(32768, 669): its linear and finish launches), which is
  what the two floors are held against: one read of the 87.7 MB of weights plus the input at the
  HBM rate (6.29 TB/s measured, the figure tools/bench_vlad.py uses), and 2 B 669 32768 FLOP at the
  fp32-MFMA rate (155 TF measured).  These are a call's shares, not a kernel's.
* --step pipeline: encode_images (descriptors to stored vectors, the VLAD vectors stay on the device)
  against the host round trip SoftVLAD.encode then VladEncoder.forward, at --nimg images of --per
  descriptors, host clock around calls that end synchronised.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MFMA_F32_FLOPS = 155e12
HBM_BYTES_PER_S = 6.29e12
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


def step_forward(a) -> dict:
    import numpy as np
    import torch
    from torch import nn
    import torch.nn.functional as F
    from image_recommender_amd.vlad_encoder import VladEncoder
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda")
    B = a.batch
    W, b, g, be = params()
    enc = VladEncoder(W, b, g, be)
    first = VladEncoder(W[:1], b[:1], [], [])
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
    seq = nn.Sequential(*mods).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn((B, WIDTHS[0]), generator=gen, device=dev)
    x /= x.norm(dim=1, keepdim=True)                     # unit rows, as VLAD vectors are
    out = torch.empty((B, WIDTHS[-1]), dtype=torch.float32, device=dev)
    out1 = torch.empty((B, WIDTHS[1]), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def run_hip():
        enc.forward_device(x.data_ptr(), B, out.data_ptr(), stream=st)

    def run_first():
        first.forward_device(x.data_ptr(), B, out1.data_ptr(), stream=st, model_output=True)

    def run_torch():
        with torch.no_grad():
            z = F.normalize(seq(x), p=2, dim=-1)
            return z / (z.norm(dim=1, keepdim=True) + 1e-7)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.inner, r

    for _ in range(3):
        run_hip()
        run_first()
        run_torch()
    torch.cuda.synchronize()
    hip_ms, first_ms, torch_ms = [], [], []
    ref = None
    for _ in range(a.repeats):
        hip_ms.append(timed(run_hip)[0])
        t, ref = timed(run_torch)
        torch_ms.append(t)
        first_ms.append(timed(run_first)[0])
    hm, tm, fm = (float(np.median(v)) for v in (hip_ms, torch_ms, first_ms))
    nbytes = 4.0 * (WIDTHS[0] * WIDTHS[1] + B * WIDTHS[0])
    flop = 2.0 * B * WIDTHS[0] * WIDTHS[1]
    res = {
        "step": "forward", "batch": B, "repeats": a.repeats, "inner": a.inner,
        "hip_ms": hip_ms, "torch_ms": torch_ms, "first_layer_ms": first_ms,
        "hip_ms_median": hm, "torch_ms_median": tm, "first_layer_ms_median": fm,
        "hip_over_torch": hm / tm, "within_10_percent_of_torch": hm <= 1.1 * tm,
        "first_layer_hbm_floor_ms": 1e3 * nbytes / HBM_BYTES_PER_S, "first_layer_mfma_floor_ms": 1e3 * flop / MFMA_F32_FLOPS,
        "first_layer_share_of_hbm_limit": (1e3 * nbytes / HBM_BYTES_PER_S) / fm,
        "first_layer_share_of_mfma_limit": (1e3 * flop / MFMA_F32_FLOPS) / fm,
        "first_layer_tflops": flop / (fm * 1e-3) / 1e12, "first_layer_tb_per_s": nbytes / (fm * 1e-3) / 1e12,
        "max_abs_difference_hip_vs_torch": (out - ref).abs().max().item(),
    }
    print(f"B={B}: hip {hm:.4f} ms, torch {tm:.4f} ms (hip / torch = {hm / tm:.2f}); first layer alone {fm:.4f} ms = "
          f"{res['first_layer_tb_per_s']:.2f} TB/s, {res['first_layer_tflops']:.1f} TF; outputs differ by at most "
          f"{res['max_abs_difference_hip_vs_torch']:.2e}")
    return res


def step_pipeline(a) -> dict:
    import numpy as np
    import torch
    from image_recommender_amd.vlad import SoftVLAD, rootsift
    from image_recommender_amd.vlad_encoder import VladEncoder
    rng = np.random.default_rng(9)
    descs = [rootsift(rng.gamma(0.6, 1.0, (a.per, 128)) * (rng.uniform(size=(a.per, 128)) < 0.35)) for _ in range(a.nimg)]
    cb = np.concatenate(descs)[rng.choice(a.nimg * a.per, 256, replace=False)]
    sv = SoftVLAD(cb)
    enc = VladEncoder(*params())

    def host_clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), r

    for _ in range(2):
        enc.encode_images(sv, descs)
        enc.forward(sv.encode(descs))
    dev_ms, host_ms = [], []
    for _ in range(a.repeats):
        t, got = host_clock(lambda: enc.encode_images(sv, descs))
        dev_ms.append(t)
        t, want = host_clock(lambda: enc.forward(sv.encode(descs)))
        host_ms.append(t)
    dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
    res = {"step": "pipeline", "nimg": a.nimg, "per_image": a.per, "repeats": a.repeats,
           "encode_images_ms": dev_ms, "host_round_trip_ms": host_ms, "encode_images_ms_median": dm,
           "host_round_trip_ms_median": hm, "round_trip_over_encode_images": hm / dm,
           "byte_equal": bool(got.tobytes() == want.tobytes())}
    print(f"{a.nimg} images x {a.per} descriptors: encode_images {dm:.2f} ms, encode then forward over the host "
          f"{hm:.2f} ms ({hm / dm:.2f}x); byte-equal: {res['byte_equal']}")
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="vladenc_bench.json")
    ap.add_argument("--step", choices=("forward", "pipeline"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 128, 1024])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="calls per timing")
    ap.add_argument("--nimg", type=int, default=128)
    ap.add_argument("--per", type=int, default=1000, help="descriptors per image")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per child step")
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))

    if a.step:
        import torch
        if not torch.cuda.is_available():
            print("no GPU: nothing is measured", file=sys.stderr)
            return 2
        res = step_forward(a) if a.step == "forward" else step_pipeline(a)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return 0

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    steps = [["--step", "forward", "--batch", str(b)] for b in a.batches] + [["--step", "pipeline"]]
    docs = []
    for i, extra in enumerate(steps):
        part = out.with_suffix(f".step{i}.json")
        cmd = [sys.executable, str(Path(__file__).resolve()), *extra, "--out", str(part), "--repeats", str(a.repeats),
               "--inner", str(a.inner), "--nimg", str(a.nimg), "--per", str(a.per)]
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
