"""Throughput of the device LANCZOS resize (csrc/resize.hip) beside the host path it replaces.

For each input size: a batch of --images random RGB images is resized to 224 x 224 float32 CHW by
lanczos_resize_device (HIP events around the whole call: table upload and both kernels; warm-up,
then the median of --runs), and the same decoded arrays go through what load_image does after the
decode (Image.resize(LANCZOS), float32 / 255) on --threads host threads.  Reports images/s of
both, the bytes the kernels must read (the input, once) over the device time as a share of the
HBM rate, and checks a few device results against Pillow.  One JSON line per size.

Usage: python tools/bench_resize.py [--images 512] [--sizes 256x256,1024x768] [--runs 30]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

HBM_SPEC = 8.0e12        # bytes/s, MI355X datasheet
HBM_COPY = 6.29e12       # bytes/s, measured float4 copy


def host_resize(arr):
    from PIL import Image
    img = Image.fromarray(arr).resize((224, 224), resample=Image.Resampling.LANCZOS)
    return (np.asarray(img).astype(np.float32) / 255.0).transpose(2, 0, 1)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--sizes", default="256x256,1024x768", help="WxH,...")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    from image_recommender_amd.resize import lanczos_resize_device
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs a HIP device")
    n = a.images
    for spec in a.sizes.split(","):
        w, h = (int(v) for v in spec.split("x"))
        g = torch.Generator(device="cuda").manual_seed(h * 10007 + w)
        per = h * w * 3
        stride = -(-per // 48) * 48
        pixels = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device="cuda", generator=g)
        offsets = [i * stride for i in range(n)]
        shapes = [(h, w)] * n
        out = torch.empty((n, 3, 224, 224), dtype=torch.float32, device="cuda")
        for _ in range(a.warmup):
            lanczos_resize_device(pixels, offsets, shapes, (224, 224), "f32", out=out)
        torch.cuda.synchronize()
        dev_ms, call_ms = [], []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            lanczos_resize_device(pixels, offsets, shapes, (224, 224), "f32", out=out)
            e1.record()
            call_ms.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        med = statistics.median(dev_ms)
        host_px = pixels.cpu().numpy()
        arrs = [host_px[o:o + per].reshape(h, w, 3) for o in offsets]
        got = out[:4].cpu().numpy()
        for k in range(4):
            if not np.array_equal(got[k].view(np.uint32), np.ascontiguousarray(host_resize(arrs[k])).view(np.uint32)):
                raise SystemExit(f"device result {k} at {spec} differs from Pillow")
        with ThreadPoolExecutor(max_workers=a.threads) as ex:
            list(ex.map(host_resize, arrs[:2 * a.threads]))            # warm the pool
            cpu_s = []
            for _ in range(3):
                t0 = time.perf_counter()
                list(ex.map(host_resize, arrs))
                cpu_s.append(time.perf_counter() - t0)
        cpu = statistics.median(cpu_s)
        bytes_in = n * per
        print(json.dumps({
            "size": spec, "images": n, "runs": a.runs,
            "device_ms_median": round(med, 4), "device_ms_min": round(min(dev_ms), 4),
            "device_ms_max": round(max(dev_ms), 4),
            "enqueue_ms_median": round(statistics.median(call_ms), 4),
            "device_images_per_s": round(n / (med * 1e-3)),
            "input_GB_per_s": round(bytes_in / (med * 1e-3) / 1e9, 1),
            "share_of_hbm_spec": round(bytes_in / (med * 1e-3) / HBM_SPEC, 4),
            "share_of_hbm_copy_rate": round(bytes_in / (med * 1e-3) / HBM_COPY, 4),
            "host_threads": a.threads, "host_s_median": round(cpu, 4),
            "host_images_per_s": round(n / cpu),
        }), flush=True)


if __name__ == "__main__":
    main()
