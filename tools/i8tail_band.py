#!/usr/bin/env python3
"""Certificate band of the 256 x 256 candidate pass's arithmetics on bench.py's generators, on the
CPU (no GPU, no native library): how many rows have an approximate key within 2 E_a of the
query's 10th best, against K' = 64 candidates (DESIGN.md "int8 tail"; the gate of
tools/i8_mfma_gate.py for this route).

Arithmetics:
  bf16        bf16 rows and query (the pure bf16 pass), bound |q| R + dq (X + R)
  i8tail      bf16 head H columns + int8 tail with one scale per row and per query, the
              per-segment bound i8tail_e_ip (tests/i8tail_ref.py restates kernel and bound)
  i8tail-lump the same arithmetic with the lumped bound |q| R + dq (X + R), R = R_t + R_h

Usage: python tools/i8tail_band.py [--rows 1000000] [--queries 64] [--config 3] [--out FILE]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (the generators)
from tests import i8tail_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    cfg = bench.CONFIGS[a.config]
    seed = a.config
    centres = bench.make_centres(torch, cfg, "cpu", seed)
    q = bench.gen_queries(torch, cfg, centres, a.queries, "cpu", seed).numpy()
    d = q.shape[1]
    dpb = (d + 63) // 64 * 64
    # pass 1: the split column from the corpus's block maxima
    blk = np.zeros(dpb // 64, np.float32)
    for x in bench.gen_rows(torch, cfg, centres, 0, a.rows, "cpu", seed):
        blk = np.maximum(blk, R.block_absmax(x.numpy(), dpb))
    head = R.pick_head(blk)
    assert head >= 0, "the index is not eligible"
    dpt = (dpb - head + 127) // 128 * 128
    # pass 2: approximate and exact keys, corpus maxima
    q64 = q.astype(np.float64)
    qn = (q64 * q64).sum(1)
    qb = R.bf16_rne(q)
    cq, sq = R.quantize_tail(q, head, dpb, dpt)
    qh = R.bf16_rne(R.pad_cols(q, dpb)[:, :head])
    keys = {"bf16": [], "i8tail": []}
    exact = []
    mx = np.zeros(4)
    rb_max = xn_max = 0.0
    for x in bench.gen_rows(torch, cfg, centres, 0, a.rows, "cpu", seed):
        x = x.numpy()
        x64 = x.astype(np.float64)
        xn = (x64 * x64).sum(1)
        xn_max = max(xn_max, float(xn.max()))
        exact.append((qn[:, None] + xn[None, :] - 2.0 * q64 @ x64.T).astype(np.float32))
        xb = R.bf16_rne(x)
        rb_max = max(rb_max, float(np.linalg.norm(x64 - xb.astype(np.float64), axis=1).max()))
        ipb = (qb.astype(np.float64) @ xb.astype(np.float64).T)
        keys["bf16"].append((qn[:, None] + xn[None, :] - 2.0 * ipb).astype(np.float32))
        codes, s = R.quantize_tail(x, head, dpb, dpt)
        mx = np.maximum(mx, R.row_stats64(x, head, dpb, codes, s).max(axis=0))
        # R.approx_ip for all queries at once (the integer dots are exact in float64)
        dot = cq.astype(np.float64) @ codes.astype(np.float64).T
        ipt = dot.astype(np.float32) * s[None, :] * sq[:, None]
        xh = R.bf16_rne(R.pad_cols(x, dpb)[:, :head])
        for c0 in range(0, head, 32):
            ipt = (ipt + (qh[:, c0:c0 + 32].astype(np.float64) @ xh[:, c0:c0 + 32].astype(np.float64).T)
                   .astype(np.float32)).astype(np.float32)
        keys["i8tail"].append((qn[:, None] + xn[None, :] - 2.0 * ipt.astype(np.float64)).astype(np.float32))
    exact = np.concatenate(exact, 1)
    keys = {k_: np.concatenate(v, 1) for k_, v in keys.items()}
    keys["i8tail-lump"] = keys["i8tail"]
    maxima = (mx * float(R.UP)).astype(np.float32)
    X = np.sqrt(xn_max)
    # bounds per query
    dq_b = np.linalg.norm(q64 - qb.astype(np.float64), axis=1)
    e = {"bf16": np.sqrt(qn) * rb_max + dq_b * (X + rb_max)}
    e["i8tail"] = np.array([float(R.e_ip(q[i], head, dpb, dpt, maxima, xn_max)) for i in range(a.queries)])
    lump = []
    for i in range(a.queries):
        cq, sq = R.quantize_tail(q[i][None, :], head, dpb, dpt)
        st = R.row_stats64(q[i][None, :], head, dpb, cq, sq)[0]
        Rl = float(maxima[0] + maxima[1])
        lump.append(np.sqrt(qn[i]) * Rl + (st[0] + st[1]) * (X + Rl))
    e["i8tail-lump"] = np.array(lump)
    res = {"rows": a.rows, "queries": a.queries, "config": a.config, "k": a.k, "head": head, "dpt": dpt,
           "maxima_Rt_Rh_Xt_Xh": [float(v) for v in maxima], "arithmetics": {}}
    for name, ky in keys.items():
        Ea = 2.0 * e[name]
        kth = np.partition(ky, a.k - 1, axis=1)[:, a.k - 1]
        band = (ky <= (kth + 2.0 * Ea)[:, None]).sum(1)
        res["arithmetics"][name] = {
            "E_a_median": float(np.median(Ea)),
            "band_median_p90_max": [float(np.median(band)), float(np.percentile(band, 90)), int(band.max())],
            "max_key_error": float(np.abs(ky.astype(np.float64) - exact).max()),
            "queries_over_64": int((band > 64).sum()),
        }
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
