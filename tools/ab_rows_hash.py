"""Hashes of what the kernels on the row tile's stage stream (csrc/rows_tile.h) return on the suite's
seeded cases, for A/B bit-identity of library variants (run once per IMGREC_LIB_NAME; equal hashes =
identical results).  One line per case:

    kmeans <case> plain|spherical   the five outputs of kmeans_step_device, every kmeans_check.CASES
                                    entry (spherical: rows and centroids L2-normalised first)
    vlad <case>                     (vlad, raw, nn_idx, nn_dist) of vlad_encode_device, every
                                    vlad_check.CASES entry
    vladenc <case>                  (stored, model, hidden) of vladenc_forward_device at each of the
                                    case's batch sizes, every vladenc_check.CASES entry

Usage: IMGREC_LIB_NAME=libimgrec_x.so python tools/ab_rows_hash.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.ab_result_hash import digest  # noqa: E402


def main():
    from image_recommender_amd import _lib
    from image_recommender_amd.vlad_encoder import VladEncoder
    from tests import kmeans_check as kc, vlad_check as vc, vladenc_check as ec
    from tests.test_kmeans_gpu import gpu_step
    from tests.test_vlad_gpu import gpu_encode
    from tests.test_vladenc_gpu import gpu_forward
    lib = os.environ.get("IMGREC_LIB_NAME", "libimgrec.so")
    for cs in kc.CASES:
        x, c = kc.case_data(cs.name)
        xs = np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))
        cn = np.ascontiguousarray(c / np.linalg.norm(c, axis=1, keepdims=True))
        for tag, a, b, flags in (("plain", x, c, 0), ("spherical", xs, cn, _lib.KMEANS_SPHERICAL)):
            out = gpu_step(a, b, flags=flags, part=cs.part)
            print(f"{lib} kmeans {cs.name} {tag} {digest(*out[:4], np.float64(out[4]))}", flush=True)
    for cs in vc.CASES:
        x, off, c = vc.case_data(cs.name)
        vlad, idx, dist = gpu_encode(x, off, c, cs.nn, cs.sigma)
        raw = gpu_encode(x, off, c, cs.nn, cs.sigma, raw=True)[0]
        print(f"{lib} vlad {cs.name} {digest(vlad, raw, idx, dist)}", flush=True)
    for cs in ec.CASES:
        p = ec.case_params(cs.name)
        enc = VladEncoder(p.W, p.b, p.g, p.be, ln_eps=p.eps)
        outs = []
        for n in cs.batches:
            x = ec.case_input(cs.name, n)
            stored, hidden = gpu_forward(enc, x)
            outs += [stored, gpu_forward(enc, x, model_output=True)[0], hidden]
        enc.close()
        print(f"{lib} vladenc {cs.name} {digest(*outs)}", flush=True)


if __name__ == "__main__":
    main()
