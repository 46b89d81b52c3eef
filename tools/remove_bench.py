"""remove_ids cost on 1M x 1968 rows (tests.datagen.concat_rows, generated on the host in blocks)
with the bf16 and the int8 copy materialised, beside the only route there was before it and a copy
floor.  Measurement tool (not bench.py); prints one JSON line per removal pattern.

Patterns: 1 % of the rows at random, 50 % at random, one contiguous 1 % block at the front.
Per pattern and repeat, on an index that has just been rebuilt from all rows:
  remove_ms   host clock around index.remove_ids(ids) (the call waits for the device);
  rebuild_ms  (a) host clock around index.reset() + index.add(survivors) from host memory, the route
              without remove_ids (the add re-derives the bf16 and int8 copies as it goes); the
              survivors' host array is prepared outside the timed window;
and once per pattern
  floor_ms    (b) 4 x moved bytes / the device-to-device copy rate measured in this run on a buffer
              of the moved size (at most 4 GiB), moved bytes = (surviving rows from the first
              removed row on) x the bytes per row of every per-row array the index holds.
The medians over the repeats, the minimum and maximum, remove_ms as a multiple of the floor and
rebuild_ms over remove_ms are reported; the first and last 4,096 stored rows after a removal are
compared with the survivors'.

ROWS=<n> shrinks the corpus (rehearsal), REPS=<n> sets the repeats per pattern (default 3).
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from image_recommender_amd import faiss_compat as faiss  # noqa: E402
from tests.datagen import concat_rows  # noqa: E402

BLOCK = 50_000


def host_rows(n):
    out = np.empty((n, 1968), dtype=np.float32)
    for b, r0 in enumerate(range(0, n, BLOCK)):
        out[r0:r0 + BLOCK] = concat_rows(min(BLOCK, n - r0), seed=3 + b)
    return out


def row_bytes(d):
    """Bytes per stored row over every per-row array of an index with the bf16 and int8 copies:
    fp32 row (stride padded to 32 floats from d >= 256), norm, bf16 row (stride padded to 64
    elements) + residual, int8 blocks of 64 + one scale per block + residual."""
    dp = -(-d // 32) * 32 if d >= 256 else -(-d // 16) * 16
    dpb = -(-d // 64) * 64
    nblk = -(-d // 64)
    return dp * 4 + 4 + dpb * 2 + 4 + nblk * 64 + nblk * 4 + 4


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def d2d_rate(nbytes, dev):
    """Bytes per second of a device-to-device copy of nbytes (bytes copied, not read + written)."""
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for _ in range(2):
        b.copy_(a)
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return nbytes / (float(np.median(ts)) * 1e-3)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rows = int(os.environ.get("ROWS", 1_000_000))
    reps = int(os.environ.get("REPS", 3))
    d = 1968
    xb = host_rows(rows)
    xq = np.ascontiguousarray(xb[:4])
    idx = faiss.IndexFlatL2(d, device=0)
    idx.reserve(rows)

    def rebuild():
        idx.reset()
        idx.add(xb)

    rebuild()
    idx.search(xq, 10)                        # AUTO, 4 queries: the int8 copy
    idx.search_mode = "bf16"
    idx.search(xq, 10)                        # (the bf16 copy exists from the first add)
    idx.search_mode = "auto"

    rng = np.random.default_rng(17)
    u = rng.random(rows)
    front = np.zeros(rows, dtype=bool)
    front[:rows // 100] = True
    for tag, mask in (("1% random", u < 0.01), ("50% random", u < 0.5), ("1% block at the front", front)):
        ids = np.nonzero(mask)[0]
        left = np.ascontiguousarray(xb[~mask])
        moved = (len(left) - int(ids[0])) * row_bytes(d)
        rate = d2d_rate(min(moved, 4 << 30), dev)
        t_rm, t_rb = [], []
        ok = True
        for _ in range(reps):
            t_rm.append(wall_ms(lambda: idx.remove_ids(ids)))
            n = idx.ntotal
            c = min(4096, n)
            ok = ok and n == len(left) and \
                idx.reconstruct_n(0, c).tobytes() == left[:c].tobytes() and \
                idx.reconstruct_n(n - c, c).tobytes() == left[n - c:].tobytes()
            t_rb.append(wall_ms(lambda: (idx.reset(), idx.add(left))))
            rebuild()
        rm, rb = stats(t_rm), stats(t_rb)
        floor_ms = 4 * moved / rate * 1e3
        print(json.dumps({
            "rows": rows, "d": d, "pattern": tag, "removed": int(mask.sum()), "moved_bytes": moved,
            "remove_ms": rm, "rebuild_ms": rb, "rebuild_over_remove": rb["median"] / rm["median"],
            "d2d_GBps": rate / 1e9, "floor_ms": floor_ms, "remove_over_floor": rm["median"] / floor_ms,
            "rows_equal_survivors": bool(ok), "reps": reps}), flush=True)
        del left


if __name__ == "__main__":
    main()
