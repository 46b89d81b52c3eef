"""numpy restatement of the 256 x 256 candidate kernel's int8 tail (csrc/knn_b16w.hip
knn_b16w_tile_kernel_i8t, DESIGN.md "int8 tail"): the split column rule, the tail copy, the
arithmetic of one (query, row) product and its error bound e_ip.  Test helper, shared by
tests/test_i8tail_cpu.py and tests/test_i8tail_gpu.py and by tools/i8tail_band.py.
"""
import numpy as np

MIN_TAIL = 512
F32 = np.float32
UP = F32(1.0) + F32(1.0 / 512.0)          # stored norms and residuals are rounded up by this


def block_absmax(x, dpb):
    """Corpus-wide max |x| of every 64-column block of the rows padded to dpb columns."""
    m = np.zeros(dpb, np.float32)
    m[: x.shape[1]] = np.abs(x).max(axis=0)
    return m.reshape(-1, 64).max(axis=1)


def pick_head(blkmax):
    """i8t_pick_head (csrc/knn_plan.cpp): the smallest block boundary from which every block is
    within 2x of the (lower) median of the blocks at or after it; -1 = the route is off."""
    nblk = len(blkmax)
    for j in range(nblk):
        v = np.sort(np.asarray(blkmax[j:], np.float32))
        med = v[(len(v) - 1) // 2]
        b = np.asarray(blkmax[j:], np.float32)
        if np.all(b <= F32(2.0) * med) and np.all(F32(2.0) * b >= med):
            head, dpb = 64 * j, 64 * nblk
            return head if dpb - head >= MIN_TAIL and head <= dpb // 2 else -1
    return -1


def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def pad_cols(x, dpb):
    out = np.zeros((x.shape[0], dpb), np.float32)
    out[:, : x.shape[1]] = x
    return out


def quantize_tail(x, head, dpb, dpt):
    """The tail copy of rows x (n x d fp32): codes (n x dpt int8, pad 0) and scales (n), in the
    kernel's fp32 arithmetic: s = max|x_tail| / 127, c = clamp(rint(x * (127 / max)))."""
    t = pad_cols(x, dpb)[:, head:]
    amax = np.abs(t).max(axis=1).astype(np.float32)
    s = amax / F32(127.0)
    with np.errstate(divide="ignore"):
        inv = np.where(amax > 0, F32(127.0) / amax, F32(0.0)).astype(np.float32)
    c = np.clip(np.rint(t * inv[:, None]), -127, 127).astype(np.int8)
    codes = np.zeros((x.shape[0], dpt), np.int8)
    codes[:, : t.shape[1]] = c
    return codes, s


def row_stats64(x, head, dpb, codes, s):
    """float64 (|x_t - s c|, |x_h - bf16(x_h)|, |x_t|, |x_h|) per row."""
    p = pad_cols(x, dpb).astype(np.float64)
    t, h = p[:, head:], p[:, :head]
    rt = np.linalg.norm(t - s.astype(np.float64)[:, None] * codes[:, : t.shape[1]], axis=1)
    rh = np.linalg.norm(h - bf16_rne(h.astype(np.float32)).astype(np.float64), axis=1)
    return np.stack([rt, rh, np.linalg.norm(t, axis=1), np.linalg.norm(h, axis=1)], 1)


def acc_coef(head):
    """i8t_acc_coef (csrc/knn_plan.cpp)."""
    return F32(1.02 * (5.0 * (head // 16) + 16.0 + 3.0) * 2.0 ** -23)


def approx_ip(xrows, q, head, dpb, dpt):
    """The kernel's approximate q.x for every row: the exact integer dot of the tail codes, folded
    float32(sum) * s_row * s_query in fp32, then the bf16 head's products accumulated on top in
    fp32 (sequentially per 32-column step: a stand-in for the MFMA's own order, which c_acc
    covers)."""
    cx, sx = quantize_tail(xrows, head, dpb, dpt)
    cq, sq = quantize_tail(q[None, :], head, dpb, dpt)
    dot = cx.astype(np.int64) @ cq[0].astype(np.int64)
    assert np.abs(dot).max(initial=0) < 2 ** 31
    acc = dot.astype(np.float32) * sx * sq[0]
    xh = bf16_rne(pad_cols(xrows, dpb)[:, :head])
    qh = bf16_rne(pad_cols(q[None, :], dpb)[0, :head])
    for c0 in range(0, head, 32):
        acc = (acc + (xh[:, c0:c0 + 32].astype(np.float64) @ qh[c0:c0 + 32].astype(np.float64))
               .astype(np.float32)).astype(np.float32)
    return acc


def corpus_maxima(x, head, dpb, dpt):
    """(R_t, R_h, X_t, X_h) as the index stores them: per-row float64 values rounded up."""
    codes, s = quantize_tail(x, head, dpb, dpt)
    st = row_stats64(x, head, dpb, codes, s)
    return (st.max(axis=0) * float(UP)).astype(np.float32)


def e_ip(q, head, dpb, dpt, maxima, xn_max, drop=None):
    """i8tail_e_ip (csrc/knn_certify.h) for one query; `drop` names a term to leave out (the CPU
    test checks that every term is needed)."""
    cq, sq = quantize_tail(q[None, :], head, dpb, dpt)
    st = row_stats64(q[None, :], head, dpb, cq, sq)[0] * float(UP)
    dq_t, dq_h, q_t, q_h = (F32(v) for v in st)
    R_t, R_h, X_t, X_h = (F32(v) for v in maxima)
    qn = F32(np.linalg.norm(q.astype(np.float64)) * float(UP))
    X = F32(np.sqrt(float(xn_max)) * float(UP))
    terms = {
        "qt_Rt": q_t * R_t,
        "dqt_Xt": dq_t * (X_t + R_t),
        "qh_Rh": q_h * R_h,
        "dqh_Xh": dq_h * (X_h + R_h),
        "acc": acc_coef(head) * (qn + dq_t + dq_h) * (X + R_t + R_h),
    }
    tot = F32(0)
    for name, v in terms.items():
        if name != drop:
            tot = F32(tot + v)
    return F32(tot * (F32(1) + F32(1.0 / 256.0)) + F32(1e-30))
