"""The three IVF-PQ kernels of csrc/ivfpq.hip through their C ABI (include/imgrec_ivfpq.h):

* ivfpq_lut_device against the float64 table within the bound derived from the kernel's arithmetic
  (tests/ivfpq_check.lut_bound), at the tails of its tiling (nr % 8, ksub around 256, dsub 1 and 256),
  and on integer inputs, where the table must equal the float64 one;
* ivfpq_scan_device and ivfpq_scan_all_device, on tables the test supplies, against
  tests/ivfpq_check.expected_scan for equality of the D bytes and of I: no tolerance.

tests/test_ivfpq_check_cpu.py shows that each of these comparisons can fail.  Every output buffer
is pre-filled with NaN (D, lut) or a sentinel (I) and is 256 elements longer than the output:
afterwards the body is written throughout and the tail untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ivfpq_check as ic

pytestmark = pytest.mark.gpu

TAIL = 256
UNSET = -7777            # no label: labels are >= 0 or the padding -1
KNN_EINVAL = -1


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from image_recommender_amd import _lib
    return _lib.load()


def _lut_call(resid, cbt, nr, d, m, ksub, numel):
    """ivfpq_lut_device into a NaN-filled buffer of numel + TAIL floats -> (rc, buffer on the host)."""
    buf = torch.full((numel + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    r, c = torch.from_numpy(resid).cuda(), torch.from_numpy(cbt).cuda()
    rc = _lib().ivfpq_lut_device(_ptr(r), nr, d, m, ksub, _ptr(c), _ptr(buf), _stream())
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy()


def _lut(resid, cbt):
    m, dsub, ksub = cbt.shape
    nr = resid.shape[0]
    rc, buf = _lut_call(resid, cbt, nr, m * dsub, m, ksub, nr * m * ksub)
    assert rc == 0
    assert np.isnan(buf[nr * m * ksub:]).all(), "the kernel wrote past the end of lut"
    lut = buf[:nr * m * ksub].reshape(nr, m, ksub)
    assert not np.isnan(lut).any(), "a table entry was not written"
    return lut


@pytest.mark.parametrize("shape", ic.LUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tables_within_the_derived_bound(gpu, shape):
    resid, cbt = ic.lut_inputs(*shape)
    r = ic.lut_ratio(_lut(resid, cbt), resid, cbt)
    print(f"[ivfpq_lut] {shape}: worst error / bound {r:.3f}")
    assert r <= 1.0, (shape, r)


@pytest.mark.parametrize("shape", [(9, 3, 5, 257), (3, 2, 256, 64), (17, 48, 41, 4096)],
                         ids=lambda s: "x".join(map(str, s)))
def test_tables_equal_float64_on_integers(gpu, shape):
    """Small-integer residuals and codebooks: every entry is an integer below 2^24, so a residual
    row, a sub-quantiser, a dimension or a centroid read at a wrong index cannot hide in a bound."""
    resid, cbt = ic.lut_inputs_int(*shape)
    T, _ = ic.lut_bound(resid, cbt)
    np.testing.assert_array_equal(_lut(resid, cbt).astype(np.float64), T)


@pytest.mark.parametrize("d,m,ksub", [(514, 2, 16),      # dsub = 257
                                      (10, 3, 16),       # d % m != 0
                                      (8, 2, 0)])        # ksub = 0
def test_table_rejections_write_nothing(gpu, d, m, ksub):
    resid = np.ones((4, d), np.float32)
    cbt = np.ones(max(1, d * max(ksub, 1)), np.float32)
    numel = 4 * m * max(ksub, 16)
    rc, buf = _lut_call(resid, cbt, 4, d, m, ksub, numel)
    assert rc == KNN_EINVAL
    assert np.isnan(buf).all()


# ---- the scan routes ----------------------------------------------------------------------------

class _Scan:
    """A scan case on the GPU; scan(k) / scan_all(k) return (D, I) on the host."""

    def __init__(self, case):
        self.c = case
        self.nq, self.nprobe = case["probes"].shape
        self.m, self.ksub = case["m"], case["ksub"]
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()      # (a writable copy: the case is read-only)
        self.lut, self.probes, self.list_off = dev(case["lut"]), dev(case["probes"]), dev(case["list_off"])
        self.codes = dev(case["codes"].view(np.int16))          # the uint16 bytes
        self.ids = dev(case["ids"])
        # probe_off / seg_off as IndexIVFPQ.search builds them
        pr = self.probes.reshape(-1)
        cnt = torch.where(pr >= 0, self.list_off[pr.clamp_min(0) + 1] - self.list_off[pr.clamp_min(0)],
                          torch.zeros_like(pr))
        self.probe_off = (torch.cumsum(cnt, 0) - cnt).contiguous()
        self.total = int(cnt.sum())
        qoff = torch.cat([self.probe_off.reshape(self.nq, self.nprobe)[:, 0],
                          torch.tensor([self.total], dtype=torch.int64, device="cuda")])
        self.seg_off = qoff.to(torch.int32).contiguous()
        _, po, so, total = ic.probe_slots(case["probes"], case["list_off"])
        assert total == self.total and (self.probe_off.cpu().numpy() == po).all()
        assert (qoff.cpu().numpy() == so).all()

    def _run(self, k, call):
        n = self.nq * k
        D = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
        I = torch.full((n + TAIL,), UNSET, dtype=torch.int64, device="cuda")
        assert call(D, I) == 0
        torch.cuda.synchronize()
        D, I = D.cpu().numpy(), I.cpu().numpy()
        assert np.isnan(D[n:]).all() and (I[n:] == UNSET).all(), "the kernel wrote past the end of D / I"
        assert not np.isnan(D[:n]).any() and not (I[:n] == UNSET).any(), "an output entry was not written"
        return D[:n].reshape(self.nq, k), I[:n].reshape(self.nq, k)

    def scan(self, k):
        return self._run(k, lambda D, I: _lib().ivfpq_scan_device(
            _ptr(self.lut), _ptr(self.probes), self.nq, self.nprobe, _ptr(self.list_off), _ptr(self.codes),
            _ptr(self.ids), self.m, self.ksub, k, _ptr(D), _ptr(I), _stream()))

    def scan_all(self, k):
        return self._run(k, lambda D, I: _lib().ivfpq_scan_all_device(
            _ptr(self.lut), _ptr(self.probes), self.nq, self.nprobe, _ptr(self.list_off), _ptr(self.codes),
            _ptr(self.ids), self.m, self.ksub, _ptr(self.probe_off), _ptr(self.seg_off), self.total, k,
            _ptr(D), _ptr(I), _stream()))

    def expected(self, k):
        c = self.c
        return ic.expected_scan(c["lut"], c["probes"], c["list_off"], c["codes"], c["ids"], k)


def _same(got, want, what):
    (D, I), (De, Ie) = got, want
    assert D.dtype == np.float32 and De.dtype == np.float32
    bad = np.nonzero((D.view(np.uint32) != De.view(np.uint32)) | (I != Ie))
    assert bad[0].size == 0, (f"{what}: {bad[0].size} entries differ, first at query {bad[0][0]} rank {bad[1][0]}: "
                              f"({D[bad][0]!r}, {I[bad][0]}) instead of ({De[bad][0]!r}, {Ie[bad][0]})")


@pytest.mark.parametrize("table", ["random", "ties"])
def test_both_scan_routes_equal_the_expected_bytes(gpu, table):
    s = _Scan(ic.scan_case(table))
    for k in ic.SCAN_ALL_KS:
        want = s.expected(k)
        all_ = s.scan_all(k)
        _same(all_, want, f"scan_all, {table} table, k = {k}")
        if k <= 32:
            reg = s.scan(k)
            _same(reg, want, f"scan, {table} table, k = {k}")
            _same(reg, all_, f"scan against scan_all, {table} table, k = {k}")


def test_both_scan_routes_at_the_reference_code_shape(gpu):
    s = _Scan(ic.scan_case_wide())
    _same(s.scan(10), s.expected(10), "scan, m = 48, ksub = 4096, k = 10")
    _same(s.scan_all(10), s.expected(10), "scan_all, m = 48, ksub = 4096, k = 10")
    _same(s.scan_all(40), s.expected(40), "scan_all, m = 48, ksub = 4096, k = 40")


def test_scan_all_probes_none(gpu):
    """Every probe of every query -1: total = 0 in the sort route, nothing but padding."""
    c = dict(ic.scan_case("random"))
    c["probes"] = np.full_like(c["probes"], -1)
    s = _Scan(c)
    assert s.total == 0
    for got in (s.scan(5), s.scan_all(5), s.scan_all(40)):
        assert (got[1] == -1).all() and (got[0] == ic.FLT_MAX).all()


def test_write_slices_of_65535_queries(gpu):
    """nq = 65539: the sort route writes D / I in two slices, the second from query 65535 on (its
    offsets into D, I and seg_off); the register route is one workgroup per query."""
    s = _Scan(ic.scan_case_slices())
    want = s.expected(33)
    _same(s.scan_all(33), want, "scan_all, nq = 65539, k = 33")
    assert (want[1][65535:, 0] >= 0).sum() >= 2          # the second slice holds real results
    _same(s.scan(32), s.expected(32), "scan, nq = 65539, k = 32")
