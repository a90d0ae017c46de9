"""conv_wgrad_kernel and the split-K reduce at operator level, through tbn_conv2d_wgrad_tile: every tile instantiation in both
kernel modes with and without split-K, pitched operands, and the edges of the kernel's incremental row arithmetic (maps
smaller than one 64-row step, one-column and one-pixel maps, a last split that runs past the last frame, stride 2 on odd
maps, the strided 1x1, valid 3x3, 5x5 / 7x7 filters, channel counts that are multiples of 4 only).

The backbone of the file are EXACT cases (tests/wgrad_check.py): small integers times a power of two per channel, so that
every product and every partial sum of an entry is exactly representable in fp32 and the result must equal the float64
reference bit for bit whatever the summation order -- no tolerance, a wrong row, tap, border decision, column or dropped
slab is a failure.  tests/test_wgrad_plan_cpu.py holds the census of what the case table reaches.

Buffers: dy and x are column slices of wider NaN-filled buffers with a NaN guard row below (and a dense twin), dW carries a
NaN tail and is NaN-filled before the call, the workspace is NaN-filled: the kernel leaves rows >= M and ragged column tiles
to the hardware range check, and whatever it reads beyond an operand must never reach a stored entry."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import call, lib, ptr  # noqa: E402
from tests import wgrad_check as wc  # noqa: E402

DEV = "cuda"
NAN = float("nan")
TAIL = 256


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


class Wide:
    """a (rows + 1, ld) NaN buffer and the column slice [col, col + c) of its first `rows` rows (tests/test_bn_batch_gpu.py)"""

    def __init__(self, data, ld=None, col=0):
        rows, c = data.shape
        self.ld = c if ld is None else ld
        self.buf = torch.full((rows + 1, self.ld), NAN, device=DEV)
        self.view = self.buf[:rows, col:col + c]
        self.view.copy_(data.to(DEV))
        self.snap = self.buf.clone()

    def unchanged(self):
        return torch.equal(bits(self.buf), bits(self.snap))


class Problem:
    """one case on the device: dy (M, cout) and x (n h w, cin), pitched (cout + 24 at column 8, cin + 40 at column 12) or dense"""

    def __init__(self, geom, cin, cout, dy, x, pitched):
        self.geom, self.cin, self.cout = geom, cin, cout
        dy2, x2 = dy.reshape(-1, cout), x.reshape(-1, cin)
        self.dy = Wide(dy2, cout + 24, 8) if pitched else Wide(dy2)
        self.x = Wide(x2, cin + 40, 12) if pitched else Wide(x2)
        n, h, w, k, stride, pad = geom
        self.numel = cout * k * k * cin
        self.nws = lib().tbn_conv2d_wgrad_workspace_floats(n, h, w, cin, cout, k, stride, pad)

    def run(self, tile=(0, 0), entry="tbn_conv2d_wgrad_tile", expect_ok=True):
        """one call into NaN-filled dW / workspace; returns (rc, dW on the host) after the buffer checks"""
        n, h, w, k, stride, pad = self.geom
        dw = torch.full((self.numel + TAIL,), NAN, device=DEV)
        ws = torch.full((max(self.nws, 1),), NAN, device=DEV)
        args = [self.dy.view.data_ptr(), self.dy.ld, self.x.view.data_ptr(), self.x.ld, ptr(dw), n, h, w, self.cin, self.cout,
                k, stride, pad]
        if entry == "tbn_conv2d_wgrad_tile":
            args += [tile[0], tile[1]]
        rc = getattr(lib(), entry)(*args, ptr(ws), st())
        torch.cuda.synchronize()
        assert self.dy.unchanged() and self.x.unchanged(), "an input buffer was written"
        assert bool(torch.isnan(dw[self.numel:]).all()), "dW written beyond its last entry"
        if expect_ok:
            assert rc == 0, lib().tbn_last_error()
            assert not bool(torch.isnan(dw[:self.numel]).any()), "NaN inside dW: an entry not written, or fed from beyond an operand"
        else:
            assert rc < 0 and bool(torch.isnan(dw).all()), "a refused call wrote dW"
        return rc, dw[:self.numel].reshape(self.cout, k, k, self.cin).cpu()


_DATA = {}


def exact_data(geom, cin, cout):
    """(dy, x, float64 reference cast to fp32) of an exact case, computed once"""
    key = (geom, cin, cout)
    if key not in _DATA:
        dy, x = wc.exact_case(geom, cin, cout, seed=sum(v * 131 ** i for i, v in enumerate(geom + (cin, cout))))
        ref = wc.reference(dy, x, geom)
        assert torch.equal(ref.float().double(), ref)
        _DATA[key] = (dy, x, ref.float())
    return _DATA[key]


def first_mismatch(got, ref):
    bad = (got != ref).nonzero()
    return "%d of %d entries differ, first (co, r, s, ci) = %s: got %r, reference %r" % (
        bad.shape[0], ref.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])])) if bad.shape[0] else ""


@pytest.mark.parametrize("case", wc.EXACT_CASES, ids=wc.case_id)
def test_exact_heuristic_tile(case):
    """every geometry x channel pair at the heuristic tile, pitched and dense: bit-equal to the float64 reference"""
    geom, cin, cout, tile = case
    dy, x, ref = exact_data(geom, cin, cout)
    for pitched in (True, False):
        _, got = Problem(geom, cin, cout, dy, x, pitched).run(tile)
        assert torch.equal(got, ref), (pitched, first_mismatch(got, ref))


def profiled(fn, tmp_path):
    """runs fn with the library profiler (conv-GEMM launches) and the kernel timeline (every other launch, the split-K reduce
    among them) recording; returns ({profiler entry: launches}, [timeline kernel names])"""
    L = lib()
    L.tbn_profile_reset()
    L.tbn_profile_enable(1)
    L.tbn_timeline_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.tbn_profile_enable(0)
        L.tbn_timeline_enable(0)
    prof, name = {}, C.create_string_buffer(160)
    for i in range(L.tbn_profile_num_entries()):
        cnt, ms, fl = C.c_long(), C.c_double(), C.c_double()
        L.tbn_profile_entry(i, name, 160, C.byref(cnt), C.byref(ms), C.byref(fl))
        prof[name.value.decode()] = cnt.value
    L.tbn_profile_reset()
    path = str(tmp_path / "timeline.csv")
    call("tbn_timeline_dump", path.encode())
    with open(path) as f:
        rows = [ln.split(",")[0] for ln in f.read().splitlines()[1:]]
    return prof, rows


@pytest.mark.parametrize("case", wc.TILE_CASES, ids=wc.case_id)
def test_exact_every_tile(case, tmp_path):
    """all 11 tiles at channel counts ragged under every one of them, general and pointwise, without and with split-K: bit-equal
    to the reference pitched and dense, and the kernel instantiation (and split-K reduce) that ran is the one the plan names"""
    geom, cin, cout, tile = case
    dy, x, ref = exact_data(geom, cin, cout)
    q = wc.plan(lib(), geom, cin, cout, tile)
    assert (q["mt"], q["nt"]) == tile
    pitched, dense = Problem(geom, cin, cout, dy, x, True), Problem(geom, cin, cout, dy, x, False)
    out = {}
    prof, timeline = profiled(lambda: out.update(p=pitched.run(tile)[1]), tmp_path)
    out["d"] = dense.run(tile)[1]
    assert torch.equal(out["p"], ref), first_mismatch(out["p"], ref)
    assert torch.equal(out["d"], ref), first_mismatch(out["d"], ref)
    assert prof == {"conv_wgrad_kernel<%d, %d, %d>" % (tile[0], tile[1], q["mode"]): 1}, (prof, q)
    reduces = [k for k in timeline if "splitk_reduce" in k]
    assert reduces == (["splitk_reduce_kernel<%d>" % q["reduce"]] if q["splits"] > 1 else []), (timeline, q)


@pytest.mark.parametrize("case", wc.FLOAT_CASES, ids=wc.case_id)
def test_float_accumulation_error_per_entry(case):
    """Gaussian dy, post-ReLU-like x, channel scales over three decades, under split-K: every entry within
    2 (M + 1) 2^-24 A of the float64 reference, A = the entry's sum of absolute products.  (M + 1) 2^-24 A bounds an fp32 sum
    of M rounded products in any order; the factor 2 covers the two-term step inside the fp32 MFMA.
    Measured on an MI355X, largest |err| / (2^-24 A) over the entries: 0.97 for the 3x3 case (M = 286, bound 574), 0.83 for the
    1x1 case (M = 297, bound 596), pitched and dense alike -- the errors of the products cancel far below their worst case."""
    geom, cin, cout, tile = case
    dy, x = wc.float_case(geom, cin, cout, seed=77)
    ref, a = wc.reference(dy, x, geom), wc.abs_reference(dy, x, geom)
    M = wc.rows(geom)
    assert wc.plan(lib(), geom, cin, cout, tile)["splits"] > 1 and float(a.min()) > 0
    for pitched in (True, False):
        _, got = Problem(geom, cin, cout, dy, x, pitched).run(tile)
        ratio = ((got.double() - ref).abs() / (2.0 ** -24 * a)).max()
        print("wgrad float case %s pitched=%d: M = %d, max |err| / (2^-24 A) = %.3f (bound %d)" % (
            wc.case_id(case), pitched, M, float(ratio), 2 * (M + 1)))
        assert ((got.double() - ref).abs() <= 2 * (M + 1) * 2.0 ** -24 * a).all(), float(ratio)


def test_two_runs_and_the_plain_entry_give_the_same_bits():
    """deterministic (fixed-order cross-wave and slab sums), and tile 0 x 0 is tbn_conv2d_wgrad -- on float data, where the
    summation order shows"""
    for geom, cin, cout, _ in wc.FLOAT_CASES + [(wc.MANY_SLABS[0], 32, 32, None), ((5, 3, 3, 3, 1, 1), 36, 44, None)]:
        dy, x = wc.float_case(geom, cin, cout, seed=78)
        p = Problem(geom, cin, cout, dy, x, True)
        first = p.run()[1]
        assert torch.equal(bits(first), bits(p.run()[1]))
        assert torch.equal(bits(first), bits(p.run(entry="tbn_conv2d_wgrad")[1]))
        q = wc.plan(lib(), geom, cin, cout, (0, 0))
        assert torch.equal(bits(first), bits(p.run((q["mt"], q["nt"]))[1]))


def test_linear_wgrad_is_the_pointwise_conv_entry():
    """tbn_linear_wgrad at (m, k, n) = (70, 36, 44), pitched: the bits of the 1x1 conv entry on the same data, and exact"""
    m, k, n = 70, 36, 44
    geom = (m, 1, 1, 1, 1, 0)
    dy, x, ref = exact_data(geom, k, n)
    fdy, fx = wc.float_case(geom, k, n, seed=79)
    for a, b, want in ((dy, x, ref), (fdy, fx, None)):
        p = Problem(geom, k, n, a, b, True)
        conv = p.run()[1]
        dw = torch.full((p.numel + TAIL,), NAN, device=DEV)
        ws = torch.full((max(lib().tbn_linear_wgrad_workspace_floats(m, k, n), 1),), NAN, device=DEV)
        call("tbn_linear_wgrad", p.dy.view.data_ptr(), p.dy.ld, p.x.view.data_ptr(), p.x.ld, ptr(dw), 0, m, k, n, ptr(ws), st())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw[p.numel:]).all()) and p.dy.unchanged() and p.x.unchanged()
        lin = dw[:p.numel].reshape(n, 1, 1, k).cpu()
        assert torch.equal(bits(lin), bits(conv))
        if want is not None:
            assert torch.equal(lin, want), first_mismatch(lin, want)


def test_refusals_write_nothing():
    geom, cin, cout = (2, 6, 6, 3, 1, 1), 36, 44
    dy, x, _ = exact_data(geom, cin, cout)
    p = Problem(geom, cin, cout, dy, x, True)
    for tile in ((4, 1), (5, 3), (0, 2), (2, 0), (1, 4)):
        p.run(tile, expect_ok=False)
        assert b"conv2d_wgrad_tile: tile %dx%d" % tile in lib().tbn_last_error()
    for attr, ld, needle in (("dy", cout - 4, b"dout_ld"), ("x", cin - 4, b"in_ld"), ("x", cin + 2, b"in_ld")):
        w = getattr(p, attr)
        keep, w.ld = w.ld, ld
        try:
            p.run(expect_ok=False)
        finally:
            w.ld = keep
        assert needle in lib().tbn_last_error()
    _, got = p.run()                     # ... and the same buffers still give the exact result
    assert torch.equal(got, exact_data(geom, cin, cout)[2])
