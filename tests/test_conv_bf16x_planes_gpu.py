"""GPU parity of the split-bf16 kernels on PRE-SPLIT weight planes (conv_bf16x.hip; conv flag 128 beside 32 = bf16x6 / 64 =
bf16x3 of tbn_conv_launch, tbn_conv_split_weights; reference layers: the 1x1 and 3x3 nn.Conv2d forwards of
core/models/bn_inception_audio.py:24-401 under model.eval()):

  * the split kernel writes exactly the planes of tests/bf16x_emu.py split(), both plane counts, 1x1 and 3x3 weights;
  * 3x3 with flag 128 is bit-identical to the same launch without it, every tile, both modes, all of bf16x_emu.CASES;
  * the pointwise 1x1 kernel: bf16x6 at the operator tolerance (1e-4 of the tensor's maximum) against fp64 for every tile,
    epilogue 0 (+bias, +ReLU, accumulating) and 2, two destinations with a raw second segment; bf16x3 inside its derived
    element-wise bound; the cancellation inputs (bf16x3 exactly 0.0, bf16x6 the full product); determinism;
  * every refusal names bf16x and writes nothing.
These fail on a library without flag 128.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import call, lib, ptr  # noqa: E402
from tests.bf16x_emu import ACC_REL, CASES, X3_REL  # noqa: E402
from tests.bf16x_pw_emu import PW_CASES, plane_records, pw_abs_conv, pw_cancel_problem  # noqa: E402
from tests.test_conv_bf16x_gpu import launch_sliced  # noqa: E402
from tests.test_conv_variants_gpu import ACCUM, DEV, DMA, HALO, RELU, SK4, TOL, Problem, g, nchw, nhwc, relerr, st  # noqa: E402

BF16X6, BF16X3, PLANES, OUT2 = 32, 64, 128, 256     # 256: the descriptor's out2* fields are set
NP = {BF16X6: 6, BF16X3: 3}
TILES = [(mt, nt) for mt in (1, 2) for nt in (1, 2, 3, 4)]


def split_on_gpu(wd, cout, k, cin, flag):
    """weight planes of the OHWI device tensor `wd` (uint8 device tensor)"""
    nbytes = lib().tbn_conv_weight_planes_bytes(cout, k, cin, NP[flag])
    assert nbytes == cout * k * k * cin * (6 if flag == BF16X6 else 4)
    planes = torch.full((nbytes,), 0xa5, dtype=torch.uint8, device=DEV)
    call("tbn_conv_split_weights", ptr(wd), cout, k, cin, NP[flag], ptr(planes), st())
    return planes


class PlaneProblem:
    """a Problem whose desc() points `weight` at pre-split planes when flag 128 is set"""

    def __init__(self, P):
        self.P, self.geom = P, P.geom
        self._planes = {}

    def planes(self, flag):
        if flag not in self._planes:
            n, h, w, cin, cout, k = self.geom[:6]
            self._planes[flag] = split_on_gpu(self.P.wd, cout, k, cin, flag)
        return self._planes[flag]

    def desc(self, dgrad, out, out_ld, flags=0, **kw):
        d = self.P.desc(dgrad, out, out_ld, flags=flags, **kw)
        if flags & PLANES and flags & (BF16X6 | BF16X3):
            d.weight = ptr(self.planes(BF16X6 if flags & BF16X6 else BF16X3))
        return d


@pytest.mark.parametrize("flag", [BF16X6, BF16X3])
@pytest.mark.parametrize("shape", [(96, 3, 64), (160, 1, 32), (832, 1, 1056), (40, 3, 192)])
def test_split_kernel_writes_the_exact_planes(flag, shape):
    cout, k, cin = shape
    w = torch.randn(cout, k, k, cin, generator=g(11)) * torch.logspace(-6, 3, cin).view(1, 1, 1, -1)
    planes = split_on_gpu(w.to(DEV), cout, k, cin, flag)
    nplanes = 3 if flag == BF16X6 else 2
    got = planes.cpu().view(torch.int16).view(-1, nplanes, 32)
    want = plane_records(w, nplanes)
    assert got.shape == want.shape
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", CASES)
def test_3x3_from_planes_is_bit_identical_to_splitting_while_staging(case):
    n, h, w, cin, cout = case
    Q = PlaneProblem(Problem(n, h, w, cin, cout, 3, 1, 1, seed=61))
    sc = (torch.rand(cout, generator=g(5)) + 0.5).to(DEV)
    sh = torch.randn(cout, generator=g(6)).to(DEV)
    for flag in (BF16X6, BF16X3):
        for mt, nt in TILES:
            a, _ = launch_sliced(Q.P, flag, mt, nt)
            b, _ = launch_sliced(Q, flag | PLANES, mt, nt)
            assert torch.equal(a, b), (case, flag, mt, nt)
        a, _ = launch_sliced(Q.P, flag, 2, 2, epilogue=2, scale=sc, shift=sh)
        b, _ = launch_sliced(Q, flag | PLANES, 2, 2, epilogue=2, scale=sc, shift=sh)
        assert torch.equal(a, b), (case, flag, "epilogue 2")


@pytest.mark.parametrize("case", PW_CASES)
def test_pointwise_bf16x6_every_tile_and_epilogue_at_the_operator_tolerance(case):
    n, h, w, cin, cout = case
    Q = PlaneProblem(Problem(n, h, w, cin, cout, 1, 1, 0, seed=61))
    y64 = Q.P.y_ref.detach()
    bias = torch.randn(cout, generator=g(7))
    sc = torch.rand(cout, generator=g(5)) + 0.5
    sh = torch.randn(cout, generator=g(6))
    b4 = bias.double().view(1, -1, 1, 1)
    biasd, scd, shd = bias.to(DEV), sc.to(DEV), sh.to(DEV)
    f = BF16X6 | PLANES
    worst = 0.0
    for mt, nt in TILES + [(0, 0)]:
        got, _ = launch_sliced(Q, f, mt, nt)
        e = [relerr(got, y64)]
        got, _ = launch_sliced(Q, f, mt, nt, bias=biasd)
        e.append(relerr(got, y64 + b4))
        got, _ = launch_sliced(Q, f | RELU, mt, nt, bias=biasd)
        e.append(relerr(got, F.relu(y64 + b4)))
        got, _ = launch_sliced(Q, f | ACCUM, mt, nt, bias=biasd, fill=3.0)
        e.append(relerr(got, y64 + b4 + 3.0))
        got, _ = launch_sliced(Q, f, mt, nt, epilogue=2, scale=scd, shift=shd)
        e.append(relerr(got, F.relu(y64 * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))))
        worst = max(worst, max(e))
        print(case, (mt, nt), "bf16x6 pointwise relative errors", ["%.2e" % v for v in e])
        assert max(e) < TOL, (case, mt, nt, e)
    print(case, "bf16x6 pointwise worst relative error over tiles / epilogues: %.2e" % worst)


@pytest.mark.parametrize("case", [c for c in PW_CASES if c[4] >= 64])
def test_pointwise_bf16x6_two_segments_with_a_raw_second_segment(case, flag=BF16X6):
    """what the engine's merged 1x1 groups do: columns [0, c1) folded (scale / shift / ReLU) into a slice of one buffer,
    columns [c1, cout) as the bare accumulator into another (the pool_proj part ahead of its average pool)"""
    n, h, w, cin, cout = case
    Q = PlaneProblem(Problem(n, h, w, cin, cout, 1, 1, 0, seed=61))
    y64 = Q.P.y_ref.detach()
    c1 = (cout // 64) * 32
    sc = torch.rand(cout, generator=g(5)) + 0.5
    sh = torch.randn(cout, generator=g(6))
    want0 = F.relu(y64 * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))[:, :c1]
    want1 = y64[:, c1:]
    tol = TOL
    for mt, nt in TILES:
        y0 = torch.full((n, h, w, c1 + 32), 3.0, device=DEV)
        y1 = torch.full((n, h, w, cout - c1 + 8), 5.0, device=DEV)
        d = Q.desc(False, y0.data_ptr() + 16 * 4, c1 + 32, epilogue=2, flags=flag | PLANES | OUT2, scale=sc.to(DEV), shift=sh.to(DEV))
        d.out2, d.out2_ld, d.out2_col_begin, d.out2_raw = y1.data_ptr() + 4 * 4, cout - c1 + 8, c1, 1
        call("tbn_conv_launch", C.byref(d), mt, nt, 0, st())
        assert float((y0[..., :16] - 3).abs().max()) == 0 and float((y0[..., 16 + c1:] - 3).abs().max()) == 0
        assert float((y1[..., :4] - 5).abs().max()) == 0 and float((y1[..., 4 + cout - c1:] - 5).abs().max()) == 0
        e0 = relerr(nchw(y0[..., 16:16 + c1]), want0)
        e1 = relerr(nchw(y1[..., 4:4 + cout - c1]), want1)
        print(case, flag, (mt, nt), "segment errors %.2e %.2e" % (e0, e1))
        assert e0 < tol and e1 < tol, (case, flag, mt, nt, e0, e1)
        assert float(nchw(y1[..., 4:4 + cout - c1]).min()) < 0      # raw: no ReLU


@pytest.mark.parametrize("case", PW_CASES)
def test_pointwise_bf16x3_inside_its_derived_bound(case):
    n, h, w, cin, cout = case
    Q = PlaneProblem(Problem(n, h, w, cin, cout, 1, 1, 0, seed=61))
    y64 = Q.P.y_ref.detach()
    scale = pw_abs_conv(Q.P.x, Q.P.wt)
    bound = (X3_REL + ACC_REL) * scale
    worst = 0.0
    for mt, nt in TILES:
        got, _ = launch_sliced(Q, BF16X3 | PLANES, mt, nt)
        err = (got.double().cpu() - y64).abs()
        worst = max(worst, float((err / scale).max()))
        assert bool((err <= bound).all()), (case, mt, nt, float((err / scale).max()))
    print(case, "bf16x3 pointwise worst error / (|x| conv |w|): %.2e (bound %.2e)" % (worst, X3_REL + ACC_REL))


def test_pointwise_bf16x3_drops_the_planes_it_claims_to_drop():
    n, h, w, cin, cout = 2, 9, 11, 64, 96
    x, wt, want = pw_cancel_problem(n, h, w, cin, cout)
    P = Problem(n, h, w, cin, cout, 1, 1, 0, seed=1)
    P.xd = nhwc(x).to(DEV)
    P.wd = wt.permute(0, 2, 3, 1).contiguous().to(DEV)
    Q = PlaneProblem(P)
    assert float(want.abs().min()) > 1e-5    # a product far from zero (one tap: 1 / 9 of the 3x3 problem's)
    for mt, nt in TILES:
        y3, _ = launch_sliced(Q, BF16X3 | PLANES, mt, nt)
        y6, _ = launch_sliced(Q, BF16X6 | PLANES, mt, nt)
        e6 = float(((y6.double().cpu() - want).abs() / want.abs()).max())
        print((mt, nt), "bf16x3 max |y| %.3e, bf16x6 relative error %.2e" % (float(y3.abs().max()), e6))
        assert float(y3.abs().max()) == 0.0, (mt, nt)
        assert e6 < 1e-6, (mt, nt, e6)


def test_planes_launches_are_deterministic():
    for geom in ((2, 14, 14, 576, 512, 1, 1, 0), (2, 28, 28, 192, 96, 3, 1, 1)):
        Q = PlaneProblem(Problem(*geom, seed=61))
        for mt, nt in ((1, 1), (2, 3), (0, 0)):
            a, _ = launch_sliced(Q, BF16X6 | PLANES, mt, nt)
            b, _ = launch_sliced(Q, BF16X6 | PLANES, mt, nt)
            assert torch.equal(a, b), (geom, mt, nt)


def _refused(rc):
    msg = (lib().tbn_last_error() or b"").decode()
    assert rc < 0, rc
    assert "bf16x" in msg, msg


@pytest.mark.parametrize("flag", [BF16X6, BF16X3])
def test_refusals_name_the_flag(flag):
    L = lib()
    Q = PlaneProblem(Problem(2, 9, 11, 32, 64, 1, 1, 0, seed=3))
    n, h, w, cin, cout = Q.geom[:5]
    y = torch.zeros(n, h, w, cout, device=DEV)
    dx = torch.zeros(n, h, w, cin, device=DEV)
    f = flag | PLANES
    # 128 alone (on fp32 weights and on planes)
    _refused(L.tbn_conv_launch(C.byref(Q.P.desc(False, ptr(y), cout, flags=PLANES)), 1, 1, 0, st()))
    _refused(L.tbn_conv_launch(C.byref(Q.P.desc(False, ptr(y), cout, flags=PLANES | RELU)), 0, 0, 0, st()))
    # data gradient
    _refused(L.tbn_conv_launch(C.byref(Q.desc(True, ptr(dx), cin, flags=f)), 1, 1, ptr(Q.P.ws), st()))
    # training-statistics epilogue
    part = torch.zeros(8, 2, cout, device=DEV)
    _refused(L.tbn_conv_launch(C.byref(Q.desc(False, ptr(y), cout, epilogue=1, flags=f, stat_partial=part)), 1, 1, 0, st()))
    # both math bits, and with the fp32 variant bits
    _refused(L.tbn_conv_launch(C.byref(Q.desc(False, ptr(y), cout, flags=BF16X6 | BF16X3 | PLANES)), 1, 1, 0, st()))
    for v in (HALO, DMA, SK4):
        _refused(L.tbn_conv_launch(C.byref(Q.desc(False, ptr(y), cout, flags=f | v)), 1, 1, 0, st()))
    # pair launch
    da, db = Q.desc(False, ptr(y), cout, flags=f), Q.desc(False, ptr(y), cout, flags=f)
    _refused(L.tbn_conv_launch_pair(C.byref(da), C.byref(db), 1, 1, 1, 0, 0, st()))
    # unsupported tile
    _refused(L.tbn_conv_launch(C.byref(Q.desc(False, ptr(y), cout, flags=f)), 3, 1, 0, st()))
    # geometries: stride-2 1x1 and 3x3, 1x1 with pad 1, 3x3 on a map 65 wide, cin not a multiple of 32.  `weight` stays
    # the fp32 tensor: a refused launch reads nothing
    for geom in ((2, 10, 12, 32, 64, 1, 2, 0), (2, 10, 12, 32, 64, 3, 2, 1), (2, 9, 11, 32, 64, 1, 1, 1),
                 (1, 4, 65, 32, 64, 3, 1, 1), (2, 9, 11, 48, 64, 1, 1, 0), (2, 9, 11, 16, 64, 3, 1, 1)):
        G = Problem(*geom, seed=4)
        yq = torch.zeros(geom[0], G.oh, G.ow, geom[4], device=DEV)
        _refused(L.tbn_conv_launch(C.byref(G.desc(False, ptr(yq), geom[4], flags=f)), 1, 1, 0, st()))
        _refused(L.tbn_conv_launch(C.byref(G.desc(False, ptr(yq), geom[4], flags=f)), 0, 0, 0, st()))
        torch.cuda.synchronize()
        assert float(yq.abs().max()) == 0.0      # nothing was launched
    # the split itself refuses what the kernels could not read
    pl = torch.zeros(64 * 48 * 6, dtype=torch.uint8, device=DEV)
    wq = torch.zeros(64, 1, 1, 48, device=DEV)
    _refused(L.tbn_conv_split_weights(ptr(wq), 64, 1, 48, NP[flag], ptr(pl), st()))
    _refused(L.tbn_conv_split_weights(ptr(wq), 64, 1, 32, 4, ptr(pl), st()))
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0 and int(pl.max()) == 0


def test_flags_32_and_64_alone_still_refuse_a_pointwise_layer():
    """without 128 nothing changes: the 1x1 geometry is refused, not routed to the new kernel"""
    P = Problem(2, 9, 11, 32, 64, 1, 1, 0, seed=3)
    y = torch.zeros(2, 9, 11, 64, device=DEV)
    for flag in (BF16X6, BF16X3):
        _refused(lib().tbn_conv_launch(C.byref(P.desc(False, ptr(y), 64, flags=flag)), 1, 1, 0, st()))
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0
