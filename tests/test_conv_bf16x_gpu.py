"""GPU parity of the split-bf16 3x3 convolution kernels (conv_bf16x.hip: flags 32 = bf16x6, 64 = bf16x3 of tbn_conv_launch;
reference layer: the 3x3 nn.Conv2d forwards of core/models/bn_inception_audio.py:24-401 under model.eval()):

  * bf16x6 at the operator tolerance of tests/test_conv_variants_gpu.py (1e-4 of the tensor's maximum), every tile, epilogue 0
    (+bias, +ReLU, accumulating) and 2, into a channel slice of a wider buffer;
  * bf16x3 inside its derived element-wise bound 1.25 * 2^-16 * (|x| conv |w|) + 4e-7 * (|x| conv |w|);
  * inputs on which the products bf16x3 keeps cancel exactly: bf16x3 returns 0.0, bf16x6 the full product -- proves which
    kernel ran (a library that ignores the flag bits returns the full product for both);
  * refusals of everything the kernel does not cover; determinism.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import call, lib, ptr  # noqa: E402
from tests.bf16x_emu import ACC_REL, CASES, X3_REL, abs_conv, cancel_problem  # noqa: E402
from tests.test_conv_variants_gpu import ACCUM, DEV, DMA, HALO, RELU, SK4, TOL, Problem, g, nchw, nhwc, relerr, st  # noqa: E402

BF16X6, BF16X3 = 32, 64
TILES = [(mt, nt) for mt in (1, 2) for nt in (1, 2, 3, 4)]


def launch_sliced(P, flags, mt, nt, epilogue=0, bias=None, scale=None, shift=None, fill=3.0):
    """one launch into columns [16, 16 + cout) of a buffer 32 columns wider; returns (NCHW result, buffer)"""
    n, h, w, cin, cout = P.geom[:5]
    y = torch.full((n, h, w, cout + 32), fill, device=DEV)
    d = P.desc(False, y.data_ptr() + 16 * 4, cout + 32, epilogue=epilogue, flags=flags, bias=bias, scale=scale, shift=shift)
    call("tbn_conv_launch", C.byref(d), mt, nt, 0, st())
    assert float((y[..., :16] - fill).abs().max()) == 0 and float((y[..., 16 + cout:] - fill).abs().max()) == 0
    return nchw(y[..., 16:16 + cout]), y


@pytest.mark.parametrize("case", CASES)
def test_bf16x6_every_tile_and_epilogue_at_the_operator_tolerance(case):
    n, h, w, cin, cout = case
    P = Problem(n, h, w, cin, cout, 3, 1, 1, seed=61)
    y64 = P.y_ref.detach()
    bias = torch.randn(cout, generator=g(7))
    sc = torch.rand(cout, generator=g(5)) + 0.5
    sh = torch.randn(cout, generator=g(6))
    b4 = bias.double().view(1, -1, 1, 1)
    biasd, scd, shd = bias.to(DEV), sc.to(DEV), sh.to(DEV)
    worst = 0.0
    for mt, nt in TILES:
        tag = (case, mt, nt)
        got, _ = launch_sliced(P, BF16X6, mt, nt)
        e = [relerr(got, y64)]
        got, _ = launch_sliced(P, BF16X6, mt, nt, bias=biasd)
        e.append(relerr(got, y64 + b4))
        got, _ = launch_sliced(P, BF16X6 | RELU, mt, nt, bias=biasd)
        e.append(relerr(got, F.relu(y64 + b4)))
        got, _ = launch_sliced(P, BF16X6 | ACCUM, mt, nt, bias=biasd, fill=3.0)
        e.append(relerr(got, y64 + b4 + 3.0))
        got, _ = launch_sliced(P, BF16X6, mt, nt, epilogue=2, scale=scd, shift=shd)
        e.append(relerr(got, F.relu(y64 * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))))
        worst = max(worst, max(e))
        assert max(e) < TOL, (tag, e)
    print(case, "bf16x6 worst relative error over tiles / epilogues: %.2e" % worst)


@pytest.mark.parametrize("case", CASES)
def test_bf16x3_inside_its_derived_bound(case):
    n, h, w, cin, cout = case
    P = Problem(n, h, w, cin, cout, 3, 1, 1, seed=61)
    y64 = P.y_ref.detach()
    scale = abs_conv(P.x, P.wt)
    bound = (X3_REL + ACC_REL) * scale
    worst = 0.0
    for mt, nt in TILES:
        got, _ = launch_sliced(P, BF16X3, mt, nt)
        err = (got.double().cpu() - y64).abs()
        worst = max(worst, float((err / scale).max()))
        assert bool((err <= bound).all()), (case, mt, nt, float((err / scale).max()))
    print(case, "bf16x3 worst error / (|x| conv |w|): %.2e (bound %.2e)" % (worst, X3_REL + ACC_REL))


def test_bf16x3_drops_the_planes_it_claims_to_drop():
    """the kept products (hi*hi, hi*mid, mid*hi) cancel exactly between even and odd input channels; only lo*hi survives:
    bf16x3 must return exactly 0.0, bf16x6 the full product.  Fails on a library that ignores the flag bits."""
    n, h, w, cin, cout = 2, 9, 11, 64, 96
    x, wt, want = cancel_problem(n, h, w, cin, cout)
    P = Problem(n, h, w, cin, cout, 3, 1, 1, seed=1)
    P.xd = nhwc(x).to(DEV)
    P.wd = wt.permute(0, 2, 3, 1).contiguous().to(DEV)
    assert float(want.abs().min()) > 1e-4
    for mt, nt in TILES:
        y3, _ = launch_sliced(P, BF16X3, mt, nt)
        y6, _ = launch_sliced(P, BF16X6, mt, nt)
        e6 = float(((y6.double().cpu() - want).abs() / want.abs()).max())
        print((mt, nt), "bf16x3 max |y| %.3e, bf16x6 relative error %.2e" % (float(y3.abs().max()), e6))
        assert float(y3.abs().max()) == 0.0, (mt, nt)
        assert e6 < 1e-6, (mt, nt, e6)


def _refused(rc):
    msg = (lib().tbn_last_error() or b"").decode()
    assert rc < 0, rc
    assert "bf16x" in msg, msg


@pytest.mark.parametrize("flag", [BF16X6, BF16X3])
def test_refusals_name_the_flag(flag):
    L = lib()
    P = Problem(2, 9, 11, 32, 64, 3, 1, 1, seed=3)
    n, h, w, cin, cout = P.geom[:5]
    y = torch.zeros(n, h, w, cout, device=DEV)
    dx = torch.zeros(n, h, w, cin, device=DEV)
    # data gradient
    _refused(L.tbn_conv_launch(C.byref(P.desc(True, ptr(dx), cin, flags=flag)), 1, 1, ptr(P.ws), st()))
    # training-statistics epilogue
    part = torch.zeros(8, 2, cout, device=DEV)
    _refused(L.tbn_conv_launch(C.byref(P.desc(False, ptr(y), cout, epilogue=1, flags=flag, stat_partial=part)), 1, 1, 0, st()))
    # both bits, and with the fp32 variant bits
    _refused(L.tbn_conv_launch(C.byref(P.desc(False, ptr(y), cout, flags=BF16X6 | BF16X3)), 1, 1, 0, st()))
    for v in (HALO, DMA, SK4):
        _refused(L.tbn_conv_launch(C.byref(P.desc(False, ptr(y), cout, flags=flag | v)), 1, 1, 0, st()))
    # pair launch
    da, db = P.desc(False, ptr(y), cout, flags=flag), P.desc(False, ptr(y), cout, flags=flag)
    _refused(L.tbn_conv_launch_pair(C.byref(da), C.byref(db), 0, 1, 1, 0, 0, st()))
    # geometries: 1x1, stride 2, width 65
    for geom in ((2, 9, 11, 32, 64, 1, 1, 0), (2, 10, 12, 32, 64, 3, 2, 1), (1, 4, 65, 32, 64, 3, 1, 1)):
        Q = Problem(*geom, seed=4)
        yq = torch.zeros(geom[0], Q.oh, Q.ow, geom[4], device=DEV)
        _refused(L.tbn_conv_launch(C.byref(Q.desc(False, ptr(yq), geom[4], flags=flag)), 1, 1, 0, st()))
        _refused(L.tbn_conv_launch(C.byref(Q.desc(False, ptr(yq), geom[4], flags=flag)), 0, 0, 0, st()))
        torch.cuda.synchronize()
        assert float(yq.abs().max()) == 0.0      # nothing was launched
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0


def test_bf16x6_is_deterministic():
    P = Problem(2, 28, 28, 192, 96, 3, 1, 1, seed=61)
    for mt, nt in ((1, 1), (2, 3), (0, 0)):
        a, _ = launch_sliced(P, BF16X6, mt, nt)
        b, _ = launch_sliced(P, BF16X6, mt, nt)
        assert torch.equal(a, b), (mt, nt)
