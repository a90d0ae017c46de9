"""The second output destination of one convolution launch (tbn_conv_desc flag 256: out2 / out2_ld / out2_col_begin / out2_raw
of include/tbn_hip.h -- what the engine's eval forward does on every merged 1x1 group) through EVERY forward kernel of
tbn_conv_launch and every tile each accepts: the generic kernel with 1 and 2 LDS stages, LDS-halo, LDS-DMA, the split-K tile
kernel, the split-bf16 3x3 kernel (weights split while staging and from planes) and the pointwise split-bf16 kernel.
Reference: the fp64 nn.Conv2d forward (core/models/bn_inception_audio.py:24-401) cut at the boundary column.

Per kernel, tile and boundary (32: inside every N tile wider than 32 columns; cout - 32: the last sub-tile alone):
  epilogue 0 with bias, with bias + ReLU, accumulating onto different non-zero fills; epilogue 2 with the second segment
  folded (out2_raw = 0) and bare (out2_raw = 1).
Both destinations are slices of wider buffers with different pitches; the guard columns on both sides of both stay as filled.
Tolerance: 1e-4 of the segment's maximum (TOL of tests/test_conv_variants_gpu.py); bf16x3 on epilogue 0 without ReLU inside
its derived element-wise bound (X3_REL + ACC_REL) * (|x| conv |w|).  Refusals return < 0 and write nothing."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import call, lib, ptr  # noqa: E402
from tests.bf16x_emu import ACC_REL, X3_REL, abs_conv  # noqa: E402
from tests.bf16x_pw_emu import pw_abs_conv  # noqa: E402
from tests.test_conv_bf16x_planes_gpu import BF16X3, BF16X6, OUT2, PLANES, PlaneProblem  # noqa: E402
from tests.test_conv_variants_gpu import ACCUM, DEV, DMA, HALO, RELU, SK4, TOL, Problem, g, nchw, st, tiles_for  # noqa: E402

GEOM = {3: (2, 9, 11, 64, 160, 3, 1, 1), 1: (2, 9, 11, 96, 160, 1, 1, 0)}
# name -> (filter sizes, flags, stages)
KERNELS = {
    "generic-1-stage": ((3, 1), 0, 1),
    "generic-2-stages": ((3, 1), 0, 2),
    "lds-halo": ((3,), HALO, 0),
    "lds-dma": ((3, 1), DMA, 0),
    "split-k-tile": ((3, 1), SK4, 0),
    "bf16x6-3x3-staged": ((3,), BF16X6, 0),
    "bf16x3-3x3-staged": ((3,), BF16X3, 0),
    "bf16x6-3x3-planes": ((3,), BF16X6 | PLANES, 0),
    "bf16x3-3x3-planes": ((3,), BF16X3 | PLANES, 0),
    "bf16x6-pointwise-planes": ((1,), BF16X6 | PLANES, 0),
    "bf16x3-pointwise-planes": ((1,), BF16X3 | PLANES, 0),
}
CASES = [(name, k) for name, (ks, _, _) in KERNELS.items() for k in ks]
FILL0, FILL1, PAD0, PAD1 = 3.0, 5.0, 16, 4

_shared = {}


def problem(k):
    """one Problem per filter size with its device-side fp64 references, shared by every case (never modified)"""
    if k not in _shared:
        P = Problem(*GEOM[k], seed=81)
        cout = GEOM[k][4]
        bias = torch.randn(cout, generator=g(7))
        sc = torch.rand(cout, generator=g(5)) + 0.5
        sh = torch.randn(cout, generator=g(6))
        y64 = P.y_ref.detach().to(DEV)
        b4, sc4, sh4 = (t.double().view(1, -1, 1, 1).to(DEV) for t in (bias, sc, sh))
        _shared[k] = dict(P=P, Q=PlaneProblem(P), y64=y64, yb=y64 + b4, fold=F.relu(y64 * sc4 + sh4),
                          scale=(abs_conv if k == 3 else pw_abs_conv)(P.x, P.wt).to(DEV),
                          bias=bias.to(DEV), sc=sc.to(DEV), sh=sh.to(DEV))
    return _shared[k]


def launch2(S, flags, stages, mt, nt, c1, epilogue, out2_raw=0, bias=None, scale=None, shift=None):
    """one launch with columns [0, c1) into a slice of one buffer and [c1, cout) into a slice of another; returns the two
    NCHW results after checking that the guard columns around both slices kept their fills"""
    n, h, w, cin, cout = S["P"].geom[:5]
    c2 = cout - c1
    y0 = torch.full((n, h, w, c1 + 2 * PAD0), FILL0, device=DEV)
    y1 = torch.full((n, h, w, c2 + 2 * PAD1), FILL1, device=DEV)
    src = S["Q"] if flags & PLANES else S["P"]
    d = src.desc(False, y0.data_ptr() + PAD0 * 4, c1 + 2 * PAD0, epilogue=epilogue, flags=flags | OUT2, stages=stages,
                 bias=bias, scale=scale, shift=shift)
    d.out2, d.out2_ld, d.out2_col_begin, d.out2_raw = y1.data_ptr() + PAD1 * 4, c2 + 2 * PAD1, c1, out2_raw
    call("tbn_conv_launch", C.byref(d), mt, nt, 0, st())
    assert float((y0[..., :PAD0] - FILL0).abs().max()) == 0 and float((y0[..., PAD0 + c1:] - FILL0).abs().max()) == 0
    assert float((y1[..., :PAD1] - FILL1).abs().max()) == 0 and float((y1[..., PAD1 + c2:] - FILL1).abs().max()) == 0
    return nchw(y0[..., PAD0:PAD0 + c1]), nchw(y1[..., PAD1:PAD1 + c2])


def seg_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name,k", CASES, ids=["%s-%dx%d" % (nm, k, k) for nm, k in CASES])
def test_second_segment_every_kernel_tile_epilogue_and_boundary(name, k):
    _, flags, stages = KERNELS[name]
    S = problem(k)
    cout = GEOM[k][4]
    x3 = bool(flags & BF16X3)
    bound = (X3_REL + ACC_REL) * S["scale"]
    worst = 0.0
    for c1 in (32, cout - 32):
        for mt, nt in tiles_for(flags):
            tag = (name, k, "boundary %d" % c1, (mt, nt))
            runs = [
                ("epilogue 0 + bias", dict(epilogue=0, bias=S["bias"]), 0, (S["yb"], S["yb"]), True),
                ("epilogue 0 + bias + ReLU", dict(epilogue=0, bias=S["bias"]), RELU, (F.relu(S["yb"]), F.relu(S["yb"])), False),
                ("epilogue 0 accumulating", dict(epilogue=0, bias=S["bias"]), ACCUM, (S["yb"] + FILL0, S["yb"] + FILL1), True),
                ("epilogue 2, out2 folded", dict(epilogue=2, scale=S["sc"], shift=S["sh"], out2_raw=0), 0, (S["fold"], S["fold"]), False),
                ("epilogue 2, out2 raw", dict(epilogue=2, scale=S["sc"], shift=S["sh"], out2_raw=1), 0, (S["fold"], S["y64"]), False),
            ]
            for what, kw, extra, (want0, want1), linear in runs:
                a, b = launch2(S, flags | extra, stages, mt, nt, c1, **kw)
                w0, w1 = want0[:, :c1], want1[:, c1:]
                if x3 and linear:
                    e0 = float(((a.double() - w0).abs() / S["scale"][:, :c1]).max())
                    e1 = float(((b.double() - w1).abs() / S["scale"][:, c1:]).max())
                    assert bool(((a.double() - w0).abs() <= bound[:, :c1]).all()), (tag, what, e0)
                    assert bool(((b.double() - w1).abs() <= bound[:, c1:]).all()), (tag, what, e1)
                else:
                    e0, e1 = seg_err(a, w0), seg_err(b, w1)
                    worst = max(worst, e0, e1)
                    assert e0 < TOL and e1 < TOL, (tag, what, e0, e1)
                if what.endswith("raw"):
                    assert float(b.min()) < 0 and float(a.min()) >= 0       # bare accumulator beside a folded first segment
    print("OUT2 %s %dx%d: worst segment error over tiles / boundaries / epilogues %.2e" % (name, k, k, worst))


@pytest.mark.parametrize("k", [3, 1])
def test_second_segment_refusals_write_nothing(k):
    L = lib()
    S = problem(k)
    P = S["P"]
    n, h, w, cin, cout = P.geom[:5]
    y0 = torch.full((n, h, w, cout), FILL0, device=DEV)
    y1 = torch.full((n, h, w, cout), FILL1, device=DEV)
    dx = torch.full((n, h, w, cin), FILL0, device=DEV)
    part = torch.full((8, 2, cout), FILL1, device=DEV)

    def desc(dgrad=False, out2=ptr(y1), col=32, **kw):
        d = P.desc(dgrad, ptr(dx) if dgrad else ptr(y0), cin if dgrad else cout, flags=OUT2, **kw)
        d.out2, d.out2_ld, d.out2_col_begin, d.out2_raw = out2, cout, col, 0
        return d

    def refused(d, ws=0):
        rc = L.tbn_conv_launch(C.byref(d), 1, 1, ws, st())
        msg = (L.tbn_last_error() or b"").decode()
        assert rc < 0, rc
        return msg

    assert "second output segment" in refused(desc(dgrad=True), ptr(P.ws))         # a data gradient
    assert "second output segment" in refused(desc(epilogue=1, stat_partial=part))  # the training-statistics epilogue
    assert "second output segment" in refused(desc(out2=0))                         # out2 = NULL
    for col in (0, cout, cout + 32, -32):
        assert "second output segment" in refused(desc(col=col)), col
    assert "multiple of 32" in refused(desc(col=48))
    torch.cuda.synchronize()
    assert float((y0 - FILL0).abs().max()) == 0 and float((dx - FILL0).abs().max()) == 0
    assert float((y1 - FILL1).abs().max()) == 0 and float((part - FILL1).abs().max()) == 0
