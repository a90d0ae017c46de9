"""Plane-product census of the split-bf16 kernels (conv_bf16x.hip; flags 32 = bf16x6 / 64 = bf16x3 / 128 = pre-split weight
planes of tbn_conv_launch; reference layers: the 1x1 and 3x3 nn.Conv2d forwards of core/models/bn_inception_audio.py:24-401
under model.eval()): WHICH of the nine (plane i of x) * (plane j of w) products each kernel accumulates.

include/tbn_hip.h promises i + j <= 2 for bf16x6 and i + j <= 1 for bf16x3.  On the inputs of tests/bf16x_emu.py
isolate_problem every plane product but (i, j) sums to exactly zero (tests/test_bf16x_census_cpu.py proves that of the
inputs), so per pair, mode and tile:
  * a product the mode keeps: the output is r_o D[i] D[j] (cin / 4) taps within 1e-6 relative (the figure of the
    `drops_the_planes_it_claims_to_drop` tests for their surviving product);
  * a product the mode drops: the output is exactly 0.0.
All three planes of both operands are populated, so a kernel that reads a plane from the wrong place (say the lo plane of a
weight record one plane off) leaks a product that does not cancel.  A lost mid*mid or hi*lo, 2^-18 / 2^-17 relative on
random inputs and inside every other tolerance of the suite, is a missing output here.
Kernels: the 3x3 kernel splitting its weights while staging, the same on weight planes, the pointwise kernel on planes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.bf16x_emu import PAIRS, isolate_problem, kept  # noqa: E402
from tests.test_conv_bf16x_gpu import launch_sliced  # noqa: E402
from tests.test_conv_bf16x_planes_gpu import BF16X3, BF16X6, NP, PLANES, TILES, PlaneProblem  # noqa: E402
from tests.test_conv_variants_gpu import DEV, Problem, nhwc  # noqa: E402

# kernel -> (filter size, flag 128)
KERNELS = {"3x3 staged": (3, 0), "3x3 planes": (3, PLANES), "pointwise planes": (1, PLANES)}
# (n, h, w, cin, cout): a ragged map with two M blocks and a 96-column N remainder for both filter sizes; long K for the
# pointwise kernel; cin = 192 on a 7x7 map (two M blocks at mt = 1, N tiles of every nt ragged against 160 columns) for 3x3
SHAPES = {3: [(2, 9, 11, 64, 96), (3, 7, 7, 192, 160)], 1: [(2, 9, 11, 64, 96), (1, 7, 7, 1056, 64)]}
CASES = [(name, shape) for name, (k, _) in KERNELS.items() for shape in SHAPES[k]]


@pytest.mark.parametrize("kernel,shape", CASES, ids=["%s-%s" % (k.replace(" ", "_"), "x".join(map(str, s))) for k, s in CASES])
def test_each_mode_computes_exactly_the_plane_products_it_claims(kernel, shape):
    k, planes = KERNELS[kernel]
    n, h, w, cin, cout = shape
    P = Problem(n, h, w, cin, cout, k, 1, k // 2, seed=1)
    worst = {BF16X6: (0.0, None), BF16X3: (0.0, None)}
    for i, j in PAIRS:
        x, wt, want = isolate_problem(i, j, n, h, w, cin, cout, k)
        P.xd = nhwc(x).to(DEV)
        P.wd = wt.permute(0, 2, 3, 1).contiguous().to(DEV)
        Q = PlaneProblem(P) if planes else P          # fresh planes of these weights
        wantd = want.to(DEV)
        assert float(want.abs().min()) > 0
        for flag in (BF16X6, BF16X3):
            for mt, nt in TILES:
                tag = (kernel, shape, "x plane %d * w plane %d" % (i, j), "bf16x%d" % NP[flag], (mt, nt))
                got, _ = launch_sliced(Q, flag | planes, mt, nt)
                if kept(i, j, NP[flag]):
                    e = float(((got.double() - wantd).abs() / wantd.abs()).max())
                    if e > worst[flag][0]:
                        worst[flag] = (e, tag[2:])
                    assert e < 1e-6, (tag, e)
                else:
                    assert float(got.abs().max()) == 0.0, (tag, float(got.abs().max()), float(wantd.abs().max()))
    for flag in (BF16X6, BF16X3):
        print("CENSUS %s %s bf16x%d: worst kept-product relative error %.2e%s"
              % (kernel, shape, NP[flag], worst[flag][0], " at %s" % (worst[flag][1],) if worst[flag][1] else ""))
