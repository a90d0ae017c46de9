"""The arithmetic the split-bf16 convolution kernel is specified to perform, pinned without a GPU: the three-plane split
is exact, and the emulated bf16x6 / bf16x3 convolutions stay inside the bounds the GPU tests assert on the kernel."""
import pytest
import torch
import torch.nn.functional as F

from tests.bf16x_emu import ACC_REL, CASES, X3_REL, abs_conv, cancel_problem, conv_emulated, split

TOL = 1e-4   # tests/test_conv_variants_gpu.py


def test_three_plane_split_is_exact():
    g = torch.Generator().manual_seed(0)
    mant = torch.rand(1000000, generator=g) + 1.0
    expo = torch.randint(-100, 101, (1000000,), generator=g)
    sign = torch.randint(0, 2, (1000000,), generator=g).float() * 2 - 1
    x = torch.ldexp(mant * sign, expo)
    assert x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    hi, mid, lo = split(x)
    assert torch.equal((hi + mid) + lo, x)
    assert torch.equal(hi + (mid + lo), x)
    for p in (hi, mid, lo):     # every plane is a bf16 value
        assert torch.equal(p.bfloat16().float(), p)


@pytest.mark.parametrize("case", CASES)
def test_emulated_convolutions_inside_the_kernel_bounds(case):
    n, h, w, cin, cout = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    y64 = F.conv2d(x.double(), wt.double(), None, padding=1)
    scale = abs_conv(x, wt)
    e6 = (conv_emulated(x, wt, 6).double() - y64).abs()
    e3 = (conv_emulated(x, wt, 3).double() - y64).abs()
    r6, r3 = float(e6.max() / y64.abs().max()), float(e3.max() / y64.abs().max())
    b6, b3 = float((e6 / scale).max()), float((e3 / scale).max())
    print(case, "bf16x6 %.2e (%.2e of |x|*|w|), bf16x3 %.2e (%.2e)" % (r6, b6, r3, b3))
    assert r6 < TOL and r6 < 5e-7              # the issue's table: 1.4e-7 ... 1.7e-7
    assert bool((e3 <= (X3_REL + ACC_REL) * scale).all())
    assert r3 < 1e-5 and b3 < 4e-6             # the table: 4.2e-6 ... 4.8e-6, 8.5e-7 ... 2.3e-6


def test_cancellation_inputs_separate_the_two_modes():
    x, wt, want = cancel_problem(2, 9, 11, 64, 96)
    hi, mid, lo = split(x)
    assert float((hi - 1).abs().max()) == 0 and float((mid - 2.0 ** -9).abs().max()) == 0
    assert torch.equal(lo[:, 0::2], torch.full_like(lo[:, 0::2], 7 * 2.0 ** -20)) and float(lo[:, 1::2].abs().max()) == 0
    assert float(conv_emulated(x, wt, 3).abs().max()) == 0.0
    assert torch.equal(conv_emulated(x, wt, 6).double(), want)
    assert float(want.abs().min()) > 1e-4
