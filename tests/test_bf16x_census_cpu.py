"""The plane-product census inputs (tests/bf16x_emu.py isolate_problem), pinned without a GPU: for each of the nine
(plane i of x, plane j of w) pairs the three planes still add up to the operands, every OTHER plane product convolves to
exactly 0.0, and the target product is the closed form.  tests/test_conv_bf16x_census_gpu.py assumes exactly this of them
when it asks a kernel for 0.0 where its mode drops (i, j) and for the closed form where it keeps it."""
import pytest
import torch
import torch.nn.functional as F

from tests.bf16x_emu import PAIRS, isolate_problem, kept, split


def _products(x, wt, k, dtype):
    xs, ws = [p.to(dtype) for p in split(x)], [p.to(dtype) for p in split(wt)]
    return {(p, q): F.conv2d(xs[p], ws[q], None, padding=k // 2) for p, q in PAIRS}


@pytest.mark.parametrize("cin", [32, 64, 192, 1056])
@pytest.mark.parametrize("k", [1, 3])
def test_isolate_problem_leaves_exactly_one_plane_product(k, cin):
    n, h, w, cout = 1, 4, 5, 8
    for i, j in PAIRS:
        x, wt, want = isolate_problem(i, j, n, h, w, cin, cout, k)
        assert x.dtype == wt.dtype == torch.float32 and want.dtype == torch.float64
        assert x.shape == (n, cin, h, w) and wt.shape == (cout, cin, k, k) and want.shape == (n, cout, h, w)
        for t in (x, wt):
            hi, mid, lo = split(t)
            assert torch.equal((hi + mid) + lo, t)
            assert all(float(p.abs().min()) > 0 for p in (hi, mid, lo))       # a swapped plane leaks a non-zero product
        assert float(want.abs().min()) > 0
        p32, p64 = _products(x, wt, k, torch.float32), _products(x, wt, k, torch.float64)
        for pq in PAIRS:
            if pq != (i, j):
                assert float(p32[pq].abs().max()) == 0.0 and float(p64[pq].abs().max()) == 0.0, ((i, j), pq)
        assert torch.equal(p64[(i, j)], want), (i, j)
        assert float(((p32[(i, j)].double() - want).abs() / want.abs()).max()) < 1e-6, (i, j)
        # what a kernel's single fp32 accumulator holds after the products its mode keeps, small first or large first
        for nprod in (6, 3):
            order = sorted([pq for pq in PAIRS if kept(pq[0], pq[1], nprod)], key=lambda t: -(t[0] + t[1]))
            for seq in (order, order[::-1]):
                acc = torch.zeros_like(p32[(0, 0)])
                for pq in seq:
                    acc = acc + p32[pq]
                if kept(i, j, nprod):
                    assert float(((acc.double() - want).abs() / want.abs()).max()) < 1e-6, ((i, j), nprod)
                else:
                    assert float(acc.abs().max()) == 0.0, ((i, j), nprod)
