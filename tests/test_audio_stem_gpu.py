"""The separable audio stem (tbn_audio_stem_*: conv1_1x3_s2 | conv1_3x1_s2 of BNInception_Audio, concatenated) at operator
level, through the C-ABI, against float64 F.conv2d.

Exact cases: inputs are integers in [-8, 8], weights and dy integers in [-4, 4].  A conv value is at most 3 * 4 * 8 = 96, its
square 9216; a workgroup's statistics row sums at most 4 rows x 65 pixels of them (2.4e6), a weight-gradient partial at most
260 * 32 -- every fp32 sum stays far below 2^24, so forward, statistics and weight gradient must EQUAL the float64 result.
Sizes: the degenerate maps, odd and even heights and widths, a width that crosses the 64-pixel chunk of a row (ow = 63, 64,
65), heights around the 4-row strip of a workgroup (oh = 3, 4, 5), and (3, 10, 12): oh = 5, so 15 flattened output rows in
four workgroups with both frame boundaries inside a workgroup's strip.
Random floats: 1e-4 relative to the tensor's maximum (TOL of tests/test_kernels_gpu.py), two runs bit-identical."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import call, lib, ptr  # noqa: E402

DEV = "cuda"
TOL = 1e-4
SENTINEL = -777.0
SIZES = [(1, 1, 1), (2, 1, 6), (2, 5, 7), (2, 8, 6), (2, 2, 9), (2, 33, 130), (3, 10, 12), (1, 5, 9), (1, 7, 9), (1, 9, 9),
         (1, 4, 125), (1, 4, 127)]


def st():
    return torch.cuda.current_stream().cuda_stream


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def floats(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def reference(x, w, bias, dy):
    """float64: NHWC conv output without bias, with bias, and the [64][3] weight gradient for dy (NHWC)"""
    w = w.clone().requires_grad_(True)
    ya = F.conv2d(x, w[:32].view(32, 1, 3, 1), None, stride=2, padding=(1, 0))
    yb = F.conv2d(x, w[32:].view(32, 1, 1, 3), None, stride=2, padding=(0, 1))
    y = torch.cat([ya, yb], 1).permute(0, 2, 3, 1)
    (y * dy).sum().backward()
    return y.detach(), (y + bias).detach(), w.grad.detach()


@functools.lru_cache(maxsize=None)
def case(n, h, w, exact):
    oh, ow = out_hw(h, w)
    seed = 1000 * n + 10 * h + w
    if exact:
        x, wt, bias = ints((n, 1, h, w), -8, 8, seed), ints((64, 3), -4, 4, seed + 1), ints((64,), -4, 4, seed + 2)
        dy = ints((n, oh, ow, 64), -4, 4, seed + 3)
    else:
        x, wt, bias = floats((n, 1, h, w), seed), floats((64, 3), seed + 1, 0.6), floats((64,), seed + 2, 0.3)
        dy = floats((n, oh, ow, 64), seed + 3)
    return x, wt, bias, dy, reference(x, wt, bias, dy)


def dev(t):
    return t.float().contiguous().to(DEV)


def run_fwd(x, wt, bias, n, h, w, epilogue, flags=0, ld=64, scale=None, shift=None):
    oh, ow = out_hw(h, w)
    out = torch.full((n, oh, ow, ld), SENTINEL, device=DEV, dtype=torch.float32)
    rows = lib().tbn_audio_stem_stat_rows(n, h, w)
    assert rows >= 1
    partial = torch.full((rows, 2, 64), SENTINEL, device=DEV, dtype=torch.float32) if epilogue == 1 else None
    call("tbn_audio_stem_fwd", ptr(x), ptr(wt), ptr(bias), ptr(out), ld, n, h, w, epilogue, flags, ptr(scale), ptr(shift),
         ptr(partial), st())
    return out, partial


def run_wgrad(dy, x, n, h, w):
    nws = lib().tbn_audio_stem_wgrad_workspace_floats(n, h, w)
    assert nws >= 192 and nws % 192 == 0
    ws = torch.empty(nws, device=DEV, dtype=torch.float32)
    dw = torch.full((64, 3), SENTINEL, device=DEV, dtype=torch.float32)
    call("tbn_audio_stem_wgrad", ptr(dy), dy.shape[3], ptr(x), ptr(dw), n, h, w, ptr(ws), st())
    return dw


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_exact_forward_statistics_and_weight_gradient(size):
    n, h, w = size
    x, wt, bias, dy, (y, yb, dw) = case(n, h, w, True)
    xd, wd, bd = dev(x), dev(wt), dev(bias)
    out, _ = run_fwd(xd, wd, bd, n, h, w, 0)
    assert torch.equal(out.cpu().double(), yb)
    out, _ = run_fwd(xd, wd, None, n, h, w, 0, flags=2)              # no bias, ReLU
    assert torch.equal(out.cpu().double(), y.clamp_min(0))
    raw, partial = run_fwd(xd, wd, bd, n, h, w, 1)                   # the bias is ignored
    assert torch.equal(raw.cpu().double(), y)
    sums = partial.cpu().double().sum(0)
    flat = y.reshape(-1, 64)
    assert torch.equal(sums[0], flat.sum(0)) and torch.equal(sums[1], (flat * flat).sum(0))
    got = run_wgrad(dev(dy), xd, n, h, w)
    assert torch.equal(got.cpu().double(), dw)


def test_pitched_output_leaves_the_other_columns_alone():
    n, h, w = 2, 5, 7
    x, wt, bias, dy, (y, yb, dw) = case(n, h, w, True)
    out, _ = run_fwd(dev(x), dev(wt), dev(bias), n, h, w, 0, ld=96)
    assert torch.equal(out[..., :64].cpu().double(), yb)
    assert bool((out[..., 64:] == SENTINEL).all())
    # the weight gradient reads dy through the same pitch
    oh, ow = out_hw(h, w)
    wide = torch.full((n, oh, ow, 96), 3.0, device=DEV, dtype=torch.float32)
    wide[..., :64] = dev(dy)
    assert torch.equal(run_wgrad(wide, dev(x), n, h, w).cpu().double(), dw)


@pytest.mark.parametrize("size", [(2, 33, 130), (3, 10, 12)], ids=lambda s: "x".join(map(str, s)))
def test_random_floats_within_tolerance_and_reproducible(size):
    n, h, w = size
    x, wt, bias, dy, (y, yb, dw) = case(n, h, w, False)
    xd, wd, bd, dyd = dev(x), dev(wt), dev(bias), dev(dy)
    a, _ = run_fwd(xd, wd, bd, n, h, w, 0)
    b, _ = run_fwd(xd, wd, bd, n, h, w, 0)
    err = relerr(a, yb)
    print("audio stem forward", size, err)
    assert err < TOL, err
    assert torch.equal(a, b)
    scale, shift = floats((64,), 5).abs() + 0.5, floats((64,), 6, 0.3)
    e2, _ = run_fwd(xd, wd, None, n, h, w, 2, scale=dev(scale), shift=dev(shift))
    err = relerr(e2, (y * scale + shift).clamp_min(0))
    print("audio stem epilogue 2", size, err)
    assert err < TOL, err
    raw, partial = run_fwd(xd, wd, None, n, h, w, 1)
    raw2, partial2 = run_fwd(xd, wd, None, n, h, w, 1)
    assert torch.equal(raw, raw2) and torch.equal(partial, partial2)
    flat = y.reshape(-1, 64)
    sums = partial.cpu().double().sum(0)
    assert relerr(sums[0], flat.sum(0)) < TOL and relerr(sums[1], (flat * flat).sum(0)) < TOL
    g1, g2 = run_wgrad(dyd, xd, n, h, w), run_wgrad(dyd, xd, n, h, w)
    err = relerr(g1, dw)
    print("audio stem weight gradient", size, err)
    assert err < TOL, err
    assert torch.equal(g1, g2)


def test_refused_arguments_return_a_status_and_launch_nothing():
    n, h, w = 2, 5, 7
    oh, ow = out_hw(h, w)
    x = torch.ones(n, 1, h, w, device=DEV)
    wt, vec = torch.ones(64, 3, device=DEV), torch.ones(64, device=DEV)
    out = torch.full((n, oh, ow, 96), SENTINEL, device=DEV)
    partial = torch.full((lib().tbn_audio_stem_stat_rows(n, h, w) * 128,), SENTINEL, device=DEV)
    fwd, s = lib().tbn_audio_stem_fwd, st()
    good = [ptr(x), ptr(wt), ptr(vec), ptr(out), 64, n, h, w, 0, 0, ptr(vec), ptr(vec), ptr(partial), s]
    bad = {"null x": {0: 0}, "null weight": {1: 0}, "null out": {3: 0}, "pitch below 64": {4: 60},
           "pitch not a multiple of 4": {4: 66}, "epilogue 3": {8: 3}, "unknown flag": {9: 1}, "n = 0": {5: 0},
           "epilogue 1 without partial": {8: 1, 12: 0}, "epilogue 2 without scale": {8: 2, 10: 0}}
    for what, change in bad.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert fwd(*args) != 0, what
        assert len(lib().tbn_last_error()) > 0, what
    assert lib().tbn_audio_stem_stat_rows(0, h, w) == 0 and lib().tbn_audio_stem_wgrad_workspace_floats(n, 0, w) == 0
    dw = torch.full((64, 3), SENTINEL, device=DEV)
    ws = torch.full((lib().tbn_audio_stem_wgrad_workspace_floats(n, h, w),), SENTINEL, device=DEV)
    wgrad = lib().tbn_audio_stem_wgrad
    goodw = [ptr(out), 96, ptr(x), ptr(dw), n, h, w, ptr(ws), s]
    for what, change in {"null dy": {0: 0}, "null x": {2: 0}, "null dweight": {3: 0}, "null workspace": {7: 0},
                         "pitch below 64": {1: 32}, "pitch not a multiple of 4": {1: 70}, "w = 0": {6: 0}}.items():
        args = list(goodw)
        for i, v in change.items():
            args[i] = v
        assert wgrad(*args) != 0, what
        assert b"audio_stem_wgrad" in lib().tbn_last_error(), what
    torch.cuda.synchronize()
    for t in (out, partial, dw, ws):
        assert bool((t == SENTINEL).all())
