"""The operators of the VGG backbones through the C-ABI and the ops_conv wrappers against torch on the CPU (fp64 where a
tolerance applies, fp32 where the result must be EXACT): the 3x3 first layer from NCHW frames (tbn_conv3_first_*), the 2x2 max
pool (tbn_maxpool2_*), the 7x7 adaptive average pool + flatten (tbn_adaptive_avgpool7_*), conv_bias_act, and the Linear entries
at the classifier's K = 25088.

Bounds (relative to the tensor's maximum, the project's own as stated in tests/test_resnet_gpu.py): one operator forward 1e-4,
operator gradients 1e-3.  The adaptive pool has a derived bound: a window of `a` elements is a chain of a - 1 fp32 additions
and one division, each rounding by at most 2^-24 of a partial sum that never exceeds the largest window sum -- (largest
window's element count) * 2^-23 of the maximum covers it with a factor of two to spare.  Every gradient-parity test of a
composed unit first asserts the conditioning guard of tests/test_resnet_gpu.py (the fp32 CPU twin within a tenth of the bound
of the fp64 twin on the same inputs)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.vgg_twin import rel_err  # noqa: E402

DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL = 1e-4, 1e-3
SENT = -7777.0


def rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def guard(a, b, bound, what):
    err = rel_err(a, b)
    assert err < bound / 10, "conditioning guard: fp32 twin vs fp64 twin on %s: %.3g (bound %.1g / 10)" % (what, err, bound)


def abi():
    from attention_based_tbn_amd._lib import call, lib, ptr, stream_ptr
    return call, lib(), ptr, stream_ptr


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pitched(t_nhwc, ld):
    """an NHWC tensor inside a buffer of pitch ld, sentinel in the spare columns"""
    n, h, w, c = t_nhwc.shape
    buf = torch.full((n, h, w, ld), SENT, device=DEV, dtype=torch.float32)
    buf[..., :c] = t_nhwc.to(DEV)
    return buf


# ---------------------------------------------------------------------------------------------- the first convolution
FIRST_SHAPES = [(1, 1, 1), (2, 5, 7), (2, 32, 32), (1, 9, 130)]       # the last crosses a pixel tile (64) and a row strip (8)


@functools.lru_cache(maxsize=None)
def first_reference(cin, shape):
    n, h, w = shape
    seed = 100 * cin + h
    x = rand((n, cin, h, w), seed).float()
    wt = rand((64, cin, 3, 3), seed + 1, (2.0 / (9 * cin)) ** 0.5).float()
    bias = rand((64,), seed + 2, 0.3).float()
    scale, shift = (0.5 + rand((64,), seed + 3).abs()).float(), rand((64,), seed + 4, 0.3).float()
    dy = rand((n, 64, h, w), seed + 5).float()
    wd = wt.double().requires_grad_(True)
    y = F.conv2d(x.double(), wd, None, 1, 1)
    (y * dy.double()).sum().backward()
    return x, wt, bias, scale, shift, dy, y.detach(), wd.grad.detach()


def first_fwd(x, wk, out_ld, epilogue, flags=0, bias=None, scale=None, shift=None):
    call, L, ptr, stream_ptr = abi()
    n, cin, h, w = x.shape
    out = torch.full((n, h, w, out_ld), SENT, device=DEV, dtype=torch.float32)
    partial = None
    if epilogue == 1:
        rows = L.tbn_conv3_first_stat_rows(n, cin, h, w)
        assert rows == n * ((h + 7) // 8)
        partial = torch.full((rows, 2, 64), SENT, device=DEV, dtype=torch.float32)
    call("tbn_conv3_first_fwd", ptr(x), ptr(wk), ptr(bias), ptr(out), out_ld, n, h, w, cin, 64, epilogue, flags, ptr(scale),
         ptr(shift), ptr(partial), stream_ptr())
    return out, partial


@pytest.mark.parametrize("shape", FIRST_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cin", [1, 3, 10, 16])
def test_first_conv_forward_epilogues_and_weight_gradient(cin, shape):
    call, L, ptr, stream_ptr = abi()
    x, wt, bias, scale, shift, dy, y64, dw64 = first_reference(cin, shape)
    n, h, w = shape
    xd, wk = x.to(DEV), nhwc(wt).to(DEV)                                   # [cout][3][3][cin]
    bd, scd, shd = bias.to(DEV), scale.to(DEV), shift.to(DEV)
    want = {
        "none": y64,
        "bias": y64 + bias.double().view(1, 64, 1, 1),
        "bias_relu": (y64 + bias.double().view(1, 64, 1, 1)).relu(),
        "stats": y64,
        "affine_relu": (y64 * scale.double().view(1, 64, 1, 1) + shift.double().view(1, 64, 1, 1)).relu(),
    }
    for out_ld in (64, 96):
        got = {
            "none": first_fwd(xd, wk, out_ld, 0)[0],
            "bias": first_fwd(xd, wk, out_ld, 0, bias=bd)[0],
            "bias_relu": first_fwd(xd, wk, out_ld, 0, flags=2, bias=bd)[0],
            "affine_relu": first_fwd(xd, wk, out_ld, 2, scale=scd, shift=shd)[0],
        }
        # epilogue 1 ignores a bias: the output is bias-free
        call_out, partial = first_fwd(xd, wk, out_ld, 1, bias=bd)
        got["stats"] = call_out
        for k, out in got.items():
            err = rel_err(out[..., :64].permute(0, 3, 1, 2), want[k])
            print(cin, shape, out_ld, k, err)
            assert err < FWD_TOL, (k, out_ld, err)
            assert bool((out[..., 64:] == SENT).all()), (k, out_ld)          # the spare columns are untouched
        sums = partial.double().sum(0).cpu()                                  # (2, 64)
        assert rel_err(sums[0], y64.sum((0, 2, 3))) < FWD_TOL
        assert rel_err(sums[1], (y64 * y64).sum((0, 2, 3))) < FWD_TOL
        again, partial2 = first_fwd(xd, wk, out_ld, 1)
        assert torch.equal(again, call_out) and torch.equal(partial2, partial)            # bit-identical runs
    # weight gradient, dy unpitched and pitched
    ws_floats = L.tbn_conv3_first_wgrad_workspace_floats(n, cin, h, w)
    assert ws_floats == min(n * ((h + 7) // 8), 1024) * 64 * 9 * cin
    results = []
    for dy_ld in (64, 96, 64):
        dyd = pitched(nhwc(dy), dy_ld)
        ws = torch.empty(ws_floats, device=DEV, dtype=torch.float32)
        dwk = torch.full((64, 3, 3, cin), SENT, device=DEV, dtype=torch.float32)
        call("tbn_conv3_first_wgrad", ptr(dyd), dy_ld, ptr(xd), ptr(dwk), n, h, w, cin, 64, ptr(ws), stream_ptr())
        err = rel_err(dwk.permute(0, 3, 1, 2), dw64)
        print(cin, shape, "wgrad", dy_ld, err)
        assert err < GRAD_TOL, (dy_ld, err)
        results.append(dwk)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])   # bit-identical, whatever the pitch


def test_first_conv_refuses_bad_arguments_without_a_launch():
    _, L, ptr, stream_ptr = abi()
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    wk = torch.zeros(64, 3, 3, 3, device=DEV)
    out = torch.full((1, 8, 8, 64), SENT, device=DEV)
    dwk = torch.full((64, 3, 3, 3), SENT, device=DEV)
    ws = torch.empty(64 * 27 * 4, device=DEV)
    st = stream_ptr()
    ARG, UNSUPPORTED = -1, -3

    def fwd(x_=x, w_=wk, o_=out, ld=64, n=1, h=8, w=8, cin=3, cout=64, epi=0, flags=0, sc=None, sh=None, part=None):
        return L.tbn_conv3_first_fwd(ptr(x_), ptr(w_), 0, ptr(o_), ld, n, h, w, cin, cout, epi, flags, ptr(sc), ptr(sh),
                                     ptr(part), st)

    def wgrad(dy_=out, x_=x, dw_=dwk, ws_=ws, ld=64, n=1, h=8, w=8, cin=3, cout=64):
        return L.tbn_conv3_first_wgrad(ptr(dy_), ld, ptr(x_), ptr(dw_), n, h, w, cin, cout, ptr(ws_), st)

    assert fwd(cin=0) == ARG and fwd(cin=17) == ARG
    assert fwd(cout=32) == UNSUPPORTED and fwd(cout=128) == UNSUPPORTED
    assert fwd(ld=60) == ARG and fwd(ld=66) == ARG
    assert fwd(x_=None) == ARG and fwd(w_=None) == ARG and fwd(o_=None) == ARG
    assert fwd(n=0) == ARG and fwd(h=0) == ARG and fwd(w=-1) == ARG
    assert fwd(epi=3) == ARG and fwd(epi=1) == ARG and fwd(epi=2) == ARG         # no partials / no scale and shift
    assert fwd(flags=1) == ARG and fwd(epi=2, flags=2, sc=wk, sh=wk) == ARG
    assert L.tbn_last_error().decode().startswith("conv3_first_fwd")
    assert wgrad(cin=0) == ARG and wgrad(cin=17) == ARG and wgrad(cout=96) == UNSUPPORTED
    assert wgrad(ld=32) == ARG and wgrad(ld=70) == ARG
    assert wgrad(dy_=None) == ARG and wgrad(x_=None) == ARG and wgrad(dw_=None) == ARG and wgrad(ws_=None) == ARG
    assert L.tbn_last_error().decode().startswith("conv3_first_wgrad")
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((dwk == SENT).all())               # nothing was launched
    assert fwd() == 0 and wgrad() == 0                                           # ... and the good call goes through
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((dwk == 0).all())


# ---------------------------------------------------------------------------------------------- MaxPool2d(2, 2)
POOL_SHAPES = [(1, 2, 2, 4), (2, 6, 8, 64), (1, 7, 5, 32), (1, 4, 4, 132)]


def pool_fwd(xd, in_ld, out_ld, c, want_argmax=True):
    call, _, ptr, stream_ptr = abi()
    n, h, w, _ = xd.shape
    out = torch.full((n, h // 2, w // 2, out_ld), SENT, device=DEV, dtype=torch.float32)
    argmax = torch.full((n, h // 2, w // 2, c), 99, device=DEV, dtype=torch.uint8) if want_argmax else None
    call("tbn_maxpool2_fwd", ptr(xd), in_ld, ptr(out), out_ld, ptr(argmax), n, h, w, c, stream_ptr())
    return out, argmax


def pool_bwd(dout, dout_ld, argmax, shape, din_ld, z=None, z_ld=0, base=None):
    call, _, ptr, stream_ptr = abi()
    n, h, w, c = shape
    din = torch.full((n, h, w, din_ld), SENT, device=DEV, dtype=torch.float32)
    if base is not None:
        din[..., :c] = base
    call("tbn_maxpool2_bwd", ptr(dout), dout_ld, ptr(argmax), ptr(z), z_ld, ptr(din), din_ld, n, h, w, c,
         int(base is not None), stream_ptr())
    return din


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool2_equals_torch_exactly(shape):
    n, h, w, c = shape
    x = rand((n, c, h, w), 7 + h).float().requires_grad_(True)
    ref = F.max_pool2d(x, 2, 2)
    dout = rand(tuple(ref.shape), 8 + h).float()
    ref.backward(dout)
    in_ld, out_ld, din_ld = c + 4, c + 8, c + 12
    xd = pitched(nhwc(x.detach()), in_ld)
    out, argmax = pool_fwd(xd, in_ld, out_ld, c)
    assert torch.equal(out[..., :c].cpu(), nhwc(ref.detach()))
    assert bool((out[..., c:] == SENT).all()) and int(argmax.max()) <= 3
    out2, _ = pool_fwd(xd, in_ld, out_ld, c, want_argmax=False)                     # argmax is optional in the forward
    assert torch.equal(out2, out)
    doutd = pitched(nhwc(dout), out_ld)
    din = pool_bwd(doutd, out_ld, argmax, shape, din_ld)
    assert torch.equal(din[..., :c].cpu(), nhwc(x.grad))                             # dropped rows / columns: zeros
    assert bool((din[..., c:] == SENT).all())
    # accumulate: added to what the buffer holds
    base = rand((n, h, w, c), 9 + h).float().to(DEV)
    acc = pool_bwd(doutd, out_ld, argmax, shape, din_ld, base=base)
    assert torch.equal(acc[..., :c].cpu(), base.cpu() + nhwc(x.grad))
    assert bool((acc[..., c:] == SENT).all())


def test_maxpool2_ties_go_to_the_first_element_of_the_window():
    n, h, w, c = 1, 6, 4, 8
    xd = torch.full((n, h, w, c), 0.5, device=DEV)
    out, argmax = pool_fwd(xd, c, c, c)
    assert bool((out == 0.5).all()) and int(argmax.max()) == 0
    dout = torch.arange(1, n * 3 * 2 * c + 1, device=DEV, dtype=torch.float32).view(n, 3, 2, c)
    din = pool_bwd(dout, c, argmax, (n, h, w, c), c)
    want = torch.zeros(n, h, w, c, device=DEV)
    want[:, 0::2, 0::2] = dout
    assert torch.equal(din, want)
    # the same rule as torch on the CPU
    xc = torch.full((n, c, h, w), 0.5, requires_grad=True)
    F.max_pool2d(xc, 2, 2).backward(dout.cpu().permute(0, 3, 1, 2))
    assert torch.equal(din.cpu(), nhwc(xc.grad))


@pytest.mark.parametrize("shape", [(2, 6, 8, 64), (1, 7, 5, 32)], ids=lambda s: "x".join(map(str, s)))
def test_maxpool2_relu_gate_equals_pool_backward_then_relu_mask(shape):
    call, _, ptr, stream_ptr = abi()
    n, h, w, c = shape
    z = nhwc(rand((n, c, h, w), 21 + h).relu().float()).to(DEV)                      # a post-ReLU map: about half zeros
    z[0, 0, 0] = 0.0                                                                 # a window whose maximum is zero
    z[0, 0, 1] = 0.0
    z[0, 1, 0] = 0.0
    z[0, 1, 1] = 0.0
    out, argmax = pool_fwd(z, c, c, c)
    dout = nhwc(rand((n, c, h // 2, w // 2), 22 + h).float()).to(DEV)
    plain = pool_bwd(dout, c, argmax, shape, c)
    two_pass = torch.empty_like(plain)
    call("tbn_relu_mask_bwd", ptr(plain), ptr(z), 0, ptr(two_pass), plain.numel(), stream_ptr())
    gated = pool_bwd(dout, c, argmax, shape, c, z=z, z_ld=c)
    assert torch.equal(gated, two_pass)
    assert not torch.equal(gated, plain)                                             # the gate did something
    base = nhwc(rand((n, c, h, w), 23 + h).float()).to(DEV)
    assert torch.equal(pool_bwd(dout, c, argmax, shape, c, z=z, z_ld=c, base=base), base + two_pass)


def test_maxpool2_refuses_bad_arguments():
    _, L, ptr, stream_ptr = abi()
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    out = torch.full((1, 2, 2, 8), SENT, device=DEV)
    am = torch.zeros(1, 2, 2, 8, device=DEV, dtype=torch.uint8)
    st = stream_ptr()

    def f(h=4, w=4, c=8, in_ld=8, out_ld=8, x_=x):
        return L.tbn_maxpool2_fwd(ptr(x_), in_ld, ptr(out), out_ld, ptr(am), 1, h, w, c, st)

    def b(h=4, w=4, c=8, ld=8, am_=am, z=None, z_ld=0):
        return L.tbn_maxpool2_bwd(ptr(out), ld, ptr(am_), ptr(z), z_ld, ptr(x), 8, 1, h, w, c, 0, st)

    assert f(h=1) == -1 and f(w=1) == -1 and f(c=6) == -1 and f(in_ld=4) == -1 and f(out_ld=10) == -1 and f(x_=None) == -1
    assert b(h=1) == -1 and b(c=2) == -1 and b(ld=4) == -1 and b(am_=None) == -1 and b(z=x, z_ld=4) == -1
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert f() == 0 and b() == 0


# ---------------------------------------------------------------------------------------------- AdaptiveAvgPool2d((7, 7))
def largest_window(L):
    return max(math.ceil((i + 1) * L / 7) - (i * L) // 7 for i in range(7))


@pytest.mark.parametrize("c", [4, 512])
@pytest.mark.parametrize("hw", [(7, 7), (1, 1), (8, 8), (14, 14), (3, 5), (10, 9)], ids=lambda s: "%dx%d" % s)
def test_adaptive_avgpool7_against_torch(hw, c):
    call, _, ptr, stream_ptr = abi()
    h, w = hw
    n = 2
    g = torch.Generator().manual_seed(31 * h + w + c)
    x = (1.0 + 0.5 * torch.rand((n, c, h, w), generator=g, dtype=torch.float64)).float()     # a post-ReLU map: positive
    dout = rand((n, c * 49), 32 + h).float()
    x64 = x.double().requires_grad_(True)
    ref = torch.flatten(F.adaptive_avg_pool2d(x64, (7, 7)), 1)
    ref.backward(dout.double())
    bound = largest_window(h) * largest_window(w) * 2.0 ** -23
    ld = c + 8
    xd = pitched(nhwc(x), ld)
    out = torch.full((n, c * 49), SENT, device=DEV, dtype=torch.float32)
    call("tbn_adaptive_avgpool7_fwd", ptr(xd), ld, ptr(out), n, h, w, c, stream_ptr())
    err = rel_err(out, ref)
    print(hw, c, "fwd", err, bound)
    assert err <= bound, (err, bound)
    if hw == (7, 7):
        assert torch.equal(out.cpu(), torch.flatten(x, 1))                           # the transposition, bit for bit
    doutd = dout.to(DEV)
    din = torch.full((n, h, w, ld), SENT, device=DEV, dtype=torch.float32)
    call("tbn_adaptive_avgpool7_bwd", ptr(doutd), ptr(din), ld, n, h, w, c, 0, stream_ptr())
    err = rel_err(din[..., :c].permute(0, 3, 1, 2), x64.grad)
    print(hw, c, "bwd", err, bound)
    assert err <= bound, (err, bound)
    assert bool((din[..., c:] == SENT).all())
    # accumulate
    base = nhwc(rand((n, c, h, w), 33 + h).float()).to(DEV)
    acc = torch.full((n, h, w, ld), SENT, device=DEV, dtype=torch.float32)
    acc[..., :c] = base
    call("tbn_adaptive_avgpool7_bwd", ptr(doutd), ptr(acc), ld, n, h, w, c, 1, stream_ptr())
    want = base.double().cpu() + nhwc(x64.grad)
    assert rel_err(acc[..., :c], want) <= bound + 2.0 ** -24                          # one more rounding: the final add
    assert bool((acc[..., c:] == SENT).all())


def test_adaptive_avgpool7_wrapper_and_refusals():
    from attention_based_tbn_amd import ops_conv
    _, L, ptr, stream_ptr = abi()
    x = rand((2, 8, 8, 8), 41).float()                                               # NCHW
    xd = nhwc(x).to(DEV).requires_grad_(True)
    R = rand((2, 8 * 49), 42)
    out = ops_conv.adaptive_avgpool7_flat(xd)
    (out * R.float().to(DEV)).sum().backward()
    x64 = x.double().requires_grad_(True)
    ref = torch.flatten(F.adaptive_avg_pool2d(x64, (7, 7)), 1)
    (ref * R).sum().backward()
    assert rel_err(out, ref) < FWD_TOL and rel_err(xd.grad.permute(0, 3, 1, 2), x64.grad) < GRAD_TOL
    o = torch.empty(2, 8 * 49, device=DEV)
    st = stream_ptr()
    assert L.tbn_adaptive_avgpool7_fwd(ptr(xd), 8, ptr(o), 2, 8, 8, 6, st) == -1      # c not a multiple of 4
    assert L.tbn_adaptive_avgpool7_fwd(ptr(xd), 4, ptr(o), 2, 8, 8, 8, st) == -1      # pitch below c
    assert L.tbn_adaptive_avgpool7_fwd(0, 8, ptr(o), 2, 8, 8, 8, st) == -1
    assert L.tbn_adaptive_avgpool7_bwd(ptr(o), 0, 8, 2, 8, 8, 8, 0, st) == -1
    assert L.tbn_adaptive_avgpool7_bwd(ptr(o), ptr(xd), 8, 2, 0, 8, 8, 0, st) == -1


# ---------------------------------------------------------------------------------------------- conv + bias + ReLU
@functools.lru_cache(maxsize=None)
def conv_bias_reference(pool):
    cin, cout = 64, 128
    x = rand((2, cin, 9, 7), 51).relu()
    w, b = rand((cout, cin, 3, 3), 52, (2.0 / (9 * cin)) ** 0.5), rand((cout,), 53, 0.2)
    R = rand((2, cout, 4, 3) if pool else (2, cout, 9, 7), 54)
    runs = []
    for dtype in (torch.float64, torch.float32):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, w, b)]
        out = F.relu(F.conv2d(leaves[0], leaves[1], leaves[2], 1, 1))
        if pool:
            out = F.max_pool2d(out, 2, 2)
        (out * R.to(dtype)).sum().backward()
        runs.append((out.detach(), [t.grad for t in leaves]))
    return x, w, b, R, runs[0], runs[1]


def run_conv_bias(x, w, b, R, pool, gated=False, freeze_weight=False):
    from attention_based_tbn_amd import ops_conv
    xd = nhwc(x.float()).to(DEV).requires_grad_(True)
    wd = w.float().to(DEV).requires_grad_(not freeze_weight)
    bd = b.float().to(DEV).requires_grad_(True)
    out = ops_conv.conv_bias_act(xd, wd, bd, 1, 1, relu=True, relu_in_pool=gated)
    if pool:
        out = ops_conv.maxpool2(out, relu_gate=gated)
    (out * nhwc(R.float()).to(DEV)).sum().backward()
    return out.detach(), xd.grad, wd.grad, bd.grad


def test_conv_bias_act_output_and_gradients():
    x, w, b, R, (out64, g64), (out32, g32) = conv_bias_reference(False)
    guard(out32, out64, FWD_TOL, "output")
    for name, a, bb in zip(("dx", "dw", "db"), g32, g64):
        guard(a, bb, GRAD_TOL, name)
    out, dx, dw, db = run_conv_bias(x, w, b, R, False)
    assert rel_err(out.permute(0, 3, 1, 2), out64) < FWD_TOL
    errs = (rel_err(dx.permute(0, 3, 1, 2), g64[0]), rel_err(dw, g64[1]), rel_err(db, g64[2]))
    print("conv_bias_act dx, dw, db", errs)
    assert max(errs) < GRAD_TOL, errs
    # a frozen weight: no weight gradient (and no launch for it), the others unchanged
    _, dx2, dw2, db2 = run_conv_bias(x, w, b, R, False, freeze_weight=True)
    assert dw2 is None and torch.equal(dx2, dx) and torch.equal(db2, db)


def test_conv_bias_act_with_the_pool_carrying_its_relu_mask():
    x, w, b, R, (out64, g64), (out32, g32) = conv_bias_reference(True)
    guard(out32, out64, FWD_TOL, "output")
    for name, a, bb in zip(("dx", "dw", "db"), g32, g64):
        guard(a, bb, GRAD_TOL, name)
    plain = run_conv_bias(x, w, b, R, True, gated=False)
    gated = run_conv_bias(x, w, b, R, True, gated=True)
    for a, bb in zip(plain, gated):
        assert torch.equal(a, bb)                                                    # identical, bit for bit
    out, dx, dw, db = gated
    assert rel_err(out.permute(0, 3, 1, 2), out64) < FWD_TOL
    errs = (rel_err(dx.permute(0, 3, 1, 2), g64[0]), rel_err(dw, g64[1]), rel_err(db, g64[2]))
    print("conv_bias_act + maxpool2 dx, dw, db", errs)
    assert max(errs) < GRAD_TOL, errs


# ---------------------------------------------------------------------------------------------- Linear at K = 25088
@functools.lru_cache(maxsize=None)
def linear_reference():
    m, k, n = 4, 25088, 128
    x, w, b = rand((m, k), 61).relu(), rand((n, k), 62, (2.0 / k) ** 0.5), rand((n,), 63, 0.1)
    R = rand((m, n), 64)
    runs = []
    for dtype in (torch.float64, torch.float32):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, w, b)]
        out = F.linear(*leaves)
        (out * R.to(dtype)).sum().backward()
        runs.append((out.detach(), [t.grad for t in leaves]))
    return x, w, b, R, runs[0], runs[1]


def test_linear_entries_at_the_classifiers_width():
    """(m, k, n) = (4, 25088, 128): the K of classifier.0, which the head GEMMs never ran at"""
    from attention_based_tbn_amd import ops
    x, w, b, R, (out64, g64), (out32, g32) = linear_reference()
    for name, a, bb in zip(("dx", "dw", "db"), g32, g64):
        guard(a, bb, GRAD_TOL, name)
    leaves = [t.float().to(DEV).requires_grad_(True) for t in (x, w, b)]
    out = ops.linear(*leaves)
    (out * R.float().to(DEV)).sum().backward()
    err = rel_err(out, out64)
    print("linear fwd", err)
    assert err < FWD_TOL, err
    errs = [rel_err(t.grad, g) for t, g in zip(leaves, g64)]
    print("linear dx, dw, db", errs)
    assert max(errs) < GRAD_TOL, errs
