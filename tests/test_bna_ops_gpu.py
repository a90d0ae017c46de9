"""The ops_conv additions BNInception_Audio is composed from, each against a float64 torch statement of the same op:
audio_stem_bn_pool, conv_bn_act(bias=), maxpool3 / avgpool3, freq_mean.

Bounds (relative to the tensor's maximum): forward 1e-4 (TOL of tests/test_kernels_gpu.py), gradients 1e-3 (a node chains
2-4 operators), as tests/test_resnet_gpu.py."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.resnet_twin import rel_err  # noqa: E402

DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL = 1e-4, 1e-3


def rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def nhwc(t):
    return t.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def stem_modules(seed, dtype):
    """conv1_1x3_s2, its BatchNorm, conv1_3x1_s2, its BatchNorm with every tensor away from its initial value"""
    mods = [nn.Conv2d(1, 32, (3, 1), stride=2, padding=(1, 0)), nn.BatchNorm2d(32),
            nn.Conv2d(1, 32, (1, 3), stride=2, padding=(0, 1)), nn.BatchNorm2d(32)]
    with torch.no_grad():
        for i, m in enumerate(mods):
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(rand(m.weight.shape, seed + 10 * i, 0.6))
                m.bias.copy_(rand((32,), seed + 10 * i + 1, 0.3))
            else:
                m.weight.copy_(0.5 + rand((32,), seed + 10 * i, 1.0).abs())
                m.bias.copy_(rand((32,), seed + 10 * i + 1, 0.2))
                m.running_mean.copy_(rand((32,), seed + 10 * i + 2, 0.2))
                m.running_var.copy_(0.5 + rand((32,), seed + 10 * i + 3).abs())
    return [m.to(dtype) for m in mods]


def stem_reference(mods, x):
    ca, ba, cb, bb = mods
    return F.max_pool2d(torch.cat([F.relu(ba(ca(x))), F.relu(bb(cb(x)))], 1), 3, 2, ceil_mode=True)


@pytest.mark.parametrize("shape", [(2, 1, 32, 40), (3, 1, 37, 51)], ids=lambda s: "x".join(map(str, s)))
def test_audio_stem_bn_pool(shape):
    from attention_based_tbn_amd import ops_conv
    from attention_based_tbn_amd._lib import TbnHipError
    seed = shape[2]
    x = rand(shape, seed)
    ref = stem_modules(seed, torch.float64)
    for m in ref:
        m.train()
    want = stem_reference(ref, x)
    R = rand(tuple(want.shape), seed + 1)
    (want * R).sum().backward()
    got_m = [m.to(DEV) for m in stem_modules(seed, torch.float32)]
    xd = x.float().to(DEV)
    out = ops_conv.audio_stem_bn_pool(xd, *got_m, training=True)
    assert tuple(out.shape) == (shape[0],) + tuple(want.shape[2:]) + (64,)
    (out * nhwc(R)).sum().backward()
    err = rel_err(out.permute(0, 3, 1, 2), want)
    print("audio_stem_bn_pool", shape, "pooled", err)
    assert err < FWD_TOL, err
    for i, (g, r) in enumerate(zip(got_m, ref)):
        err = rel_err(g.weight.grad, r.weight.grad)
        print("audio_stem_bn_pool", shape, "module", i, "weight gradient", err)
        assert g.weight.grad.shape == r.weight.shape and err < GRAD_TOL, (i, err)
        if isinstance(g, nn.Conv2d):
            # a constant in front of a batch-statistics BatchNorm: exactly zero, (rounding noise in the float64 statement)
            assert bool((g.bias.grad == 0).all()) and float(r.bias.grad.abs().max()) < 1e-9, i
        else:
            err = rel_err(g.bias.grad, r.bias.grad)
            assert err < GRAD_TOL, (i, err)
            for stat in ("running_mean", "running_var"):
                err = rel_err(getattr(g, stat), getattr(r, stat))
                print("audio_stem_bn_pool", shape, "module", i, stat, err)
                assert err < FWD_TOL, (i, stat, err)
    # eval: the running statistics just written, the conv bias folded into the shift
    for m in ref:
        m.eval()
    with torch.no_grad():
        want_e = stem_reference(ref, x)
        got_e = ops_conv.audio_stem_bn_pool(xd, *got_m, training=False)
    err = rel_err(got_e.permute(0, 3, 1, 2), want_e)
    print("audio_stem_bn_pool", shape, "eval", err)
    assert err < FWD_TOL, err
    with pytest.raises(TbnHipError, match="eval-mode backbone"):
        ops_conv.audio_stem_bn_pool(xd, *got_m, training=False).sum().backward()
    with pytest.raises(TbnHipError, match="gradient with respect to the input frames"):
        ops_conv.audio_stem_bn_pool(xd.clone().requires_grad_(True), *got_m, training=True).sum().backward()


def test_conv_bn_act_with_a_conv_bias():
    from attention_based_tbn_amd import ops_conv
    from attention_based_tbn_amd._lib import TbnHipError
    cin, cout = 64, 96
    x, w = rand((2, cin, 9, 7), 1).relu(), rand((cout, cin, 3, 3), 2, (2.0 / (9 * cin)) ** 0.5)
    bias, gamma, beta = rand((cout,), 3, 0.3), 0.5 + rand((cout,), 5).abs(), rand((cout,), 6, 0.2)
    R = rand((2, cout, 9, 7), 4)
    xd, Rd = nhwc(x), nhwc(R)

    def run(with_bias):
        p = [t.float().to(DEV).requires_grad_(True) for t in (w, gamma, beta, bias)]
        rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
        out = ops_conv.conv_bn_act(xd, p[0], p[1], p[2], rm, rv, 1, 1, relu=True, training=True,
                                   bias=p[3] if with_bias else None)
        (out * Rd).sum().backward()
        return out.detach(), rm, rv, p

    out_b, rm_b, rv_b, p_b = run(True)
    out_0, rm_0, rv_0, p_0 = run(False)
    assert torch.equal(out_b, out_0) and torch.equal(rv_b, rv_0)
    for i in range(3):
        assert torch.equal(p_b[i].grad, p_0[i].grad), i
    assert p_0[3].grad is None and p_b[3].grad.shape == (cout,) and bool((p_b[3].grad == 0).all())
    # from zero: running_mean = 0.1 * (mean + bias) against 0.1 * mean, a handful of fp32 roundings of O(1) numbers
    err = rel_err(rm_b - rm_0, 0.1 * bias)
    print("conv_bn_act running-mean difference", err)
    assert err < 1e-5, err
    y = F.conv2d(x, w, bias, 1, 1)
    assert rel_err(rm_b, 0.1 * y.mean((0, 2, 3))) < FWD_TOL
    ref = F.relu(F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5))
    assert rel_err(out_b.permute(0, 3, 1, 2), ref) < FWD_TOL
    # eval: shift = beta + (bias - running_mean) * scale; the fold follows the bias when it changes in place
    rm, rv = rand((cout,), 7, 0.2), 0.5 + rand((cout,), 8).abs()
    state = ops_conv.BnState(1, 1, None, None)
    pb, rmd, rvd = p_b[3].detach().clone(), rm.float().to(DEV), rv.float().to(DEV)
    for k in range(2):
        want = F.relu(F.batch_norm(F.conv2d(x, w, pb.double().cpu(), 1, 1), rm, rv, gamma, beta, False, 0.1, 1e-5))
        with torch.no_grad():
            got = ops_conv.conv_bn_act(xd, p_b[0], p_b[1], p_b[2], rmd, rvd, 1, 1, relu=True, training=False, state=state,
                                       bias=pb)
        err = rel_err(got.permute(0, 3, 1, 2), want)
        print("conv_bn_act eval with bias", k, err)
        assert err < FWD_TOL, err
        pb.add_(0.5)
    # the join of a residual block does not take a bias
    res = nhwc(rand((2, cout, 9, 7), 9))
    with pytest.raises(TbnHipError, match="bias"):
        ops_conv.conv_bn_act(xd, p_b[0], p_b[1], p_b[2], None, None, 1, 1, residual=res, training=True, bias=p_b[3])


@pytest.mark.parametrize("stride,pad,ceil", [(2, 0, True), (1, 1, False)])
def test_maxpool3_and_avgpool3(stride, pad, ceil):
    from attention_based_tbn_amd import ops_conv
    x = rand((2, 32, 9, 7), 21).float().double()                      # fp32-exact values: the maximum is exact
    leaf = x.clone().requires_grad_(True)
    want = F.max_pool2d(leaf, 3, stride, pad, ceil_mode=ceil)
    R = rand(tuple(want.shape), 22)
    (want * R).sum().backward()
    xd = nhwc(x).requires_grad_(True)
    got = ops_conv.maxpool3(xd, stride, pad, ceil)
    (got * nhwc(R)).sum().backward()
    assert torch.equal(got.permute(0, 3, 1, 2).cpu().double(), want.detach())
    assert rel_err(xd.grad.permute(0, 3, 1, 2), leaf.grad) < 1e-5            # fp32 sums of at most 9 values: 9 * 2^-23
    if stride == 1:
        leaf = x.clone().requires_grad_(True)
        want = F.avg_pool2d(leaf, 3, 1, 1, count_include_pad=True)
        (want * R).sum().backward()
        xd = nhwc(x).requires_grad_(True)
        got = ops_conv.avgpool3(xd)
        (got * nhwc(R)).sum().backward()
        assert rel_err(got.permute(0, 3, 1, 2), want) < FWD_TOL
        assert rel_err(xd.grad.permute(0, 3, 1, 2), leaf.grad) < FWD_TOL


def test_freq_mean():
    from attention_based_tbn_amd import ops_conv
    x = rand((3, 2, 5, 64), 31)                                        # NHWC
    R = rand((3, 5, 64), 32)
    leaf = x.clone().requires_grad_(True)
    want = leaf.mean(1)
    (want * R).sum().backward()
    xd = x.float().to(DEV).requires_grad_(True)
    got = ops_conv.freq_mean(xd)
    assert tuple(got.shape) == (3, 5, 64)
    (got * R.float().to(DEV)).sum().backward()
    assert rel_err(got, want) < FWD_TOL and rel_err(xd.grad, leaf.grad) < FWD_TOL
    # the global mean beside it is unchanged
    assert rel_err(ops_conv.global_mean(xd.detach()), x.mean((1, 2))) < FWD_TOL
