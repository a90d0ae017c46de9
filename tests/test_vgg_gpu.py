"""VGG backbones (core.models.VGG) on the operator-level HIP path against the plain-torch twin (tests/vgg_twin.py) run on the
CPU in float64: VGG 11 on RGB with every parameter gradient, VGG 11 with BatchNorm on one-channel audio (batch statistics,
running statistics, eval), VGG 16 on ten-channel flow at 64 x 64 (the 2 x 2 map the adaptive pool replicates), Dropout, the
chunked eval forward, and a train step with FusedSGD.

Bound (relative to the tensor's maximum): 1e-3 for everything end to end, the project's own as stated in
tests/test_resnet_gpu.py.  The gradient-parity test first asserts that file's conditioning guard: the float32 CPU twin is
within a tenth of the bound of the float64 twin on the very inputs used (seeds were picked on the CPU) -- a condition on the
test's inputs, not a tolerance of the product."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.vgg_twin import TwinVGG, randomize, rel_err  # noqa: E402

DEV = torch.device("cuda")
E2E_TOL = 1e-3


def rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def guard(a, b, bound, what):
    err = rel_err(a, b)
    assert err < bound / 10, "conditioning guard: fp32 twin vs fp64 twin on %s: %.3g (bound %.1g / 10)" % (what, err, bound)


def no_dropout(net):
    net.model.classifier[2].p = net.model.classifier[5].p = 0.0
    return net


def product(model_type, modality, cin, sd, p0=True):
    """the product on the device with the twin's (float64) state dict"""
    from attention_based_tbn_amd.core.models import VGG
    net = VGG(model_type, modality, cin)
    net.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    return (no_dropout(net) if p0 else net).to(DEV)


def twin_train_run(twin, x, R, dtype):
    twin = twin.to(dtype).train()
    twin.zero_grad()
    out = twin(x.to(dtype))
    (out * R.to(dtype)).sum().backward()
    return out.detach(), {n: p.grad.detach().clone() for n, p in twin.named_parameters()}


# ---------------------------------------------------------------------------------------------- VGG 11, RGB
@functools.lru_cache(maxsize=None)
def vgg11_reference():
    twin = no_dropout(randomize(TwinVGG("11", 3), 71).double())
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    x, R = rand((2, 3, 32, 32), 72), rand((2, 4096), 73)
    ref64 = twin_train_run(twin, x, R, torch.float64)
    ref32 = twin_train_run(twin, x, R, torch.float32)
    twin.double().load_state_dict(sd)                    # (the round trip through float32 rounded the weights)
    with torch.no_grad():
        eval64 = twin.eval()(x)
    return sd, x, R, ref64, ref32, eval64


def test_vgg11_training_forward_and_every_gradient():
    sd, x, R, (out64, g64), (out32, g32), _ = vgg11_reference()
    guard(out32, out64, E2E_TOL, "output")
    for k in g64:
        guard(g32[k], g64[k], E2E_TOL, k)
    net = product("11", "RGB", 3, sd).train()
    out = net(x.float().to(DEV))
    (out * R.float().to(DEV)).sum().backward()
    assert tuple(out.shape) == (2, 4096)
    err = rel_err(out, out64)
    print("vgg11 output", err)
    assert err < E2E_TOL, err
    grads = dict(net.named_parameters())
    assert set(grads) == set(g64) and len(g64) == 20
    for k, want in g64.items():
        assert grads[k].grad is not None and grads[k].grad.shape == want.shape, k
        err = rel_err(grads[k].grad, want)
        print("vgg11", k, err)
        assert err < E2E_TOL, (k, err)


def test_vgg11_dropout_masks_and_scales():
    sd, x, _, _, _, eval64 = vgg11_reference()
    net = product("11", "RGB", 3, sd, p0=False)
    net.model.classifier[2].p, net.model.classifier[5].p = 0.0, 0.5          # read at every forward
    xd = x.float().to(DEV)
    with torch.no_grad():
        e1, e2 = net.eval()(xd), net(xd)
        torch.manual_seed(5)
        t1, t2 = net.train()(xd), net(xd)
    assert torch.equal(e1, e2)
    assert rel_err(e1, eval64) < E2E_TOL
    assert not torch.equal(t1, t2)
    for t in (t1, t2):
        assert bool(((t == 0) | (t == 2 * e1)).all())                         # dropped, or kept and scaled by 1 / (1 - p)
        live = e1 != 0
        dropped = float(((t == 0) & live).sum()) / float(live.sum())
        assert 0.3 < dropped < 0.7, dropped                                   # p = 0.5 over a few thousand elements


def test_eval_forward_in_chunks_is_bit_equal():
    """eval under no_grad walks the frames in chunks (the 2 GiB operand rule); forced to one frame per chunk through the
    class's private attribute the features equal the unchunked call bit for bit -- plain and BatchNorm variant"""
    from attention_based_tbn_amd.core.models import VGG
    sd, x, _, _, _, eval64 = vgg11_reference()
    xd = torch.cat([x, rand((1, 3, 32, 32), 74)]).float().to(DEV)             # three frames
    nets = [product("11", "RGB", 3, sd), product("11bn", "Audio", 1, vgg11bn_reference()[0])]
    inputs = [xd, xd[:, :1].contiguous()]
    assert VGG._chunk_frames is None
    for net, inp in zip(nets, inputs):
        net.eval()
        with torch.no_grad():
            whole = net(inp)
            try:
                VGG._chunk_frames = 1
                chunked = net(inp)
            finally:
                VGG._chunk_frames = None
        assert tuple(whole.shape) == (3, 4096) and torch.equal(whole, chunked)
    with torch.no_grad():
        assert rel_err(nets[0](xd[:2]), eval64) < E2E_TOL


# ---------------------------------------------------------------------------------------------- VGG 11 + BatchNorm, Audio
@functools.lru_cache(maxsize=None)
def vgg11bn_reference():
    twin = no_dropout(randomize(TwinVGG("11bn", 1), 81).double())
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    x = rand((4, 1, 32, 32), 82)
    with torch.no_grad():
        eval64 = twin.eval()(x)
        train64 = twin.train()(x)                           # one training step of the statistics
    after = {k: v.clone() for k, v in twin.state_dict().items()}
    return sd, x, eval64, train64, after


def test_vgg11bn_audio_training_statistics_and_eval():
    sd, x, eval64, train64, after = vgg11bn_reference()
    net = product("11bn", "Audio", 1, sd)
    xd = x.float().to(DEV)
    with torch.no_grad():
        err = rel_err(net.eval()(xd), eval64)
        print("vgg11bn eval", err)
        assert err < E2E_TOL, err
        err = rel_err(net.train()(xd), train64)
        print("vgg11bn train", err)
        assert err < E2E_TOL, err
    got = net.state_dict()
    nbn = 0
    for k, want in after.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(want) == 1, k
            nbn += 1
        elif "running_" in k:
            err = rel_err(got[k], want)
            assert err < E2E_TOL, (k, err)
            assert not torch.equal(want, sd[k])                               # the step moved it
    assert nbn == 8


# ---------------------------------------------------------------------------------------------- VGG 16, Flow, 64 x 64
def test_vgg16_flow_eval_and_live_gradients():
    twin = no_dropout(randomize(TwinVGG("16", 10), 91).double())
    x = rand((2, 10, 64, 64), 92)
    with torch.no_grad():
        eval64 = twin.eval()(x)
    net = product("16", "Flow", 10, twin.state_dict())
    xd = x.float().to(DEV)
    with torch.no_grad():
        err = rel_err(net.eval()(xd), eval64)
    print("vgg16 flow eval", err)
    assert err < E2E_TOL, err
    out = net.train()(xd)
    (out * rand((2, 4096), 93).float().to(DEV)).sum().backward()
    params = dict(net.named_parameters())
    assert len(params) == 30
    for k, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


# ---------------------------------------------------------------------------------------------- a train step
def test_train_step_with_fused_sgd_follows_the_weights():
    """features -> one ops.linear head -> cross entropy, stepped with FusedSGD: every parameter moves, and a second forward
    matches the twin loaded with the NEW weights (the kernel-layout weight copies keyed on `_version` follow the update)"""
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.utils.optim import FusedSGD
    sd, x, _, _, _, _ = vgg11_reference()
    net = product("11", "RGB", 3, sd).train()
    head_w = (rand((32, 4096), 75, (1.0 / 4096) ** 0.5).float().to(DEV)).requires_grad_(True)
    head_b = torch.zeros(32, device=DEV, requires_grad=True)
    target = torch.tensor([3, 17], device=DEV)
    opt = FusedSGD(list(net.parameters()) + [head_w, head_b], lr=0.01, momentum=0.9)
    xd = x.float().to(DEV)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    first = net(xd)
    loss = torch.nn.functional.cross_entropy(ops.linear(first, head_w, head_b), target)
    loss.backward()
    opt.step()
    for k, p in net.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k
    second = net(xd)
    assert not torch.equal(first, second)
    twin = no_dropout(TwinVGG("11", 3)).double()
    twin.load_state_dict({k: v.double().cpu() for k, v in net.state_dict().items()}, strict=True)
    with torch.no_grad():
        want = twin.train()(x)
    err = rel_err(second, want)
    print("after the step", err)
    assert err < E2E_TOL, err
    # the frames' gradient is never formed
    xg = xd.clone().requires_grad_(True)
    out = net(xg)
    with pytest.raises(TbnHipError, match="gradient with respect to the input frames"):
        out.sum().backward()
