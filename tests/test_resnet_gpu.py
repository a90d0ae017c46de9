"""ResNet backbones on the operator-level HIP path against the plain-torch twin (tests/resnet_twin.py) run on the CPU in
float64: single residual blocks, Resnet(18) with every parameter gradient, Resnet(50) on one-channel audio (the 2048-channel
join), and TBNModel with arch = resnet through a fused train step.

Bounds (relative to the tensor's maximum): forward of a block 1e-4 (TOL of tests/test_kernels_gpu.py), gradients of a block
and everything end-to-end 1e-3 (the project's end-to-end bound: a block chains 3-4 operators).

Conditioning guard.  ReLU / max-pool decisions of a deep network can flip under fp32 rounding, after which single gradient
tensors differ by 1e-1 whatever computes them (measured for ResNet-50 at small shapes).  So every gradient-parity test first
asserts that the float32 CPU twin is within ONE TENTH of the test's bound of the float64 twin on the very inputs it uses:
a condition on the test's inputs (seeds were picked on the CPU), not a tolerance of the product."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.resnet_twin import TwinBasicBlock, TwinBottleneck, TwinResnet, randomize, rel_err  # noqa: E402

DEV = torch.device("cuda")
FWD_TOL, GRAD_TOL, E2E_TOL = 1e-4, 1e-3, 1e-3


def rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def twin_run(twin, x, R, dtype, want_dx=True):
    """training forward + backward of loss = sum(out * R) -> (out, dx, {name: grad})"""
    twin = twin.to(dtype).train()
    twin.zero_grad()
    x = x.to(dtype).clone().requires_grad_(want_dx)
    out = twin(x)
    (out * R.to(dtype)).sum().backward()
    return out.detach(), (x.grad.detach() if want_dx else None), {n: p.grad.detach().clone() for n, p in twin.named_parameters()}


def guard(a, b, bound, what):
    err = rel_err(a, b)
    assert err < bound / 10, "conditioning guard: fp32 twin vs fp64 twin on %s: %.3g (bound %.1g / 10)" % (what, err, bound)


# ---------------------------------------------------------------------------------------------- blocks
BLOCKS = {
    "basic_64_64": (TwinBasicBlock, "BasicBlock", 64, 64, 1, 101),
    "basic_64_128_s2": (TwinBasicBlock, "BasicBlock", 64, 128, 2, 102),
    "bottleneck_256_64_256": (TwinBottleneck, "Bottleneck", 256, 64, 1, 103),
    "bottleneck_256_128_512_s2": (TwinBottleneck, "Bottleneck", 256, 128, 2, 104),
}


@functools.lru_cache(maxsize=None)
def block_reference(name):
    tcls, _, cin, width, stride, seed = BLOCKS[name]
    twin = randomize(tcls(cin, width, stride), seed).double()
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    x = rand((2, cin, 16, 16), seed + 1000).relu() + 0.1 * rand((2, cin, 16, 16), seed + 2000).abs()   # a post-ReLU input
    out = twin.train()(x)
    R = rand(tuple(out.shape), seed + 3000)
    twin.load_state_dict(sd)
    ref64 = twin_run(twin, x, R, torch.float64)
    twin.load_state_dict(sd)
    ref32 = twin_run(twin, x, R, torch.float32)
    twin.double()
    return sd, x, R, ref64, ref32


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_matches_twin(name):
    from attention_based_tbn_amd.core.models import resnet
    _, pcls, cin, width, stride, _ = BLOCKS[name]
    sd, x, R, (out64, dx64, g64), (out32, dx32, g32) = block_reference(name)
    guard(out32, out64, FWD_TOL, "output")
    guard(dx32, dx64, GRAD_TOL, "input gradient")
    for k in g64:
        guard(g32[k], g64[k], GRAD_TOL, k)
    blk = getattr(resnet, pcls)(cin, width, stride)
    blk.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    blk.to(DEV).train()
    xd = x.float().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)          # NHWC
    out = blk(xd)
    (out * R.float().permute(0, 2, 3, 1).to(DEV)).sum().backward()
    err = rel_err(out.permute(0, 3, 1, 2), out64)
    print(name, "output", err)
    assert err < FWD_TOL, err
    err = rel_err(xd.grad.permute(0, 3, 1, 2), dx64)
    print(name, "dx", err)
    assert err < GRAD_TOL, err
    grads = dict(blk.named_parameters())
    assert set(grads) == set(g64)
    for k, want in g64.items():
        assert grads[k].grad is not None and grads[k].grad.shape == want.shape, k
        err = rel_err(grads[k].grad, want)
        print(name, k, err)
        assert err < GRAD_TOL, (k, err)
    for k, m in blk.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert int(m.num_batches_tracked) == 1, k


def test_block_with_frozen_first_unit_and_no_input_gradient():
    """requires_grad = False on conv1 / bn1 and an input without gradient: the remaining gradients are unchanged, the
    frozen parameters get none (their weight-gradient and the data-gradient launches below conv2 are skipped)"""
    from attention_based_tbn_amd.core.models import resnet
    name = "bottleneck_256_128_512_s2"
    _, pcls, cin, width, stride, _ = BLOCKS[name]
    sd, x, R, (out64, _, g64), _ = block_reference(name)
    blk = getattr(resnet, pcls)(cin, width, stride)
    blk.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    blk.to(DEV).train()
    for p in list(blk.conv1.parameters()) + list(blk.bn1.parameters()):
        p.requires_grad = False
    out = blk(x.float().permute(0, 2, 3, 1).contiguous().to(DEV))
    (out * R.float().permute(0, 2, 3, 1).to(DEV)).sum().backward()
    assert rel_err(out.permute(0, 3, 1, 2), out64) < FWD_TOL
    for k, p in blk.named_parameters():
        if k.startswith(("conv1.", "bn1.")):
            assert p.grad is None, k
        else:
            err = rel_err(p.grad, g64[k])
            assert err < GRAD_TOL, (k, err)


def test_conv_bn_act_unit_and_its_residual_gradient():
    """the single fused unit with an EXTERNAL residual: output and all five gradients against float64 torch"""
    from attention_based_tbn_amd import ops_conv
    import torch.nn.functional as F
    cin, cout = 64, 128
    x, w = rand((2, cin, 9, 7), 1).relu(), rand((cout, cin, 3, 3), 2, (2.0 / (9 * cin)) ** 0.5)
    res, R = rand((2, cout, 5, 4), 3), rand((2, cout, 5, 4), 4)
    gamma, beta = 0.5 + rand((cout,), 5).abs(), rand((cout,), 6, 0.2)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, gamma, beta, res)]
    y = F.conv2d(leaves[0], leaves[1], None, 2, 1)
    ref = F.relu(F.batch_norm(y, None, None, leaves[2], leaves[3], True, 0.1, 1e-5) + leaves[4])
    (ref * R).sum().backward()
    nhwc = lambda t: t.float().permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    dev = [nhwc(x).requires_grad_(True), w.float().to(DEV).requires_grad_(True), gamma.float().to(DEV).requires_grad_(True),
           beta.float().to(DEV).requires_grad_(True), nhwc(res).requires_grad_(True)]
    rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    out = ops_conv.conv_bn_act(dev[0], dev[1], dev[2], dev[3], rm, rv, 2, 1, residual=dev[4], relu=True, training=True)
    (out * nhwc(R)).sum().backward()
    assert rel_err(out.permute(0, 3, 1, 2), ref) < FWD_TOL
    for i, (d, l) in enumerate(zip(dev, leaves)):
        got = d.grad.permute(0, 3, 1, 2) if i in (0, 4) else d.grad
        err = rel_err(got, l.grad)
        print("conv_bn_act grad", i, err)
        assert err < GRAD_TOL, (i, err)
    assert rel_err(rm, 0.1 * y.detach().mean((0, 2, 3))) < FWD_TOL
    assert rel_err(rv, 0.9 + 0.1 * y.detach().var((0, 2, 3), unbiased=True)) < FWD_TOL


# ---------------------------------------------------------------------------------------------- Resnet(18), RGB
R18_SEED = 7


@functools.lru_cache(maxsize=None)
def r18_reference():
    twin = randomize(TwinResnet(18), R18_SEED).double()
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    x = rand((4, 3, 64, 64), R18_SEED + 1)
    R = rand((4, 512), R18_SEED + 2)
    ref64 = twin_run(twin, x, R, torch.float64, want_dx=False)
    after = {k: v.clone() for k, v in twin.state_dict().items()}
    twin.load_state_dict(sd)
    ref32 = twin_run(twin, x, R, torch.float32, want_dx=False)
    twin.double()
    return twin, sd, after, x, R, ref64, ref32


def test_resnet18_training_step_and_eval_match_twin():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.models import Resnet
    twin, sd, after, x, R, (f64, _, g64), (f32, _, g32) = r18_reference()
    guard(f32, f64, E2E_TOL, "features")
    for k in g64:
        guard(g32[k], g64[k], E2E_TOL, k)
    net = Resnet(18, "RGB", 3)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    net.to(DEV).train()
    xd = x.float().to(DEV)
    feat = net(xd)
    assert tuple(feat.shape) == (4, 512)
    (feat * R.float().to(DEV)).sum().backward()
    err = rel_err(feat, f64)
    print("resnet18 features", err)
    assert err < E2E_TOL, err
    params = dict(net.named_parameters())
    assert set(params) == set(g64)
    worst = 0.0
    for k, want in g64.items():
        assert params[k].grad is not None and params[k].grad.shape == want.shape, k
        err = rel_err(params[k].grad, want)
        worst = max(worst, err)
        assert err < E2E_TOL, (k, err)
    print("resnet18 worst parameter gradient", worst)
    got = net.state_dict()
    for k, want in after.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == 1 == int(want), k
        elif "running_" in k:
            err = rel_err(got[k], want)
            assert err < E2E_TOL, (k, err)
    # eval: running statistics, against the twin's eval forward with the SAME state dict
    twin.load_state_dict({k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in got.items()})
    net.eval()
    with torch.no_grad():
        fe = net(xd)
        want = twin.eval()(x)
    err = rel_err(fe, want)
    print("resnet18 eval features", err)
    assert err < E2E_TOL, err
    assert int(net.state_dict()["model.1.num_batches_tracked"]) == 1        # eval does not advance it
    # no input-frame gradient, no backward through an eval-mode backbone
    net.train()
    xg = xd.clone().requires_grad_(True)
    with pytest.raises(TbnHipError, match="gradient with respect to the input frames"):
        net(xg).sum().backward()
    net.eval()
    with pytest.raises(TbnHipError, match="eval-mode backbone"):
        net(xd).sum().backward()


# ---------------------------------------------------------------------------------------------- Resnet(50), Audio
def test_resnet50_audio_reaches_the_2048_channel_join():
    from attention_based_tbn_amd.core.models import Resnet
    twin = randomize(TwinResnet(50, in_channels=1), 11).double()
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    x = rand((4, 1, 64, 64), 12)
    with torch.no_grad():
        f64 = twin.train()(x)
    net = Resnet(50, "Audio", 1)
    assert tuple(net.model[0].weight.shape) == (64, 1, 7, 7)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    net.to(DEV).train()
    xd = x.float().to(DEV)
    feat = net(xd)
    assert tuple(feat.shape) == (4, 2048) and net.feature_size == 2048       # layer4 joins at 2048 channels
    err = rel_err(feat, f64)
    print("resnet50 audio training features", err)
    assert err < E2E_TOL, err
    (feat * rand((4, 2048), 13).float().to(DEV)).sum().backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    twin.load_state_dict({k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in net.state_dict().items()})
    net.eval()
    with torch.no_grad():
        fe = net(xd)
        want = twin.eval()(x)
    err = rel_err(fe, want)
    print("resnet50 audio eval features", err)
    assert err < E2E_TOL, err


# ---------------------------------------------------------------------------------------------- TBNModel, arch = resnet
def tbn_cfg(*extra):
    from attention_based_tbn_amd.config import get_modality, load_config
    cfg = load_config(["model.arch=resnet", "model.resnet.depth=18", "model.attention.enable=False", "data.flow.enable=False",
                       "model.fusion_dropout=0", "model.freeze_base=False", "model.num_classes.verb=12",
                       "model.num_classes.noun=20"] + list(extra))
    return cfg, get_modality(cfg)


def tbn_inputs():
    return {"RGB": rand((2, 2, 3, 64, 64), 31).float(), "Audio": rand((2, 2, 1, 64, 64), 32).float()}


def reference_logits(model, inp):
    """classifier(fusion(cat(twin features))) averaged over the segments, float64 torch, from the model's own weights;
    training-mode BatchNorm (batch statistics) in the twins"""
    sd = {k: v.detach().double().cpu() if v.is_floating_point() else v.cpu() for k, v in model.state_dict().items()}
    feats = []
    for m, cin in (("RGB", 3), ("Audio", 1)):
        twin = TwinResnet(18, in_channels=cin).double()
        twin.load_state_dict({k[len("Base_%s." % m):]: v for k, v in sd.items() if k.startswith("Base_%s." % m)})
        with torch.no_grad():
            feats.append(twin.train()(inp[m].double().reshape(4, cin, 64, 64)))
    f = torch.cat(feats, 1)
    h = torch.relu(f @ sd["fusion.fusion_layer.0.weight"].t() + sd["fusion.fusion_layer.0.bias"])
    out = {}
    for k in ("verb", "noun"):
        s = h @ sd["classifier.%s.weight" % k].t() + sd["classifier.%s.bias" % k]
        out[k] = s.reshape(2, 2, -1).mean(1)
    return out


def test_tbn_model_with_resnet_backbones_trains():
    from attention_based_tbn_amd.core.models import build_model, Resnet
    from attention_based_tbn_amd.core.utils import FusedSGD
    from attention_based_tbn_amd.core.utils.train_step import TrainStep
    cfg, mod = tbn_cfg()
    assert mod == ["RGB", "Audio"]
    torch.manual_seed(3)
    model, crit, _ = build_model(cfg, mod, DEV)
    assert isinstance(model.Base_RGB, Resnet) and isinstance(model.Base_Audio, Resnet)
    with torch.no_grad():                       # heads of a size whose update is visible in fp32 after one step
        for n, p in model.named_parameters():
            if n.startswith(("fusion.", "classifier.")) and p.dim() == 2:
                p.normal_(0, 0.05)
    model.train()
    inp = tbn_inputs()
    dev_inp = {k: v.to(DEV) for k, v in inp.items()}
    want = reference_logits(model, inp)
    out = model(dev_inp)
    for k in ("verb", "noun"):
        err = rel_err(out[k], want[k])
        print("tbn resnet logits", k, err)
        assert err < E2E_TOL, (k, err)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = FusedSGD(model.parameters(), 0.1, momentum=0.9, weight_decay=0)
    step = TrainStep(model, opt, crit, clip_grad=20)
    tgt = {"class": {"verb": torch.tensor([1, 2], device=DEV), "noun": torch.tensor([3, 4], device=DEV)}}
    loss, _ = step(0, dev_inp, tgt)
    assert bool(torch.isfinite(loss["total"]))
    for n, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        assert not torch.equal(p, before[n]), n + " did not change"
    for n, b in model.named_buffers():
        assert bool(torch.isfinite(b.float()).all()), n
    # a second forward sees the new weights (the kernel-layout weight copies are keyed on the parameters' versions)
    want2 = reference_logits(model, inp)
    out2 = model(dev_inp)
    for k in ("verb", "noun"):
        err = rel_err(out2[k], want2[k])
        print("tbn resnet logits after the step", k, err)
        assert err < E2E_TOL, (k, err)
        assert rel_err(out2[k], want[k]) > 10 * E2E_TOL, k          # and they did move


def test_tbn_model_frozen_resnet_backbones_get_no_gradient():
    from attention_based_tbn_amd.core.models import build_model
    cfg, mod = tbn_cfg("model.freeze_base=True", "model.freeze_mode=all")
    torch.manual_seed(4)
    model, crit, _ = build_model(cfg, mod, DEV)
    model.train()
    out = model({k: v.to(DEV) for k, v in tbn_inputs().items()})
    tgt = {"class": {"verb": torch.tensor([1, 2], device=DEV), "noun": torch.tensor([3, 4], device=DEV)}}
    loss, _ = model.get_loss(crit, tgt, out, 0)
    loss["total"].backward()
    for n, p in model.named_parameters():
        if n.startswith("Base_"):
            assert not p.requires_grad and p.grad is None, n
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
