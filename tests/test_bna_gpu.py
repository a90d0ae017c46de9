"""BNInception_Audio on the operator-level HIP path: against the reference class's recorded outputs
(tests/golden/bna_audio.npz, written by tests/golden/make_golden_bna.py), every parameter gradient against the plain-torch
twin (tests/bna_twin.py) run on the CPU in float64, and inside TBNModel through a fused train step.

Bounds (relative to the tensor's maximum): everything end-to-end 1e-3 (E2E_TOL of tests/test_resnet_gpu.py), the stem's running
statistics 1e-4.  The conditioning guard of tests/test_resnet_gpu.py applies to the gradient test: ReLU / max-pool decisions of
a deep network can flip under fp32 rounding, so the float32 CPU twin must be within one tenth of the bound of the float64 twin
on the very inputs the test uses."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.fill import fill_state_dict  # noqa: E402
from tests.bna_twin import STEM, TwinBNA, randomize  # noqa: E402
from tests.resnet_twin import rel_err  # noqa: E402

DEV = torch.device("cuda")
E2E_TOL, STAT_TOL = 1e-3, 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bna_audio.npz")


def rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def product(attend=False, sd=None):
    from attention_based_tbn_amd.core.models import BNInception_Audio
    net = BNInception_Audio(1000, attend)
    if sd is not None:
        net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    return net.to(DEV)


# ---------------------------------------------------------------------------------------------- the reference's outputs
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_matches_the_reference_fixture(mode):
    g = np.load(GOLDEN)
    net = product()
    net.load_state_dict(fill_state_dict(net.state_dict(), int(g["seed"])), strict=True)
    net.train(mode == "train")
    x = torch.from_numpy(g["x"].astype(np.float32)).to(DEV)
    with torch.no_grad():
        feat = net.features(x)
        net.attend = True
        freq = net.logits(feat)
        net.attend = False
        glob = net.logits(feat)
    tracked = {k: int(v) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")}
    assert len(tracked) == 70 and set(tracked.values()) == {1 if mode == "train" else 0}
    if mode == "train":
        sd = net.state_dict()
        for name in STEM:
            for stat in ("running_mean", "running_var"):
                key = "%s_bn.%s" % (name, stat)
                err = rel_err(sd[key], torch.from_numpy(g["train_" + key]))
                print("bna", key, err)
                assert err < STAT_TOL, (key, err)
    with torch.no_grad():
        p1 = net.pool1(x)             # (train: the batch statistics again, whatever the running ones have become)
    for name, got in (("p1", p1), ("feat", feat), ("logits_freq", freq), ("logits_global", glob)):
        want = torch.from_numpy(g["%s_%s" % (mode, name)])
        assert tuple(got.shape) == tuple(want.shape), name
        err = rel_err(got, want)
        print("bna", mode, name, err)
        assert err < E2E_TOL, (name, err)
    seq = net.forward_sequence(x) if mode == "eval" else None
    if seq is not None:               # the native layout of the attention heads: (n, w', 1024)
        assert tuple(seq.shape) == (2, 3, 1024) and rel_err(seq.permute(0, 2, 1).unsqueeze(2), freq) < 1e-6


# ---------------------------------------------------------------------------------------------- gradients
GRAD_SEED = 48


def twin_run(twin, x, R, dtype):
    twin = twin.to(dtype).train()
    twin.zero_grad()
    out = twin(x.to(dtype))
    (out * R.to(dtype)).sum().backward()
    return out.detach(), {n: p.grad.detach().clone() for n, p in twin.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def grad_reference():
    twin = randomize(TwinBNA(), GRAD_SEED).double()
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    x, R = rand((4, 1, 64, 64), GRAD_SEED + 1), rand((4, 1024), GRAD_SEED + 2)
    ref64 = twin_run(twin, x, R, torch.float64)
    twin.load_state_dict(sd)
    ref32 = twin_run(twin, x, R, torch.float32)
    return sd, x, R, ref64, ref32


def is_conv_bias(name):
    return name.endswith(".bias") and "_bn." not in name


def test_every_parameter_gradient_matches_the_twin():
    """loss = sum(forward(x) * R) at (4, 1, 64, 64) in training mode, seed 48 (picked on the CPU among 21..69: the seeds
    whose fp32 twin takes every ReLU / max-pool decision of the fp64 twin).  Conditioning guard as measured on the CPU:
    fp32 twin against fp64 twin, output 3.7e-5, worst parameter gradient 7.3e-5 (inception_5b_pool_proj.weight), both
    below 1e-3 / 10.  The gradient of a conv bias in front of a batch-statistics BatchNorm is exactly zero (the fp64 twin
    gives rounding noise of 4.4e-13): the product must give zeros, a relative measure does not exist there."""
    from attention_based_tbn_amd._lib import TbnHipError
    sd, x, R, (f64, g64), (f32, g32) = grad_reference()
    err = rel_err(f32, f64)
    assert err < E2E_TOL / 10, "conditioning guard: fp32 twin vs fp64 twin on the output: %.3g" % err
    for k in g64:
        if is_conv_bias(k):
            assert float(g64[k].abs().max()) < 1e-9, k
        else:
            err = rel_err(g32[k], g64[k])
            assert err < E2E_TOL / 10, "conditioning guard: fp32 twin vs fp64 twin on %s: %.3g" % (k, err)
    net = product(sd=sd).train()
    xd = x.float().to(DEV)
    out = net(xd)
    assert tuple(out.shape) == (4, 1024)
    (out * R.float().to(DEV)).sum().backward()
    err = rel_err(out, f64)
    print("bna training output", err)
    assert err < E2E_TOL, err
    params = dict(net.named_parameters())
    assert set(params) == set(g64) | {"last_linear.weight", "last_linear.bias"}
    worst = (0.0, None)
    for k, want in g64.items():
        got = params[k].grad
        assert got is not None and got.shape == want.shape, k
        if is_conv_bias(k):
            assert bool((got == 0).all()), k
            continue
        err = rel_err(got, want)
        worst = max(worst, (err, k))
        assert err < E2E_TOL, (k, err)
    print("bna worst parameter gradient", worst)
    # no input-frame gradient, no backward through an eval-mode backbone
    with pytest.raises(TbnHipError, match="gradient with respect to the input frames"):
        net(xd.clone().requires_grad_(True)).sum().backward()
    net.eval()
    tracked = int(net.conv2_3x3_bn.num_batches_tracked)
    with pytest.raises(TbnHipError, match="eval-mode backbone"):
        net(xd).sum().backward()
    assert int(net.conv2_3x3_bn.num_batches_tracked) == tracked == 2


# ---------------------------------------------------------------------------------------------- TBNModel
def audio_sequence_reference(model, audio):
    """the audio backbone's (R, T, 1024) sequence from the float64 twin with the model's own weights, batch statistics"""
    sd = {k[len("Base_Audio."):]: (v.detach().double().cpu() if v.is_floating_point() else v.cpu())
          for k, v in model.state_dict().items() if k.startswith("Base_Audio.")}
    twin = TwinBNA(attend=True).double()
    del twin.last_linear
    twin.load_state_dict(sd, strict=True)
    with torch.no_grad():
        return twin.train()(audio.double().reshape(-1, 1, 64, 256)).squeeze(2).permute(0, 2, 1)


def test_tbn_model_with_the_separable_audio_stem_trains():
    """mirror of test_tbn_model_with_resnet_backbones_trains: RGB on the engine, Audio on BNInception_Audio, attended (T = 8).
    Weight decay is on: a conv bias in front of a batch-statistics BatchNorm has a zero gradient in either backbone and
    moves through the decay alone."""
    from attention_based_tbn_amd.config import get_modality, load_config
    from attention_based_tbn_amd.core.models import BNInception, BNInception_Audio, TBNModel, build_model
    from attention_based_tbn_amd.core.utils import FusedSGD
    from attention_based_tbn_amd.core.utils.train_step import TrainStep
    cfg = load_config(["model.attention.enable=True", "model.attention.type=mha", "model.attention.attn_dropout=0",
                       "data.audio.audio_length=1.279", "data.flow.enable=False", "model.fusion_dropout=0",
                       "model.freeze_base=False", "model.num_classes.verb=12", "model.num_classes.noun=20"])
    mod = get_modality(cfg)
    assert mod == ["RGB", "Audio"]
    torch.manual_seed(3)
    TBNModel.audio_stem = "1x3_3x1"
    try:
        model, crit, _ = build_model(cfg, mod, DEV)
    finally:
        TBNModel.audio_stem = "7x7"
    assert type(model.Base_RGB) is BNInception and type(model.Base_Audio) is BNInception_Audio
    assert model.Base_Audio.attend and not hasattr(model.Base_Audio, "last_linear")
    model.Base_RGB.autotune = False            # (the heuristic plan: tuning a plan is not what this test is about)
    with torch.no_grad():                      # heads of a size whose update is visible in fp32 after one step
        for n, p in model.named_parameters():
            if n.startswith(("fusion.", "classifier.")) and p.dim() == 2:
                p.normal_(0, 0.05)
    model.train()
    inp = {"RGB": rand((2, 2, 3, 64, 64), 31).float(), "Audio": rand((2, 2, 1, 64, 256), 32).float()}
    dev_inp = {k: v.to(DEV) for k, v in inp.items()}
    want = audio_sequence_reference(model, inp["Audio"])
    assert tuple(want.shape) == (4, 8, 1024)
    with torch.no_grad():
        seq = model.Base_Audio.forward_sequence(dev_inp["Audio"].reshape(4, 1, 64, 256))
    err = rel_err(seq, want)
    print("tbn bna audio sequence", err)
    assert err < E2E_TOL, err
    out = model(dev_inp)
    assert tuple(out["verb"].shape) == (2, 12) and tuple(out["noun"].shape) == (2, 20)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = FusedSGD(model.parameters(), 0.1, momentum=0.9, weight_decay=5e-4)
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
    want2 = audio_sequence_reference(model, inp["Audio"])
    with torch.no_grad():
        seq2 = model.Base_Audio.forward_sequence(dev_inp["Audio"].reshape(4, 1, 64, 256))
    err = rel_err(seq2, want2)
    print("tbn bna audio sequence after the step", err)
    assert err < E2E_TOL, err
    assert rel_err(seq2, want) > 10 * E2E_TOL                    # and they did move
    out2 = model(dev_inp)
    for k in ("verb", "noun"):
        assert bool(torch.isfinite(out2[k]).all()) and not torch.equal(out2[k], out[k]), k
