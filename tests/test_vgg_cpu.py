"""VGG backbones (core.models.VGG) without a GPU: the checkpoint-name contract against the plain-torch twin
(tests/vgg_twin.py; the reference keeps torchvision's `features` / `avgpool` / `classifier` under `self.model` and removes the
last Linear, core/models/vgg.py:33-36), torchvision's initialisation, the modality rule of reference vgg.py:24-31, the
construction and input errors, the knobs TBNModel sets on a backbone, and the scope boundary (model.arch = vgg stays refused
by TBNModel)."""
import functools

import pytest
import torch
import torch.nn as nn

from tests.vgg_twin import KEY_COUNTS, TwinVGG, randomize

TYPES = ("16", "16bn", "11", "11bn")


def product(model_type, modality="RGB", cin=3, **kw):
    from attention_based_tbn_amd.core.models.vgg import VGG
    return VGG(model_type, modality, cin, **kw)


@functools.lru_cache(maxsize=None)
def fresh(model_type):
    """a freshly initialised product, shared by the tests that only read it"""
    torch.manual_seed(11)
    return product(model_type)


@pytest.mark.parametrize("model_type", TYPES)
def test_state_dict_is_the_reference_one(model_type):
    net, twin = fresh(model_type), TwinVGG(model_type)
    sd, want = net.state_dict(), twin.state_dict()
    assert len(want) == KEY_COUNTS[model_type] == len(sd)
    assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [(k, tuple(v.shape), v.dtype) for k, v in want.items()]
    assert net.feature_size == 4096 == twin.feature_size
    last_conv = {"16": 28, "16bn": 40, "11": 18, "11bn": 25}[model_type]
    for k in ("model.features.0.weight", "model.features.0.bias", "model.features.%d.weight" % last_conv,
              "model.classifier.0.weight", "model.classifier.3.bias"):
        assert k in sd, k
    assert ("model.features.1.num_batches_tracked" in sd) == model_type.endswith("bn")
    assert not any(k.startswith("model.classifier.6") for k in sd)
    assert tuple(sd["model.features.0.weight"].shape) == (64, 3, 3, 3)                 # OIHW
    assert tuple(sd["model.classifier.0.weight"].shape) == (4096, 25088)
    children = [n for n, _ in net.model.named_children()]
    assert children == ["features", "avgpool", "classifier"]
    assert [type(m) for m in net.model.classifier] == [nn.Linear, nn.ReLU, nn.Dropout, nn.Linear, nn.ReLU, nn.Dropout]


@pytest.mark.parametrize("model_type", ("11", "11bn"))
def test_strict_load_in_both_directions(model_type):
    net, twin = product(model_type), TwinVGG(model_type)
    randomize(twin, 3)
    net.load_state_dict(twin.state_dict(), strict=True)
    tsd = twin.state_dict()
    for k, v in net.state_dict().items():
        assert torch.equal(v, tsd[k]), k
    randomize(net, 4)
    twin.load_state_dict(net.state_dict(), strict=True)
    assert torch.equal(twin.model.features[0].weight, net.model.features[0].weight)
    assert torch.equal(twin.model.classifier[3].bias, net.model.classifier[3].bias)


@pytest.mark.parametrize("model_type", ("16", "11bn"))
def test_initialisation_is_torchvisions(model_type):
    """conv: kaiming_normal_(fan_out, relu) -> std = sqrt(2 / (cout * 9)), bias 0; BatchNorm 1 / 0; Linear N(0, 0.01), bias 0"""
    net = fresh(model_type)
    seen = set()
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            want = (2.0 / (m.out_channels * 9)) ** 0.5
            w, n = m.weight.detach(), m.weight.numel()
            # the standard deviation of n normal draws is within 5 / sqrt(2 n) of the truth (five sigma)
            assert abs(float(w.std()) / want - 1) < 5 / (2 * n) ** 0.5, (m, float(w.std()), want)
            assert abs(float(w.mean())) < 5 * want / n ** 0.5
            assert float(m.bias.detach().abs().max()) == 0
            seen.add("conv")
        elif isinstance(m, nn.BatchNorm2d):
            assert torch.equal(m.weight.detach(), torch.ones_like(m.weight)) and float(m.bias.detach().abs().max()) == 0
            assert float(m.running_mean.abs().max()) == 0 and torch.equal(m.running_var, torch.ones_like(m.running_var))
            assert int(m.num_batches_tracked) == 0
            seen.add("bn")
        elif isinstance(m, nn.Linear):
            w, n = m.weight.detach(), m.weight.numel()
            assert abs(float(w.std()) / 0.01 - 1) < 5 / (2 * n) ** 0.5
            assert abs(float(w.mean())) < 5 * 0.01 / n ** 0.5
            assert float(m.bias.detach().abs().max()) == 0
            seen.add("linear")
    assert seen == ({"conv", "bn", "linear"} if model_type.endswith("bn") else {"conv", "linear"})


@pytest.mark.parametrize("modality,cin", [("Flow", 10), ("Audio", 1)])
def test_other_modalities_get_a_fresh_first_conv(modality, cin):
    """reference vgg.py:24-31: nn.Conv2d(in_channels, 64, 3, 1, 1) with PyTorch's default initialisation -- NOT the mean of
    the RGB filters (the ResNet rule)"""
    sd = {k[len("model."):]: v.clone() for k, v in randomize(TwinVGG("11"), 5).state_dict().items()}
    net = product("11", modality, cin, state_dict=sd)
    conv = net.model.features[0]
    assert tuple(conv.weight.shape) == (64, cin, 3, 3) and tuple(conv.bias.shape) == (64,)
    assert conv.stride == (1, 1) and conv.padding == (1, 1) and conv.kernel_size == (3, 3)
    rgb_mean = sd["features.0.weight"].mean(dim=1, keepdim=True)
    assert not torch.allclose(conv.weight, rgb_mean.expand_as(conv.weight))
    # the default initialisation is uniform in +- 1 / sqrt(fan_in), for the bias as well (not zero, not normal)
    bound = 1.0 / (cin * 9) ** 0.5
    assert float(conv.weight.detach().abs().max()) <= bound and float(conv.weight.detach().abs().max()) > 0.8 * bound
    assert 0 < float(conv.bias.detach().abs().max()) <= bound
    # everything else is what the state dict brought
    assert torch.equal(net.model.features[3].weight, sd["features.3.weight"])
    assert tuple(net.state_dict()["model.features.0.weight"].shape) == (64, cin, 3, 3)


def test_state_dict_argument_ignores_the_removed_linear():
    sd = {k[len("model."):]: v.clone() for k, v in randomize(TwinVGG("11bn"), 6).state_dict().items()}
    sd["classifier.6.weight"], sd["classifier.6.bias"] = torch.zeros(10, 4096), torch.zeros(10)
    net = product("11bn", state_dict=sd)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k[len("model."):]]), k
    with pytest.raises(RuntimeError):                       # any other stray or missing key is an error (strict)
        product("11bn", state_dict={k: v for k, v in sd.items() if k != "features.0.bias"})


def test_construction_and_input_errors():
    from attention_based_tbn_amd._lib import TbnHipError
    for bad in ("19", 13, "16_bn", "vgg16"):
        with pytest.raises(ValueError, match="model_type"):
            product(bad)
    assert product(11).model_type == "11"                   # compared as str(model_type), as the reference does
    net = fresh("11")
    with pytest.raises(ValueError, match="five"):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="five"):
        net(torch.zeros(1, 3, 64, 31))
    with pytest.raises(TbnHipError, match="CPU"):
        net(torch.zeros(1, 3, 32, 32))


def test_engine_knobs_are_accepted_or_refused():
    net = fresh("11")
    net.use_aux_stream = net.use_branch_streams = net.stem_wgrad_last = True
    net.flip_weights_early()
    net.conv_math, net.conv_math_layers = "f32", "3x3"
    with pytest.raises(ValueError):
        net.conv_math = "bf16x6"
    with pytest.raises(ValueError):
        net.conv_math_layers = "all"
    assert not hasattr(net, "plan_sync") and not hasattr(net, "grad_bucket_fn")
    net.use_aux_stream = net.use_branch_streams = net.stem_wgrad_last = False


def test_export_and_scope_boundary():
    """`from core.models import VGG` works (the last name of the reference's import line); TBNModel keeps refusing
    model.arch = vgg in this step"""
    from attention_based_tbn_amd.core.models import TBNModel, VGG
    from attention_based_tbn_amd.core.models.vgg import VGG as direct
    from attention_based_tbn_amd.config import get_modality, load_config
    assert VGG is direct
    cfg = load_config(["model.arch=vgg", "model.attention.enable=False"])
    with pytest.raises(NotImplementedError):
        TBNModel(cfg, get_modality(cfg), torch.device("cpu"))


def test_new_entries_are_declared_and_exported():
    from attention_based_tbn_amd import _lib
    handle = _lib.lib()
    for name in ("tbn_conv3_first_stat_rows", "tbn_conv3_first_fwd", "tbn_conv3_first_wgrad_workspace_floats",
                 "tbn_conv3_first_wgrad", "tbn_maxpool2_fwd", "tbn_maxpool2_bwd", "tbn_adaptive_avgpool7_fwd",
                 "tbn_adaptive_avgpool7_bwd"):
        assert name in _lib.SIGNATURES and getattr(handle, name) is not None
    # the host-only queries answer without a device: 0 for what the entries refuse
    assert handle.tbn_conv3_first_stat_rows(2, 3, 32, 32) == 2 * 4
    assert handle.tbn_conv3_first_stat_rows(2, 17, 32, 32) == 0 and handle.tbn_conv3_first_stat_rows(2, 0, 32, 32) == 0
    assert handle.tbn_conv3_first_wgrad_workspace_floats(2, 10, 32, 32) == 8 * 64 * 9 * 10
    assert handle.tbn_conv3_first_wgrad_workspace_floats(96, 3, 224, 224) == 1024 * 64 * 9 * 3
    assert handle.tbn_conv3_first_wgrad_workspace_floats(0, 3, 224, 224) == 0
