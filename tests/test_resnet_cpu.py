"""ResNet backbones (model.arch = "resnet") without a GPU: the checkpoint-name contract against the plain-torch twin
(tests/resnet_twin.py; the reference wraps torchvision's children in `self.model = nn.Sequential(...)`,
core/models/resnet.py:39), the modality rules of reference resnet.py:26-36, construction errors and the wiring into
TBNModel / build_model."""
import pytest
import torch

from tests.resnet_twin import TwinResnet, randomize


def product(depth, modality="RGB", cin=3, **kw):
    from attention_based_tbn_amd.core.models.resnet import Resnet
    return Resnet(depth, modality, cin, **kw)


def resnet_cfg(*extra):
    from attention_based_tbn_amd.config import get_modality, load_config
    cfg = load_config(["model.arch=resnet", "model.resnet.depth=18", "model.attention.enable=False"] + list(extra))
    return cfg, get_modality(cfg)


@pytest.mark.parametrize("depth,nkeys,width", [(18, 120, 512), (50, 318, 2048)])
def test_state_dict_is_the_reference_one(depth, nkeys, width):
    net, twin = product(depth), TwinResnet(depth)
    sd, want = net.state_dict(), twin.state_dict()
    assert len(want) == nkeys
    assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [(k, tuple(v.shape), v.dtype) for k, v in want.items()]
    assert net.feature_size == width == twin.feature_size
    for k in ("model.0.weight", "model.1.num_batches_tracked", "model.4.0.conv1.weight", "model.5.0.downsample.0.weight",
              "model.5.0.downsample.1.running_var", "model.7.%d.bn2.bias" % (1 if depth == 18 else 2)):
        assert k in sd, k
    assert tuple(sd["model.0.weight"].shape) == (64, 3, 7, 7)            # OIHW
    # strict load in both directions, values arrive
    randomize(twin, 3)
    net.load_state_dict(twin.state_dict(), strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, twin.state_dict()[k]), k
    randomize(net, 4)
    twin.load_state_dict(net.state_dict(), strict=True)
    assert torch.equal(twin.model[7][0].downsample[0].weight, net.model[7][0].downsample[0].weight)


def test_initialisation_is_torchvisions():
    torch.manual_seed(0)
    net = product(18)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
    w = net.model[4][0].conv1.weight           # kaiming_normal_(fan_out, relu): std = sqrt(2 / (64 * 9))
    assert abs(float(w.detach().std()) / (2.0 / (64 * 9)) ** 0.5 - 1) < 0.05


def test_audio_conv1_is_the_channel_mean():
    torch.manual_seed(5)
    rgb = product(18)
    torch.manual_seed(5)
    audio = product(18, "Audio", 1)
    w = audio.model[0].weight
    assert tuple(w.shape) == (64, 1, 7, 7) and isinstance(w, torch.nn.Parameter) and w.requires_grad
    assert torch.equal(w, rgb.model[0].weight.mean(dim=1).unsqueeze(1))
    assert audio.state_dict()["model.0.weight"].shape == (64, 1, 7, 7) and len(audio.state_dict()) == 120
    # from supplied (torchvision-named) weights: the mean of THOSE filters
    twin = randomize(TwinResnet(18), 9)
    tv = {}
    names = {"model.0": "conv1", "model.1": "bn1", "model.4": "layer1", "model.5": "layer2", "model.6": "layer3",
             "model.7": "layer4"}
    for k, v in twin.state_dict().items():
        head = ".".join(k.split(".")[:2])
        tv[names[head] + k[len(head):]] = v
    tv["fc.weight"], tv["fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)
    audio = product(18, "Audio", 1, state_dict=tv)
    assert torch.equal(audio.model[0].weight, twin.model[0].weight.mean(dim=1).unsqueeze(1))
    assert torch.equal(audio.model[6][1].bn2.running_var, twin.model[6][1].bn2.running_var)


def test_construction_errors():
    with pytest.raises(ValueError, match="resnet.py:26-36"):
        product(18, "Flow", 10)
    for depth in (0, 20, 100):
        with pytest.raises(ValueError, match="model_depth"):
            product(depth)
    from attention_based_tbn_amd.core.models import TBNModel
    cfg, mod = resnet_cfg("model.attention.enable=True", "data.flow.enable=False")
    assert "Audio" in mod and len(mod) > 1
    with pytest.raises(ValueError, match="attention"):
        TBNModel(cfg, mod, torch.device("cpu"))
    cfg, mod = resnet_cfg("model.arch=vgg")
    with pytest.raises(NotImplementedError):
        TBNModel(cfg, mod, torch.device("cpu"))


def test_engine_knobs_are_accepted_or_refused():
    net = product(18)
    net.use_aux_stream = net.use_branch_streams = net.stem_wgrad_last = True
    net.flip_weights_early()
    net.conv_math, net.conv_math_layers = "f32", "3x3"
    with pytest.raises(ValueError):
        net.conv_math = "bf16x6"
    with pytest.raises(ValueError):
        net.conv_math_layers = "all"
    assert not hasattr(net, "plan_sync") and not hasattr(net, "grad_bucket_fn")


def test_build_model_accepts_resnet():
    from attention_based_tbn_amd.core.models import build_model, Resnet
    cfg, mod = resnet_cfg("data.flow.enable=False", "model.freeze_base=True", "model.freeze_mode=partialbn")
    assert mod == ["RGB", "Audio"]
    model, crit, _ = build_model(cfg, mod, torch.device("cpu"))
    assert isinstance(model.Base_RGB, Resnet) and isinstance(model.Base_Audio, Resnet)
    assert model.Base_Audio.model[0].weight.shape == (64, 1, 7, 7)
    assert model.fusion.fusion_layer[0].in_features == 1024
    # "partialbn" is a no-op for resnet (reference model.py:164): everything stays trainable
    assert all(p.requires_grad for p in model.parameters())
    cfg, mod = resnet_cfg("data.flow.enable=False", "data.audio.enable=False", "model.resnet.depth=50",
                          "model.freeze_base=True", "model.freeze_mode=all")
    model, _, _ = build_model(cfg, mod, torch.device("cpu"))
    assert model.classifier.verb.in_features == 2048
    assert not any(p.requires_grad for p in model.Base_RGB.parameters())
    assert all(p.requires_grad for p in model.classifier.parameters())


def test_cpu_forward_raises():
    from attention_based_tbn_amd._lib import TbnHipError, lib
    from attention_based_tbn_amd import ops_conv
    lib()                                   # the library itself loads without a GPU
    net = product(18)
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        net(torch.zeros(1, 3, 64, 64))
    blk = net.model[4][0]
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        blk(torch.zeros(1, 16, 16, 64))
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        ops_conv.conv_bn_act(torch.zeros(1, 8, 8, 64), blk.conv1.weight, blk.bn1.weight, blk.bn1.bias,
                             blk.bn1.running_mean, blk.bn1.running_var, 1, 1)
