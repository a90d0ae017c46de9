"""What the operator-level backbones share (core/models/ops_backbone.py) without a GPU: the per-unit state kept on the conv
container and the knob mix-in of Resnet, VGG and BNInception_Audio."""
import pytest
import torch


def backbones():
    from attention_based_tbn_amd.core.models import BNInception_Audio, Resnet, VGG
    return [Resnet(18, "RGB", 3), VGG("11", "RGB", 3), BNInception_Audio()]


def test_unit_state_lives_on_the_conv_and_follows_the_buffers():
    from attention_based_tbn_amd.core.models import Resnet, VGG
    from attention_based_tbn_amd.core.models.ops_backbone import unit_state
    from attention_based_tbn_amd.ops_conv import BnState
    net = Resnet(18, "RGB", 3)
    blk = net.model[5][0]                                   # conv1 is 3x3 / stride 2 / pad 1
    s = unit_state(blk.conv1, blk.bn1)
    assert isinstance(s, BnState) and unit_state(blk.conv1, blk.bn1) is s
    assert (s.stride, s.pad) == (2, 1) and s.running_mean is blk.bn1.running_mean and s.running_var is blk.bn1.running_var
    assert unit_state(blk.downsample[0], blk.downsample[1]).pad == 0 and unit_state(net.model[0], net.model[1]).pad == 3
    old = blk.bn1.running_mean
    net.double().float()                                    # replaces the buffers
    assert blk.bn1.running_mean is not old and s.running_mean is old
    assert unit_state(blk.conv1, blk.bn1) is s
    assert s.running_mean is blk.bn1.running_mean and s.running_var is blk.bn1.running_var
    assert "_tbn_state" not in net.state_dict() and not any("_tbn_state" in k for k in net.state_dict())
    # a conv without BatchNorm
    conv = VGG("11", "RGB", 3).model.features[3]
    s = unit_state(conv)
    assert (s.stride, s.pad) == (1, 1) and s.running_mean is None and s.running_var is None and unit_state(conv) is s


def test_the_three_backbones_share_the_knob_mixin():
    from attention_based_tbn_amd.core.models.ops_backbone import OpsBackbone
    for net in backbones():
        name = type(net).__name__
        assert isinstance(net, OpsBackbone) and isinstance(net, torch.nn.Module)
        assert (net.use_aux_stream, net.use_branch_streams, net.stem_wgrad_last) == (False, False, False)
        assert (net.conv_math, net.conv_math_layers) == ("f32", "3x3")
        net.use_aux_stream = net.use_branch_streams = net.stem_wgrad_last = True          # accepted and ignored
        assert net.use_aux_stream and not OpsBackbone.use_aux_stream
        net.conv_math, net.conv_math_layers = "f32", "3x3"
        net.flip_weights_early()
        with pytest.raises(ValueError, match=r"^%s: conv_math 'bf16x6' is not available \(the split-bf16 modes" % name):
            net.conv_math = "bf16x6"
        with pytest.raises(ValueError, match=r"^%s: conv_math_layers 'all' is not available; \"3x3\"" % name):
            net.conv_math_layers = "all"
        assert (net.conv_math, net.conv_math_layers) == ("f32", "3x3")
        for engine_only in ("plan_sync", "grad_bucket_fn", "_out_slot"):
            assert not hasattr(net, engine_only), (name, engine_only)
        from attention_based_tbn_amd._lib import TbnHipError
        with pytest.raises(TbnHipError, match=r"^%s: input is on the CPU.*no CPU fallback" % name):
            net(torch.zeros(1, 1 if name == "BNInception_Audio" else 3, 64, 64))
