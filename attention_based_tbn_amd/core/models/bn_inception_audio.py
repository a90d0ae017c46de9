"""BNInception_Audio: the BN-Inception trunk behind the separable 1x3 / 3x1 audio stem, composed from the stand-alone HIP
operators.

API mirror of reference core/models/bn_inception_audio.py: `BNInception_Audio(num_classes=1000, attend=False)` with
`features()`, `logits()`, `forward()` (:407-1029).  The two stem branches (conv1_1x3_s2: three taps along frequency,
conv1_3x1_s2: three taps along time, both Conv2d(1, 32, stride 2) + BatchNorm + ReLU, :11-20) are concatenated to 64 channels
in front of pool1_3x3_s2; from conv2_3x3_reduce on the graph is the BN-Inception trunk.

nn.Conv2d / nn.BatchNorm2d / nn.Linear are PARAMETER CONTAINERS under the reference's attribute names, registered in the
reference's order: the state-dict keys, their order and shapes are the reference's and its checkpoints load with strict=True.
Their forward is never called.  Every numerical op runs in libtbn_hip.so through attention_based_tbn_amd.ops_conv: the stem
through tbn_audio_stem_* and the pooled BatchNorm, every conv + BatchNorm + ReLU as one autograd node of conv / BatchNorm
launches, the pools through tbn_maxpool3_* / tbn_avgpool3_fwd, the head through tbn_spatial_mean_*.  Like the ResNets this
backbone does not go through the backbone engine (no plans, autotune, riders, bucketed gradient sync).

The graph is stated once: the trunk's layer hyper-parameters come by name from the engine's layer table
(tbn_backbone_conv_info, as BNInception.__init__ reads them), the block structure from `_BLOCKS` of bn_inception.py.
"""
import ctypes as C

import torch
import torch.nn as nn

from ... import ops_conv
from ..._lib import ConvInfo, call, lib
from .bn_inception import _BLOCKS, reference_conv_order
from .ops_backbone import OpsBackbone, conv_bn_relu, count_batch

# (name, kernel, padding) of the two stem branches, stride 2 (reference bn_inception_audio.py:11-13, 16-18)
_STEM = (("conv1_1x3_s2", (3, 1), (1, 0)), ("conv1_3x1_s2", (1, 3), (0, 1)))
# the pool in front of pool_proj is AvgPool2d(3, 1, 1) in every block but this one: MaxPool2d(3, 1, 1) (:394-396); a block
# without pool_proj (3c, 4e) passes MaxPool2d(3, 2, ceil_mode=True) of its input through (:155-157, 327-329)
_MAX_POOL_PROJ = ("5b",)


def _trunk_layers():
    """{conv name: (cin, cout, k, stride, pad)} of everything behind the stem, from the engine's layer table (needs the
    library, not a GPU)"""
    probe = C.c_void_p()
    call("tbn_backbone_plan_create", 1, 1, 64, 64, C.byref(probe))
    try:
        info, table = ConvInfo(), {}
        for i in range(lib().tbn_backbone_num_convs(probe)):
            call("tbn_backbone_conv_info", probe, i, C.byref(info))
            table[info.name.decode()] = (info.cin, info.cout, info.ksize, info.stride, info.pad)
    finally:
        lib().tbn_backbone_plan_destroy(probe)
    return {name: table[name] for name in reference_conv_order()[1:]}


class BNInception_Audio(OpsBackbone, nn.Module):
    def __init__(self, num_classes=1000, attend=False):
        super().__init__()
        self.attend = attend
        self.is_audio = True
        self.feature_size = 1024
        self.num_classes = num_classes
        for name, k, pad in _STEM:
            setattr(self, name, nn.Conv2d(1, 32, kernel_size=k, stride=(2, 2), padding=pad))
            setattr(self, name + "_bn", nn.BatchNorm2d(32, affine=True))
        self._layers = _trunk_layers()
        for name, (cin, cout, k, stride, pad) in self._layers.items():
            setattr(self, name, nn.Conv2d(cin, cout, kernel_size=(k, k), stride=(stride, stride), padding=(pad, pad)))
            setattr(self, name + "_bn", nn.BatchNorm2d(cout, affine=True))
        self.last_linear = nn.Linear(1024, num_classes)

    def set_bn_trainable(self, first, rest):
        """BN affine requires_grad split of TBNModel 'partialbn' (reference model.py:164-176: every BatchNorm2d child
        with index > 1 is frozen, which leaves conv1_1x3_s2_bn alone)"""
        for name, m in self.named_children():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.requires_grad = m.bias.requires_grad = first if name == _STEM[0][0] + "_bn" else rest

    # ---- compute
    def _unit(self, name, x):
        """relu(bn(conv(x))) of the trunk layer `name`, NHWC in and out"""
        return conv_bn_relu(getattr(self, name), getattr(self, name + "_bn"), x, self.training)

    def _stem(self, x):
        """NCHW spectrogram -> the NHWC output of pool1_3x3_s2"""
        self._need_gpu(x)
        (a, _, _), (b, _, _) = _STEM
        bn_a, bn_b = getattr(self, a + "_bn"), getattr(self, b + "_bn")
        out = ops_conv.audio_stem_bn_pool(x, getattr(self, a), bn_a, getattr(self, b), bn_b, training=self.training)
        count_batch(self.training, bn_a, bn_b)
        return out

    def _trunk(self, x):
        """the NHWC output of pool1_3x3_s2 -> the NHWC (n, h', w', 1024) feature map"""
        x = self._unit("conv2_3x3", self._unit("conv2_3x3_reduce", x))
        x = ops_conv.maxpool3(x, 2, 0, True)                                  # pool2_3x3_s2
        for b, has_1x1, has_proj in _BLOCKS:
            p = "inception_" + b
            outs = [self._unit(p + "_1x1", x)] if has_1x1 else []
            outs.append(self._unit(p + "_3x3", self._unit(p + "_3x3_reduce", x)))
            y = self._unit(p + "_double_3x3_1", self._unit(p + "_double_3x3_reduce", x))
            outs.append(self._unit(p + "_double_3x3_2", y))
            if has_proj:
                pooled = ops_conv.maxpool3(x, 1, 1, True) if b in _MAX_POOL_PROJ else ops_conv.avgpool3(x)
                outs.append(self._unit(p + "_pool_proj", pooled))
            else:
                outs.append(ops_conv.maxpool3(x, 2, 0, True))
            x = torch.cat(outs, 3)
        return x

    def pool1(self, x):
        """the reference-shaped (n, 64, h1, w1) output of pool1_3x3_s2 (a permuted view of the NHWC result)"""
        return self._stem(x).permute(0, 3, 1, 2)

    def features(self, x):
        """reference-shaped (n, 1024, h', w') feature map (a permuted view of the NHWC result)"""
        return self._trunk(self._stem(x)).permute(0, 3, 1, 2)

    def logits(self, features):
        """reference bn_inception_audio.py:1005-1024 on a (n, 1024, h', w') tensor: the mean over frequency alone,
        (n, 1024, 1, w'), when `attend`; else the global mean (n, 1024)"""
        nhwc = features.permute(0, 2, 3, 1)
        if self.attend:
            return ops_conv.freq_mean(nhwc).permute(0, 2, 1).unsqueeze(2)
        return ops_conv.global_mean(nhwc)

    def forward(self, x):
        return self.logits(self.features(x))

    def forward_sequence(self, x):
        """attended-audio features in the native (n, w', 1024) layout TBNModel's attention heads read"""
        return ops_conv.freq_mean(self._trunk(self._stem(x)))
