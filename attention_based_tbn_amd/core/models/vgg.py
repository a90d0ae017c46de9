"""VGG backbones composed from the stand-alone HIP operators.

API mirror of reference core/models/vgg.py:7-41: `VGG(model_type, modality, in_channels)`, `feature_size`,
`forward(frames) -> (frames, 4096)`.  The graph is torchvision's vgg11 / vgg16 with and without BatchNorm, spelled out here:
`self.model` has the children `features` (a Sequential with torchvision's indices), `avgpool` and `classifier` (the last
Linear removed, as the reference removes it), so the state-dict names are the reference's (`model.features.0.weight`, ...,
`model.classifier.3.bias`) and its checkpoints load with strict=True.

The layer table.  Every convolution is 3x3 / stride 1 / pad 1 with a bias and is followed by ReLU (in the `bn` variants by
BatchNorm2d, then ReLU); "M" is MaxPool2d(2, 2).  The 11-layer network has one convolution in front of each of its first two
pools and two in front of each of the other three; the 16-layer network has two, two, three, three, three.  The widths are
64, 128, 256, 512, 512 per stage.  Five pools: the map shrinks by 32.

nn.Conv2d / nn.BatchNorm2d / nn.Linear / nn.Dropout are PARAMETER CONTAINERS only: their forward is never called (the Dropout
containers' `p` and `training` are read at every forward).  Every numerical op runs in libtbn_hip.so through
attention_based_tbn_amd.ops_conv and ops: the first layer through tbn_conv3_first_*, the other convolutions through
tbn_conv2d_*, the pools through tbn_maxpool2_* and tbn_adaptive_avgpool7_*, the classifier through tbn_linear_*.  In the plain
variants the ReLU mask of a convolution that feeds a pool is applied by the pool's backward (one pass over the map instead of
two).  Like Resnet this backbone does not go through the backbone engine.
"""
import torch
import torch.nn as nn

from ... import ops, ops_conv
from .ops_backbone import OpsBackbone, conv_bn_relu, count_batch, unit_state

_STAGE_WIDTHS = (64, 128, 256, 512, 512)
_STAGE_CONVS = {"11": (1, 1, 2, 2, 2), "16": (2, 2, 3, 3, 3)}       # convolutions in front of each of the five pools
_MODEL_TYPES = ("16", "16bn", "11", "11bn")
_MIN_SIZE = 32                                                       # five MaxPool2d(2, 2)
_OPERAND_LIMIT = (1 << 31) - 1       # bytes: the convolution entries refuse an operand of 2 GiB or more


def _features(depth, batch_norm):
    layers, cin = [], 3
    for width, count in zip(_STAGE_WIDTHS, _STAGE_CONVS[depth]):
        for _ in range(count):
            layers.append(nn.Conv2d(cin, width, kernel_size=3, padding=1))
            if batch_norm:
                layers.append(nn.BatchNorm2d(width))
            layers.append(nn.ReLU(inplace=True))
            cin = width
        layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    return nn.Sequential(*layers)


class _Net(nn.Module):
    """the children of torchvision's VGG, in its order"""

    def __init__(self, depth, batch_norm):
        super().__init__()
        self.features = _features(depth, batch_norm)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        # torchvision's classifier without its last Linear (reference vgg.py:33-36)
        self.classifier = nn.Sequential(nn.Linear(512 * 7 * 7, 4096), nn.ReLU(inplace=True), nn.Dropout(),
                                        nn.Linear(4096, 4096), nn.ReLU(inplace=True), nn.Dropout())


class VGG(OpsBackbone, nn.Module):
    _chunk_frames = None      # tests: force the frames per chunk of the eval / no_grad forward (None: the 2 GiB rule)

    def __init__(self, model_type, modality, in_channels, state_dict=None):
        """`state_dict`: torchvision vgg weights (`features.0.weight`, `classifier.0.weight`, ...; `classifier.6.*` is
        ignored) standing in for the reference's `pretrained=True` download; None -> torchvision's random initialisation."""
        super().__init__()
        model_type = str(model_type)
        if model_type not in _MODEL_TYPES:
            raise ValueError(f"VGG: model_type {model_type!r} is not one of {list(_MODEL_TYPES)} "
                             "(reference core/models/vgg.py:15-22)")
        self.model_type, self.modality, self.in_channels = model_type, modality, in_channels
        self.batch_norm = model_type.endswith("bn")
        self.model = _Net(model_type[:2], self.batch_norm)
        for m in self.modules():      # torchvision's VGG.__init__
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)
        if state_dict is not None:
            own = {"model." + k: v for k, v in state_dict.items() if not k.startswith("classifier.6.")}
            self.load_state_dict(own, strict=True)
        if modality != "RGB":
            # reference vgg.py:24-31: a FRESH first convolution with PyTorch's default initialisation (not the mean of the
            # RGB filters, unlike the ResNet)
            self.model.features[0] = nn.Conv2d(in_channels, 64, kernel_size=3, stride=1, padding=1)
        self.feature_size = self.model.classifier[3].out_features      # in_features of the removed Linear (vgg.py:33)

    # ---- forward
    def _units(self):
        """[(conv, bn or None, a pool follows)] in order"""
        mods = list(self.model.features)
        units = []
        for i, m in enumerate(mods):
            if isinstance(m, nn.Conv2d):
                bn = mods[i + 1] if isinstance(mods[i + 1], nn.BatchNorm2d) else None
                after = i + (3 if bn is not None else 2)
                units.append((m, bn, isinstance(mods[after], nn.MaxPool2d)))
        return units

    def _features_fwd(self, frames):
        x = None
        for conv, bn, pooled in self._units():
            if bn is None:
                # the pool's backward carries this unit's ReLU mask
                if x is None:
                    x = ops_conv.first_conv3(frames, conv.weight, conv.bias, state=unit_state(conv), relu_in_pool=pooled,
                                             who="VGG")
                else:
                    x = ops_conv.conv_bias_act(x, conv.weight, conv.bias, 1, 1, relu=True, relu_in_pool=pooled,
                                               state=unit_state(conv))
            elif x is None:
                x = ops_conv.first_conv3(frames, conv.weight, conv.bias, bn.weight, bn.bias, state=unit_state(conv, bn),
                                         training=bn.training, who="VGG")
                count_batch(bn.training, bn)
            else:
                x = conv_bn_relu(conv, bn, x, bn.training)
            if pooled:
                x = ops_conv.maxpool2(x, relu_gate=bn is None)
        return x

    def _forward(self, frames):
        x = ops_conv.adaptive_avgpool7_flat(self._features_fwd(frames))
        cls = self.model.classifier
        for lin, drop in ((cls[0], cls[2]), (cls[3], cls[5])):
            x = ops.linear(x, lin.weight, lin.bias, relu=True)
            x = ops.dropout(x, drop.p, drop.training)
        return x

    def forward(self, input):
        """(frames, C, H, W) -> (frames, 4096), as reference vgg.py:38-41"""
        if input.dim() != 4 or input.shape[2] < _MIN_SIZE or input.shape[3] < _MIN_SIZE:
            raise ValueError(f"VGG: input {tuple(input.shape)} is smaller than {_MIN_SIZE} x {_MIN_SIZE}: the five "
                             "MaxPool2d(2, 2) of the features halve the map five times and would leave nothing")
        self._need_gpu(input)
        n, _, h, w = input.shape
        if not self.training and not torch.is_grad_enabled():
            # eval has no cross-frame operation: walking the frames in chunks is exact.  The largest operand of a chunk is
            # the 64-channel map at full resolution; it has to stay below the convolution entries' 2 GiB limit.
            chunk = self._chunk_frames or max(1, _OPERAND_LIMIT // (h * w * 64 * 4))
            if n > chunk:
                return torch.cat([self._forward(input[i:i + chunk]) for i in range(0, n, chunk)])
        return self._forward(input)
