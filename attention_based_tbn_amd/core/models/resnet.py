"""ResNet backbones (model.arch = "resnet") composed from the stand-alone HIP operators.

API mirror of reference core/models/resnet.py:7-44: `Resnet(model_depth, modality, in_channels)`, `feature_size`,
`forward(frames) -> (frames, feature_size)`.  The graph is torchvision's resnet{18,34,50,101,152} without `fc`, spelled out
here; the children sit in `self.model = nn.Sequential(...)` exactly as the reference wraps them, so the state-dict names
are the reference's (`model.0.weight`, `model.1.running_mean`, `model.4.0.conv1.weight`, `model.5.0.downsample.1.bias`, ...)
and its checkpoints load with strict=True.

nn.Conv2d / nn.BatchNorm2d are used as PARAMETER CONTAINERS only: their forward is never called.  Every numerical op runs in
libtbn_hip.so through attention_based_tbn_amd.ops_conv -- the stem through tbn_stem_conv_* and the pooled BatchNorm, every
block as one autograd node of conv / BatchNorm / join launches, the global average pool through tbn_spatial_mean_*.  Unlike
BN-Inception this backbone does not go through the backbone engine (no plans, autotune, riders, bucketed gradient sync).
"""
import torch.nn as nn

from ... import ops_conv
from .ops_backbone import OpsBackbone, count_batch, unit_state

_DEPTHS = {
    18: ("basic", (2, 2, 2, 2)),
    34: ("basic", (3, 4, 6, 3)),
    50: ("bottleneck", (3, 4, 6, 3)),
    101: ("bottleneck", (3, 4, 23, 3)),
    152: ("bottleneck", (3, 8, 36, 3)),
}


def _conv(cin, cout, k, stride):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=False)


class _Block(nn.Module):
    def _downsample(self, cin, cout, stride):
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))

    def forward(self, x):
        """NHWC in, NHWC out"""
        pairs = [(getattr(self, "conv%d" % i), getattr(self, "bn%d" % i)) for i in range(1, self.units + 1)]
        if self.downsample is not None:
            pairs.append(tuple(self.downsample))
        units = [(conv.weight, bn.weight, bn.bias, unit_state(conv, bn)) for conv, bn in pairs]
        out = ops_conv.residual_block(x, units[:self.units], *units[self.units:], training=self.training)
        count_batch(self.training, *(bn for _, bn in pairs))
        return out


class BasicBlock(_Block):
    """conv3x3(stride) - bn - relu - conv3x3 - bn, + shortcut, relu"""
    expansion, units = 1, 2

    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = _conv(cin, width, 3, stride), nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2 = _conv(width, width, 3, 1), nn.BatchNorm2d(width)
        self._downsample(cin, width, stride)


class Bottleneck(_Block):
    """conv1x1 - bn - relu - conv3x3(stride) - bn - relu - conv1x1(x4) - bn, + shortcut, relu"""
    expansion, units = 4, 3

    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = _conv(cin, width, 1, 1), nn.BatchNorm2d(width)
        self.conv2, self.bn2 = _conv(width, width, 3, stride), nn.BatchNorm2d(width)
        self.conv3, self.bn3 = _conv(width, 4 * width, 1, 1), nn.BatchNorm2d(4 * width)
        self.relu = nn.ReLU(inplace=True)
        self._downsample(cin, 4 * width, stride)


class Resnet(OpsBackbone, nn.Module):
    def __init__(self, model_depth, modality, in_channels, state_dict=None):
        """`state_dict`: torchvision resnet weights (`conv1.weight`, `layer1.0.bn1.weight`, ...; an `fc.*` entry is
        ignored) standing in for the reference's `pretrained=True` download; None -> torchvision's random initialisation."""
        super().__init__()
        if model_depth not in _DEPTHS:
            raise ValueError(f"Resnet: model_depth {model_depth} is not one of {sorted(_DEPTHS)} "
                             "(reference core/models/resnet.py:15-24)")
        if modality != "RGB" and in_channels != 1:
            raise ValueError(f"Resnet: modality {modality} with {in_channels} input channels is not supported: reference "
                             "core/models/resnet.py:26-36 replaces conv1's weight by its mean over the input-channel axis, "
                             "shape (64, 1, 7, 7), while the new conv1 expects in_channels planes -- its forward raises a "
                             "shape error for every modality but Audio (1 channel)")
        kind, counts = _DEPTHS[model_depth]
        block = BasicBlock if kind == "basic" else Bottleneck
        layers, cin = [], 64
        for i, (width, n) in enumerate(zip((64, 128, 256, 512), counts)):
            blocks = []
            for b in range(n):
                blocks.append(block(cin, width, 2 if (i > 0 and b == 0) else 1))
                cin = width * block.expansion
            layers.append(nn.Sequential(*blocks))
        self.feature_size = cin
        self.modality, self.in_channels, self.model_depth = modality, in_channels, model_depth
        # children in torchvision's order without `fc` (reference resnet.py:39)
        self.model = nn.Sequential(_conv(3, 64, 7, 2), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
                                   nn.MaxPool2d(kernel_size=3, stride=2, padding=1), *layers, nn.AdaptiveAvgPool2d((1, 1)))
        for m in self.modules():      # torchvision's ResNet.__init__
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if state_dict is not None:
            self._load_torchvision(state_dict)
        if modality != "RGB":
            # reference resnet.py:26-36: the (pretrained) RGB filters averaged over the input-channel axis
            conv1 = self.model[0]
            weight = conv1.weight.detach().mean(dim=1).unsqueeze(dim=1)
            self.model[0] = _conv(in_channels, 64, 7, 2)
            self.model[0].weight = nn.Parameter(weight)

    def _load_torchvision(self, sd):
        names = {"conv1": "model.0", "bn1": "model.1", "layer1": "model.4", "layer2": "model.5", "layer3": "model.6",
                 "layer4": "model.7"}
        own = {}
        for k, v in sd.items():
            head, _, rest = k.partition(".")
            if head in names:
                own[names[head] + "." + rest] = v
        self.load_state_dict(own, strict=True)

    def forward(self, input):
        """(frames, C, H, W) -> (frames, feature_size), as reference resnet.py:41-44"""
        self._need_gpu(input)
        conv1, bn1 = self.model[0], self.model[1]
        x = ops_conv.stem_bn_pool(input, conv1.weight, bn1.weight, bn1.bias, unit_state(conv1, bn1), training=bn1.training,
                                  who="Resnet")
        count_batch(bn1.training, bn1)
        for i in range(4, 8):
            for blk in self.model[i]:
                x = blk(x)
        return ops_conv.global_mean(x)
