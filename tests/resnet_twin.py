"""Plain-torch.nn twin of torchvision's resnet{18,34,50,101,152} without `fc`, wrapped as reference core/models/resnet.py
wraps it (`self.model = nn.Sequential(*children[:-1])`): the oracle of the ResNet tests.  Written out here because
torchvision is not a dependency of the project.  Everything is ordinary nn.Conv2d / nn.BatchNorm2d / F.relu."""
import torch
import torch.nn as nn

COUNTS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}


def conv(cin, cout, k, stride):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)


class TwinBlock(nn.Module):
    def _shortcut(self, cin, cout, stride):
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))


class TwinBasicBlock(TwinBlock):
    expansion = 1

    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = conv(cin, width, 3, stride), nn.BatchNorm2d(width)
        self.relu = nn.ReLU()
        self.conv2, self.bn2 = conv(width, width, 3, 1), nn.BatchNorm2d(width)
        self._shortcut(cin, width, stride)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class TwinBottleneck(TwinBlock):
    expansion = 4

    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = conv(cin, width, 1, 1), nn.BatchNorm2d(width)
        self.conv2, self.bn2 = conv(width, width, 3, stride), nn.BatchNorm2d(width)
        self.conv3, self.bn3 = conv(width, 4 * width, 1, 1), nn.BatchNorm2d(4 * width)
        self.relu = nn.ReLU()
        self._shortcut(cin, 4 * width, stride)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class TwinResnet(nn.Module):
    def __init__(self, depth, in_channels=3):
        super().__init__()
        block = TwinBasicBlock if depth in (18, 34) else TwinBottleneck
        layers, cin = [], 64
        for i, (width, n) in enumerate(zip((64, 128, 256, 512), COUNTS[depth])):
            blocks = []
            for b in range(n):
                blocks.append(block(cin, width, 2 if (i > 0 and b == 0) else 1))
                cin = width * block.expansion
            layers.append(nn.Sequential(*blocks))
        self.feature_size = cin
        self.model = nn.Sequential(conv(in_channels, 64, 7, 2), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
                                   *layers, nn.AdaptiveAvgPool2d((1, 1)))

    def forward(self, x):
        return self.model(x).flatten(1)


def randomize(module, seed, gain=1.0):
    """every parameter and running statistic away from its initial value, in place, the same for a given seed whatever the
    dtype / device of the module: conv weights fan-in scaled, BN weight in [0.5, 1.5] * gain, bias / running mean small,
    running variance in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                fan = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_((0.5 + torch.rand(c, generator=g, dtype=torch.float64)) * gain)
                m.bias.copy_(0.2 * torch.randn(c, generator=g, dtype=torch.float64))
                m.running_mean.copy_(0.2 * torch.randn(c, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64))
    return module


def rel_err(got, want):
    """max |got - want| relative to the tensor's max (the measure of tests/test_kernels_gpu.py)"""
    want = want.detach().double().cpu()
    got = got.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
