"""Plain-torch.nn twin of torchvision's vgg11 / vgg11_bn / vgg16 / vgg16_bn, wrapped as reference core/models/vgg.py wraps
them (the first conv replaced for a modality other than RGB, the classifier's last Linear removed): the oracle of the VGG
tests.  Written out here because torchvision is not a dependency of the project.  Everything is ordinary nn.Conv2d /
nn.BatchNorm2d / nn.MaxPool2d / nn.Linear; it runs in float32 or float64 alike.

The layer table, in words: all convolutions are 3x3 with padding 1 and a bias, each followed by ReLU (with BatchNorm2d in
between in the `bn` types); a 2x2 / stride 2 max pool closes each of five stages of widths 64, 128, 256, 512, 512; the stages
hold 1, 1, 2, 2, 2 convolutions in the 11-layer type and 2, 2, 3, 3, 3 in the 16-layer type."""
import torch
import torch.nn as nn

WIDTHS = (64, 128, 256, 512, 512)
CONVS = {"11": (1, 1, 2, 2, 2), "16": (2, 2, 3, 3, 3)}
KEY_COUNTS = {"16": 30, "16bn": 95, "11": 20, "11bn": 60}


class TwinNet(nn.Module):
    def __init__(self, model_type, in_channels):
        super().__init__()
        bn = model_type.endswith("bn")
        layers, cin = [], in_channels
        for width, count in zip(WIDTHS, CONVS[model_type[:2]]):
            for _ in range(count):
                layers.append(nn.Conv2d(cin, width, 3, padding=1))
                if bn:
                    layers.append(nn.BatchNorm2d(width))
                layers.append(nn.ReLU())
                cin = width
            layers.append(nn.MaxPool2d(2, 2))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(nn.Linear(25088, 4096), nn.ReLU(), nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(),
                                        nn.Dropout())

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


class TwinVGG(nn.Module):
    def __init__(self, model_type, in_channels=3):
        super().__init__()
        self.model = TwinNet(str(model_type), in_channels)
        self.feature_size = 4096

    def forward(self, x):
        feat = self.model(x)
        return feat.view(feat.size(0), -1)


def randomize(module, seed, gain=1.0):
    """every parameter and running statistic away from its initial value, in place, the same for a given seed whatever the
    dtype / device of the module: conv / linear weights fan-in scaled (He), their biases small, BN weight in [0.5, 1.5] *
    gain, BN bias / running mean small, running variance in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g, dtype=torch.float64))
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
