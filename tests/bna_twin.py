"""Plain-torch.nn twin of BNInception_Audio (the BN-Inception trunk behind the 1x3 / 3x1 audio stem): the oracle of the
gradient tests.  Everything is ordinary nn.Conv2d / nn.BatchNorm2d / F.relu / F.max_pool2d / F.avg_pool2d.

The layers come from a table: every conv's channel counts and kernel are read off its weight's shape in
tests/golden/bna_keys.json (the reference class's state-dict keys, in order), padding is kernel // 2, the stride is 2 for the
two stem convs and for the `_3x3` / `_double_3x3_2` convs of the two reduction blocks and 1 elsewhere.  The dataflow is the
ten-row block table below.  Modules are registered in the order of the keys, so the state dict is key-compatible with the
product class."""
import json
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

KEYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bna_keys.json")
# (block, what its fourth branch does): avg = AvgPool(3, 1, 1) -> pool_proj, max = MaxPool(3, 1, 1) -> pool_proj,
# pass = MaxPool(3, 2, ceil) concatenated as it is (the reduction blocks: no 1x1 branch, stride-2 3x3 convs)
BLOCKS = (("3a", "avg"), ("3b", "avg"), ("3c", "pass"), ("4a", "avg"), ("4b", "avg"), ("4c", "avg"), ("4d", "avg"),
          ("4e", "pass"), ("5a", "avg"), ("5b", "max"))
STEM = ("conv1_1x3_s2", "conv1_3x1_s2")


def _stride(name):
    if name in STEM:
        return 2
    reduction = tuple("inception_" + b for b, kind in BLOCKS if kind == "pass")
    return 2 if name.startswith(reduction) and name.endswith(("_3x3", "_double_3x3_2")) else 1


class TwinBNA(nn.Module):
    def __init__(self, attend=False):
        super().__init__()
        self.attend = attend
        with open(KEYS) as f:
            keys = json.load(f)
        for key, shape in keys:
            if key.endswith(".weight") and len(shape) == 4:
                name = key[:-len(".weight")]
                cout, cin, kh, kw = shape
                setattr(self, name, nn.Conv2d(cin, cout, (kh, kw), stride=_stride(name), padding=(kh // 2, kw // 2)))
                setattr(self, name + "_bn", nn.BatchNorm2d(cout))
            elif key == "last_linear.weight":
                self.last_linear = nn.Linear(shape[1], shape[0])

    def unit(self, name, x):
        return F.relu(getattr(self, name + "_bn")(getattr(self, name)(x)))

    def pool1(self, x):
        return F.max_pool2d(torch.cat([self.unit(n, x) for n in STEM], 1), 3, 2, ceil_mode=True)

    def features(self, x):
        x = self.pool1(x)
        x = F.max_pool2d(self.unit("conv2_3x3", self.unit("conv2_3x3_reduce", x)), 3, 2, ceil_mode=True)
        for b, kind in BLOCKS:
            p = "inception_" + b
            outs = [self.unit(p + "_1x1", x)] if hasattr(self, p + "_1x1") else []
            outs.append(self.unit(p + "_3x3", self.unit(p + "_3x3_reduce", x)))
            outs.append(self.unit(p + "_double_3x3_2", self.unit(p + "_double_3x3_1", self.unit(p + "_double_3x3_reduce", x))))
            if kind == "pass":
                outs.append(F.max_pool2d(x, 3, 2, ceil_mode=True))
            else:
                pooled = F.avg_pool2d(x, 3, 1, 1, count_include_pad=True) if kind == "avg" else F.max_pool2d(x, 3, 1, 1)
                outs.append(self.unit(p + "_pool_proj", pooled))
            x = torch.cat(outs, 1)
        return x

    def logits(self, feat):
        if self.attend:
            return feat.mean(2, keepdim=True)           # (n, 1024, 1, w')
        return feat.mean((2, 3))

    def forward(self, x):
        return self.logits(self.features(x))


def randomize(module, seed):
    """every parameter and running statistic away from its initial value, in place, the same for a given seed whatever the
    dtype of the module: conv weights fan-in scaled, conv bias / BN bias / running mean small, BN weight and running variance
    in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                fan = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5)
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g, dtype=torch.float64))
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64))
                m.bias.copy_(0.2 * torch.randn(c, generator=g, dtype=torch.float64))
                m.running_mean.copy_(0.2 * torch.randn(c, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64))
    return module
