"""fp32 torch emulation of the pointwise (1x1 / stride 1 / pad 0) split-bf16 convolution on pre-split weight planes
(attention_based_tbn_amd/csrc/conv_bf16x.hip: conv_bf16x_pw_kernel, bf16x_split_planes_kernel), beside tests/bf16x_emu.py:
the same planes and plane products, a 1x1 cancellation problem, and the byte image of the weight-plane records."""
import torch
import torch.nn.functional as F

from tests.bf16x_emu import split

# (n, h, w, cin, cout): the merged 1x1 groups of inception_4d / 5a-like widths, short K, ragged maps, a second N-tile remainder
PW_CASES = [(2, 14, 14, 576, 512), (3, 7, 7, 1056, 832), (2, 9, 11, 32, 160), (1, 28, 28, 192, 224), (1, 56, 56, 64, 64),
            (2, 14, 14, 608, 320), (2, 7, 7, 1024, 832)]


def pw_emulated(x, w, nprod):
    """1x1 convolution of NCHW x with OIHW (cout, cin, 1, 1) w from the bf16 planes (nprod = 6 | 3), small products first"""
    xs, ws = split(x), split(w)
    limit = 2 if nprod == 6 else 1
    order = sorted([(i, j) for i in range(3) for j in range(3) if i + j <= limit], key=lambda t: -(t[0] + t[1]))
    y = None
    for i, j in order:
        t = F.conv2d(xs[i], ws[j], None)
        y = t if y is None else y + t
    return y


def pw_abs_conv(x, w):
    """|x| conv |w| in fp64: the scale of the element-wise error bounds"""
    return F.conv2d(x.double().abs(), w.double().abs(), None)


def pw_cancel_problem(n, h, w, cin, cout, seed=3):
    """1x1 inputs whose bf16x3 products (hi*hi, hi*mid, mid*hi) cancel exactly between even and odd input channels while the
    dropped lo*hi survives: returns x (NCHW), wt (cout, cin, 1, 1), expected full product (fp64, NCHW)"""
    x = torch.full((n, cin, h, w), 1 + 2.0 ** -9)
    x[:, 0::2] += 7 * 2.0 ** -20
    c = 2.0 ** torch.randint(-3, 3, (cout,), generator=torch.Generator().manual_seed(seed)).float()
    wt = torch.empty(cout, cin, 1, 1)
    wt[:, 0::2] = c.view(-1, 1, 1, 1)
    wt[:, 1::2] = -c.view(-1, 1, 1, 1)
    want = c.double().view(1, -1, 1, 1) * (7 * 2.0 ** -20) * (cin // 2)
    return x, wt, want.expand(n, cout, h, w).contiguous()


def plane_records(w_ohwi, nplanes):
    """the weight-plane records of an OHWI (cout, k, k, cin) fp32 tensor as int16 bf16 bit patterns, shape
    (cout * k * k * cin / 32, nplanes, 32): record r = the 32 consecutive weights from float index 32 r, plane by plane
    (include/tbn_hip.h tbn_conv_split_weights)"""
    planes = split(w_ohwi.contiguous().float())[:nplanes]
    recs = torch.stack([p.reshape(-1, 32).bfloat16().view(torch.int16) for p in planes], dim=1)
    return recs.contiguous()
