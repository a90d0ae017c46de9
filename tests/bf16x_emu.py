"""fp32 torch emulation of the split-bf16 convolution math (attention_based_tbn_amd/csrc/conv_bf16x.hip): the exact
three-plane split and the plane products with i + j <= 2 (bf16x6) / <= 1 (bf16x3) summed in fp32, small products first."""
import torch
import torch.nn.functional as F

CASES = [(2, 14, 14, 64, 96), (3, 7, 7, 192, 320), (2, 9, 11, 32, 160), (1, 28, 28, 64, 64), (2, 28, 28, 192, 96),
         (1, 56, 56, 64, 192)]
# per product: bf16x3 drops lo*hi, hi*lo (2^-17 each, relative) and mid*mid (2^-18) and smaller
X3_REL = 1.25 * 2.0 ** -16
# fp32 accumulation of the MFMA against fp64 at K <= 4096: 3.5e-7 of sum |a b|, rounded up
ACC_REL = 4e-7


def split(x):
    """hi, mid, lo bf16 planes (as fp32 tensors) with hi + mid + lo == x"""
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return [hi, mid, lo]


def conv_emulated(x, w, nprod):
    """3x3 / stride 1 / pad 1 convolution of NCHW x with OIHW w from the bf16 planes (nprod = 6 | 3)"""
    xs, ws = split(x), split(w)
    limit = 2 if nprod == 6 else 1
    order = sorted([(i, j) for i in range(3) for j in range(3) if i + j <= limit], key=lambda t: -(t[0] + t[1]))
    y = None
    for i, j in order:
        t = F.conv2d(xs[i], ws[j], None, padding=1)
        y = t if y is None else y + t
    return y


def abs_conv(x, w):
    """|x| conv |w| in fp64: the scale of the element-wise error bounds"""
    return F.conv2d(x.double().abs(), w.double().abs(), None, padding=1)


def cancel_problem(n, h, w, cin, cout, seed=3):
    """inputs whose bf16x3 products cancel exactly while a dropped one survives (tests: `drops the planes`):
    returns x (NCHW), wt (OIHW), expected full product (fp64, NCHW)"""
    x = torch.full((n, cin, h, w), 1 + 2.0 ** -9)
    x[:, 0::2] += 7 * 2.0 ** -20
    c = 2.0 ** torch.randint(-3, 3, (cout,), generator=torch.Generator().manual_seed(seed)).float()
    wt = torch.empty(cout, cin, 3, 3)
    wt[:, 0::2] = c.view(-1, 1, 1, 1)
    wt[:, 1::2] = -c.view(-1, 1, 1, 1)
    taps = F.conv2d(torch.ones(1, 1, h, w, dtype=torch.float64), torch.ones(1, 1, 3, 3, dtype=torch.float64), padding=1)
    want = c.double().view(1, -1, 1, 1) * (7 * 2.0 ** -20) * (cin // 2) * taps
    return x, wt, want.expand(n, cout, h, w).contiguous()
