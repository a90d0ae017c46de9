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


# plane-product census: hi / mid / lo of the baseline are all populated, each perturbation moves exactly one plane
X0 = 1 + 2.0 ** -9 + 2.0 ** -19
D = [2.0 ** -3, 3 * 2.0 ** -11, 3 * 2.0 ** -21]
PAIRS = [(i, j) for i in range(3) for j in range(3)]


def kept(i, j, nprod):
    """does bf16x6 (nprod 6) / bf16x3 (nprod 3) compute the product of plane i of x with plane j of w"""
    return i + j <= (2 if nprod == 6 else 1)


def isolate_problem(i, j, n, h, w, cin, cout, k, seed=3):
    """inputs on which every plane product cancels exactly except (plane i of x) * (plane j of w): cancel_problem with a
    period-4 channel pattern.  With c4 = channel % 4: x_c = X0 + e * D[i], e = [1, 1, 0, 0][c4], at every pixel;
    w_oc = r_o * s * (X0 + f * D[j]), f = [1, 0, 1, 0][c4], s = [+1, -1, -1, +1][c4], at every tap; r_o = 2^randint(-3, 3).
    Over four channels sum s = sum s e = sum s f = 0 and sum s e f = 1, so plane product (p, q) sums to
    r_o (x_p(1) - x_p(0)) (w_q(1) - w_q(0)): zero unless (p, q) == (i, j), where it is r_o D[i] D[j].
    k = 1 (pad 0) | 3 (pad 1).  Returns x (NCHW), wt (OIHW), the exact output (fp64, NCHW)."""
    assert k in (1, 3) and cin % 4 == 0
    e = torch.tensor([1.0, 1.0, 0.0, 0.0]).repeat(cin // 4)
    f = torch.tensor([1.0, 0.0, 1.0, 0.0]).repeat(cin // 4)
    s = torch.tensor([1.0, -1.0, -1.0, 1.0]).repeat(cin // 4)
    x = (X0 + e * D[i]).float().view(1, cin, 1, 1).expand(n, cin, h, w).contiguous()
    r = 2.0 ** torch.randint(-3, 3, (cout,), generator=torch.Generator().manual_seed(seed)).float()
    wt = (r.view(-1, 1) * (s * (X0 + f * D[j])).float().view(1, -1)).view(cout, cin, 1, 1).expand(cout, cin, k, k).contiguous()
    ones = torch.ones(1, 1, h, w, dtype=torch.float64)
    taps = F.conv2d(ones, torch.ones(1, 1, k, k, dtype=torch.float64), padding=k // 2)
    want = r.double().view(1, -1, 1, 1) * (D[i] * D[j] * (cin // 4)) * taps
    return x, wt, want.expand(n, cout, h, w).contiguous()
