"""Case tables, data generators, float64 references and the comparison rules of the forward / data-gradient operator tests
(CPU only: imported by tests/test_conv_plan_cpu.py, which proves on the host that every table row reaches the mechanism it
names and that the comparison rejects what the old yardstick accepted, and by tests/test_conv_ops_gpu.py, which runs them).

    y[n][oy][ox][co]  = sum over (r, s, ci) of x[n][oy * stride + r - pad][ox * stride + s - pad][ci] * w[co][r][s][ci]
    dx[n][iy][ix][ci] = sum over (r, s, co) and the output pixels with oy * stride + r - pad == iy, ox * stride + s - pad == ix
                        of dy[n][oy][ox][co] * w[co][r][s][ci]

x, y, dy, dx are NHWC, w is [cout][k][k][cin]; taps outside the image contribute nothing.

EXACT DATA.  x and dy hold integers in [-4, 4]; w[co][r][s][ci] an integer in [-4, 4] times 2^(co % 5 - 2) * 2^(ci % 5 - 2).  For
one output element (fixed co for y, fixed ci for dx) every product is an integer multiple of ONE power-of-two unit
(2^(co % 5 - 4) resp. 2^(ci % 5 - 4)) of at most 4 * 4 * 16 = 256 units, so every partial sum of K terms, in any order, is an
integer of at most 256 K units: exact in fp32 while 256 K <= 2^24 (K = k * k * cin, or k * k * cout for a data gradient).
Bias, accumulation base and eval shift are integers in [-4, 4] times 4 units, the eval scale a power of two: at most
EXTRA_UNITS more.  Such cases are compared with torch.equal against the float64 reference rounded to fp32 -- every family,
tile and stage count must return the same bits.

FLOAT DATA.  Gaussian dy, x = relu(N(0.5, 1)), Gaussian w / sqrt(K), with the per-channel scales s(c) = 2^(c % 11 - 5) of
wgrad_check.channel_scale: x * s(ci), dy / s(co), w * s(co) / s(ci), so that y is of scale s(co), dx of scale 1 / s(ci) and the
terms of one element are balanced over its K.  Judged element by element against A = |x| conv |w|, the sum of the absolute
products of that element:  |got - ref| <= TOL * A.  A small-magnitude channel is held to its own scale.

TOL.  The project's fp32-accumulation constant is tests/bf16x_emu.py ACC_REL: 3.5e-7 of the absolute sum at K <= 4096, for
the order in which the MFMA chain sums.  A SEQUENTIAL fp32 sum of the first float case's own products, emulated on the CPU
against float64 (measure_reference_error() below; tests/test_conv_plan_cpu.py re-measures a channel subset), gives
                                                               worst order        the kernels' K order
    forward        (2, 13, 11) 3x3, 96 -> 160, K =  864:       1.11e-6 of A       2.7e-7 of A
    data gradient  (2, 13, 11) 3x3, 96 <- 160, K = 1440:       1.51e-6 of A       2.3e-7 of A
worst order = every element's terms sorted descending: the accumulator is at its largest while the small terms arrive.  The
K-order figures agree with ACC_REL.  The kernels sum in yet another order (four k groups per MFMA chain, split-K adds one
more rounding level), hence a factor-4 margin on the measured worst-order maximum:
    TOL = 4 * 1.51e-6 = 6.0e-6 of A
-- 22 times above the K-order error, and per ELEMENT against its own absolute sum, where the older tests' yardstick is 1e-4
of the tensor's maximum whatever the element's channel.

Sums over pixels formed in an epilogue (BN statistics, BN-backward reduce) are judged per channel against their own absolute
sums; their bounds are derived at stat_bounds / reduce_reference.
"""
import numpy as np
import torch
import torch.nn.functional as F

TOL = 6.0e-6
EXTRA_UNITS = 64          # bias + accumulation base + eval shift: 16 units each, with room
HALO, DMA, SK4 = 4, 8, 16  # tbn_conv_desc flags of the kernel families (0: the generic 1- / 2-stage kernel)

# (n, h, w, k, stride, pad): the smallest maps at which each mechanism of the forward / data-gradient address arithmetic exists
GEOMS = [
    (1, 5, 5, 3, 1, 1),       # M = 25: below one 32-row split-K tile
    (2, 7, 7, 3, 1, 1),       # M = 98: below one 128-row tile, ragged against the split-K tile's 32 and 64 rows
    (2, 13, 11, 3, 1, 1),     # M = 286 = 2 * 128 + 30 = 256 + 30: ragged against 128 and 256
    (5, 3, 3, 3, 1, 1),       # frames of 9 pixels: frame boundaries inside every tile
    (3, 5, 3, 3, 1, 1),       # frames of 15 pixels, 5x3
    (3, 9, 1, 3, 1, 1),       # OW == 1: narrower than the halo's W + 1 reach, no left / right tap ever inside
    (4, 1, 9, 3, 1, 1),       # OH == 1: the halo's W + 1 = 10 pixels reach past a whole frame on both sides
    (70, 1, 1, 3, 1, 1),      # OH * OW == 1: every row its own frame, only the centre tap inside
    (1, 2, 64, 3, 1, 1),      # width 64: the halo limit
    (1, 2, 65, 3, 1, 1),      # width 65: refused by the halo family, run by the others
    (2, 8, 9, 3, 1, 0),       # 3x3 / stride 1 / pad 0 (the data gradient pads by 2)
    (2, 6, 5, 3, 1, 2),       # 3x3 / stride 1 / pad 2 (the data gradient pads by 0)
    (3, 9, 11, 1, 1, 0),      # 1x1 / stride 1: the pointwise row decode, M = 297
    (3, 9, 3, 3, 1, 0),       # valid 3x3 down to a one-column output (OW == 1 forward, W == 1 for the data gradient)
    (2, 9, 6, 3, 2, 0),       # stride 2 / pad 0, odd x even: parities 5x3 | 4x3; the last column is read by no output pixel
    (2, 9, 6, 3, 2, 1),       # stride 2 / pad 1, odd x even
    (2, 9, 6, 3, 2, 2),       # stride 2 / pad 2, odd x even
    (2, 9, 6, 1, 2, 0),       # 1x1 / stride 2 (the ResNet downsample): three parities with pixels and no tap
    (2, 8, 6, 3, 2, 0),       # stride 2 / pad 0, even x even: the last row AND column are read by no output pixel
    (3, 1, 8, 3, 2, 1),       # one-row map: two parities have no pixels (pad 1)
    (3, 1, 8, 3, 2, 2),       # one-row map, pad 2
    (3, 1, 8, 1, 2, 0),       # one-row map, 1x1 / stride 2: one phase launches
    (3, 7, 1, 3, 2, 1),       # one-column map: OW == 1 under stride 2
    (3, 17, 13, 3, 2, 1),     # odd x odd: four parities of four sizes (9x7, 9x6, 8x7, 8x6), two M tiles in the largest
    (3, 17, 13, 1, 2, 0),     # the same map for the downsample: two M tiles in the phase that launches
]
# (cin, cout); the N extent is cout forward, cin for the data gradient: 32 is ragged under nt = 2, 3, 4; 64 under 3 and 4;
# 96 under 2 and 4; 160 under 2, 3 and 4 (and full tiles exist under every nt)
CHANNELS = [(32, 32), (64, 96), (96, 160)]
# cin 32 at 1x1: K is ONE 32-float chunk for the split-K tile kernel's four waves (three waves idle); cin 64 at 1x1: two
SHORT_K = [((3, 9, 11, 1, 1, 0), 32, 32), ((3, 9, 11, 1, 1, 0), 64, 96)]
# every geometry at one channel pair (in rotation), the short-K cases, and the widest pair on the ragged and the largest map
EXACT_CASES = [(g, ) + CHANNELS[i % 3] for i, g in enumerate(GEOMS)]
EXACT_CASES += [c for c in SHORT_K if c not in EXACT_CASES]
EXACT_CASES += [c for c in (((2, 13, 11, 3, 1, 1), 32, 32), ((2, 13, 11, 3, 1, 1), 64, 96), ((3, 17, 13, 3, 2, 1), 96, 160),
                            ((3, 17, 13, 1, 2, 0), 96, 160), ((2, 9, 6, 1, 2, 0), 64, 96)) if c not in EXACT_CASES]
FLOAT_CASES = [((2, 13, 11, 3, 1, 1), 96, 160), ((3, 9, 11, 1, 1, 0), 96, 160), ((3, 17, 13, 3, 2, 1), 96, 160)]
# the pair launch: two members on one map with different channel counts
PAIR_CASE = ((2, 13, 11, 3, 1, 1), (32, 96), (64, 32))


def case_id(case):
    g, cin, cout = case
    return "n%d_%dx%d_k%ds%dp%d-ci%d_co%d" % (g + (cin, cout))


def out_hw(geom):
    n, h, w, k, stride, pad = geom
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def rows(geom, dgrad):
    """GEMM rows of the launch: output pixels of the forward pass, INPUT pixels of the data gradient"""
    n, h, w = geom[:3]
    oh, ow = out_hw(geom)
    return n * h * w if dgrad else n * oh * ow


def k_terms(geom, cin, cout, dgrad):
    return geom[3] * geom[3] * (cout if dgrad else cin)


def channel_scale(c):
    """2^(c mod 11 - 5) per channel: three decades, exact in every float format (wgrad_check.channel_scale)"""
    return np.ldexp(1.0, np.arange(c) % 11 - 5)


def unit_scale(c):
    """2^(c mod 5 - 2): the power-of-two factor of the exact weights along one channel axis"""
    return np.ldexp(1.0, np.arange(c) % 5 - 2)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def exact_case(geom, cin, cout, seed):
    """dict of float32 tensors: x (n, h, w, cin), dy (n, oh, ow, cout), w (cout, k, k, cin), and per output channel of the
    forward pass bias, base (accumulation start, (n, oh, ow, cout)), scale / shift (eval epilogue); dbase (n, h, w, cin) the
    accumulation start of the data gradient.  See the module docstring for why every sum is exact."""
    n, h, w, k, stride, pad = geom
    oh, ow = out_hw(geom)
    rng = np.random.default_rng(seed)

    def ints(*shape):
        return rng.integers(-4, 5, size=shape).astype(np.float64)
    uo, ui = unit_scale(cout), unit_scale(cin)
    d = {"x": ints(n, h, w, cin), "dy": ints(n, oh, ow, cout),
         "w": ints(cout, k, k, cin) * uo[:, None, None, None] * ui}
    d["bias"] = ints(cout) * uo                      # 4 units of 2^(co % 5 - 4) each step
    d["base"] = ints(n, oh, ow, cout) * uo
    d["dbase"] = ints(n, h, w, cin) * ui
    d["scale"] = np.ldexp(1.0, np.arange(cout) % 3 - 1)          # 1/2, 1, 2: the product v * scale is exact
    d["shift"] = ints(cout) * uo * d["scale"]                      # a multiple of the scaled unit
    return {key: _t(v) for key, v in d.items()}


def float_case(geom, cin, cout, seed):
    """x = relu(N(0.5, 1)) * scale(ci), dy = Gaussian / scale(co), w = Gaussian / sqrt(k k cin) * scale(co) / scale(ci): the
    terms of one element are balanced over its K in both directions, y is of scale(co) and dx of 1 / scale(ci)"""
    n, h, w, k, stride, pad = geom
    oh, ow = out_hw(geom)
    rng = np.random.default_rng(seed)
    so, si = channel_scale(cout), channel_scale(cin)
    d = {"x": np.maximum(rng.standard_normal((n, h, w, cin)) + 0.5, 0.0) * si,
         "dy": rng.standard_normal((n, oh, ow, cout)) / so,
         "w": rng.standard_normal((cout, k, k, cin)) / np.sqrt(k * k * cin) * so[:, None, None, None] / si}
    d["scale"] = (rng.random(cout) + 0.5) / so
    d["shift"] = rng.standard_normal(cout) * 0.3
    return {key: _t(v) for key, v in d.items()}


def _nchw(a):
    return a.permute(0, 3, 1, 2)


def forward_reference(x, w, geom):
    """y (n, oh, ow, cout) in float64: F.conv2d"""
    k, stride, pad = geom[3:]
    return F.conv2d(_nchw(x.double()), _nchw(w.double()), None, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def dgrad_reference(dy, w, geom):
    """dx (n, h, w, cin) in float64: the autograd of F.conv2d"""
    n, h, wd, k, stride, pad = geom
    xz = torch.zeros(n, w.shape[3], h, wd, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xz, _nchw(w.double()), None, stride=stride, padding=pad)
    (dx,) = torch.autograd.grad(y, xz, _nchw(dy.double()))
    return dx.permute(0, 2, 3, 1).contiguous()


def loop_forward(x, w, geom):
    """the forward sum pixel by pixel and tap by tap (tiny cases only): independent of torch's padding rules"""
    n, h, wd, k, stride, pad = geom
    oh, ow = out_hw(geom)
    x64, w64 = x.double().numpy(), w.double().numpy()
    y = np.zeros((n, oh, ow, w.shape[0]))
    for f in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for r in range(k):
                    for s in range(k):
                        iy, ix = oy * stride + r - pad, ox * stride + s - pad
                        if 0 <= iy < h and 0 <= ix < wd:
                            y[f, oy, ox] += w64[:, r, s, :] @ x64[f, iy, ix]
    return torch.from_numpy(y)


def loop_dgrad(dy, w, geom):
    """the data gradient as the scatter of every (output pixel, tap) pair onto the input pixel it read"""
    n, h, wd, k, stride, pad = geom
    oh, ow = out_hw(geom)
    dy64, w64 = dy.double().numpy(), w.double().numpy()
    dx = np.zeros((n, h, wd, w.shape[3]))
    for f in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for r in range(k):
                    for s in range(k):
                        iy, ix = oy * stride + r - pad, ox * stride + s - pad
                        if 0 <= iy < h and 0 <= ix < wd:
                            dx[f, iy, ix] += dy64[f, oy, ox] @ w64[:, r, s, :]
    return torch.from_numpy(dx)


def unread_pixels(geom):
    """(h, w) bool: input pixels no output pixel reads through any tap -- their data gradient is exactly 0"""
    n, h, wd, k, stride, pad = geom
    oh, ow = out_hw(geom)
    ry, rx = np.zeros(h, bool), np.zeros(wd, bool)
    for r in range(k):
        for o in range(oh):
            if 0 <= o * stride + r - pad < h:
                ry[o * stride + r - pad] = True
        for o in range(ow):
            if 0 <= o * stride + r - pad < wd:
                rx[o * stride + r - pad] = True
    return ~np.outer(ry, rx)


# ---- the comparison rules

def exact_ok(got, ref64):
    """bit-for-bit against the float64 reference rounded to fp32 (which loses nothing on exact data)"""
    return torch.equal(got.cpu(), ref64.float())


def float_ratio(got, ref64, a64, tol=TOL):
    """worst |got - ref| / (tol * A) over the elements (<= 1 passes); where A == 0 the element has no term and must be 0"""
    err = (got.double().cpu() - ref64).abs()
    if bool(((a64 == 0) & (err != 0)).any()):
        return float("inf")
    return float((err / (tol * a64).clamp_min(1e-300)).max())


def old_yardstick(got, ref64):
    """max |got - ref| / max |ref|: what tests/test_conv_variants_gpu.py asserts to be below 1e-4"""
    return float((got.double().cpu() - ref64).abs().max() / (ref64.abs().max() + 1e-30))


def stat_bounds(a64):
    """per-channel bounds of the BN-statistics partials s1 = sum y, s2 = sum y^2 over the pixels, summed in float64 over the
    partial rows, from A (pixels..., cout) = |x| conv |w|.  Every y carries at most TOL * A, and a row of at most 256 pixels
    is summed in fp32 behind the K loop (the same chain, so the same constant on sum |y| <= sum A):
        |s1 - ref| <= TOL * sum A + TOL * sum |y|                <= 2 TOL sum A
        |s2 - ref| <= sum (2 |y| TOL A + (TOL A)^2) + TOL sum y^2  <= 4 TOL sum A^2"""
    a = a64.reshape(-1, a64.shape[-1])
    return 2 * TOL * a.sum(0), 4 * TOL * (a * a).sum(0)


def reduce_inputs(pixels, c, seed):
    """yb (pixels, c): the BN inputs of the producer layers; stats (4, c) float32: mean, rstd, gamma * rstd, beta - mean * gamma
    * rstd (as tests/test_conv_variants_gpu.py Problem)"""
    gen = torch.Generator().manual_seed(seed)
    yb = torch.randn(pixels, c, generator=gen) * 1.5 + 0.2
    mean = yb.double().mean(0)
    rstd = 1.0 / (yb.double().var(0, unbiased=False) + 1e-5).sqrt()
    gamma = torch.rand(c, generator=gen).double() + 0.5
    beta = torch.randn(c, generator=gen).double() * 0.3
    return yb, torch.stack([mean, rstd, gamma * rstd, beta - mean * gamma * rstd]).float()


def reduce_reference(dz64, a64, yb, stats):
    """(s1, s2, b1, b2) per channel: s1 = sum g, s2 = sum g * xhat with g = dz where the producer's ReLU was open (the sign of
    y * scale + shift, exact in float64 and in the kernel's fmaf alike), xhat = (y - mean) * rstd.
    Bounds, with Ag = A where the ReLU was open (|g| <= Ag) and X = (|y| + |mean|) * rstd >= |xhat|: the kernel's xhat carries
    two fp32 roundings of terms of at most X (2^-23 X <= TOL X), g carries TOL * A, the sum over at most 256 pixels TOL of its
    absolute sum:
        |s1 - ref| <= TOL sum Ag + TOL sum |g|                                   <= 2 TOL sum Ag
        |s2 - ref| <= sum (TOL Ag |xhat| + |g| TOL X) + TOL sum |g xhat|          <= 3 TOL sum Ag X"""
    st = stats.double()
    dz, a, y = dz64.reshape(yb.shape), a64.reshape(yb.shape), yb.double()
    mask = (y * st[2] + st[3]) > 0
    g, ag = dz * mask, a * mask
    xhat = (y - st[0]) * st[1]
    big = (y.abs() + st[0].abs()) * st[1]
    return g.sum(0), (g * xhat).sum(0), 2 * TOL * ag.sum(0), 3 * TOL * (ag * big).sum(0)


# ---- the launch rules restated (tests/test_conv_plan_cpu.py holds them against the built library)

def parity_taps(par, k, pad):
    """filter taps r of one axis that reach a real dy sample at the input pixels of parity `par` of a stride-2 data gradient
    (the launch pads by k - 1 - pad; conv_igemm.hip parity_tap): par - (k - 1 - pad) + r even"""
    return [r for r in range(k) if (par - (k - 1 - pad) + r) % 2 == 0]


def phases(geom):
    """the parity phases of the stride-2 data gradient of `geom`: dicts py, px, ohs, ows (pixels of that parity per frame),
    M (GEMM rows), taps, launches (pixels and taps)"""
    n, h, w, k, stride, pad = geom
    assert stride == 2
    out = []
    for py in range(2):
        for px in range(2):
            ohs, ows = (h - py + 1) // 2, (w - px + 1) // 2
            taps = len(parity_taps(py, k, pad)) * len(parity_taps(px, k, pad))
            out.append(dict(py=py, px=px, ohs=ohs, ows=ows, M=n * ohs * ows, taps=taps,
                            launches=ohs > 0 and ows > 0 and taps > 0))
    return out


def rows_written(geom, dgrad, tile_rows):
    """partial rows (M tiles) the launch writes: one per tile of the GEMM, for a strided data gradient one per tile of
    every phase that launches"""
    if dgrad and geom[4] == 2:
        return sum(-(-p["M"] // tile_rows) for p in phases(geom) if p["launches"])
    return -(-rows(geom, dgrad) // tile_rows)


def frame_boundaries_in_tile(geom, dgrad, tile_rows):
    """GEMM rows m, not tile starts, at which a new frame begins"""
    per = rows(geom, dgrad) // geom[0]
    return [m for m in range(per, rows(geom, dgrad), per) if m % tile_rows]


# ---- the reference's own fp32 error (TOL)

def dgrad_as_forward(dy, w, geom):
    """(xz, wf, geom_f): the data gradient as a unit-stride forward convolution of the zero-inserted, padded dy with the
    tap-flipped, channel-transposed weights (the inserted zeros add terms of exactly 0)"""
    n, h, wd, k, stride, pad = geom
    oh, ow = out_hw(geom)
    z = torch.zeros(n, (oh - 1) * stride + 1, (ow - 1) * stride + 1, dy.shape[3], dtype=dy.dtype)
    z[:, ::stride, ::stride] = dy
    q = k - 1 - pad
    bottom, right = h + k - 1 - q - z.shape[1], wd + k - 1 - q - z.shape[2]
    z = F.pad(z, (0, 0, q, right, q, bottom))
    wf = w.flip(1, 2).permute(3, 1, 2, 0).contiguous()
    return z, wf, (n, z.shape[1], z.shape[2], k, 1, 0)


def emulated_fp32(x, w, geom, order, channels):
    """(emu, ref, A) over the output channels `channels`: a SEQUENTIAL fp32 sum of the exact products (each step rounds the
    exact acc + product once, as an fma chain does), in the kernels' K order ("k") or with every element's terms sorted
    descending ("worst"), next to the float64 sum and the absolute sum"""
    k, stride, pad = geom[3:]
    cols = F.unfold(_nchw(x.double()), k, padding=pad, stride=stride)                    # (n, cin k k, L)
    cols = cols.permute(0, 2, 1).reshape(-1, cols.shape[1])                               # (M, K)
    wk = _nchw(w.double()).reshape(w.shape[0], -1)[channels]                              # (c, K) in unfold's (ci, r, s) order
    terms = cols[:, None, :] * wk[None]                                                   # (M, c, K): exact in float64
    if order == "worst":
        terms = terms.sort(dim=2, descending=True).values
    acc = torch.zeros(terms.shape[:2], dtype=torch.float32)
    for i in range(terms.shape[2]):
        acc = (acc.double() + terms[..., i]).float()
    return acc, terms.sum(2), terms.abs().sum(2)


def measure_reference_error(order, channels=None):
    """{"forward": e, "dgrad": e}: the worst |emulated fp32 - float64| / A of the first FLOAT_CASES geometry"""
    g, cin, cout = FLOAT_CASES[0]
    d = float_case(g, cin, cout, seed=7)
    out = {}
    emu, ref, a = emulated_fp32(d["x"], d["w"], g, order, list(range(cout)) if channels is None else channels)
    out["forward"] = float(((emu.double() - ref).abs() / a).max())
    z, wf, gf = dgrad_as_forward(d["dy"], d["w"], g)
    emu, ref, a = emulated_fp32(z, wf, gf, order, list(range(cin)) if channels is None else channels)
    out["dgrad"] = float(((emu.double() - ref).abs() / a).max())
    return out
