"""Case tables, data generators and float64 references of the weight-gradient operator tests (CPU only: imported by
tests/test_wgrad_plan_cpu.py, which checks on the host that the tables reach every kernel instantiation and address-arithmetic
edge, and by tests/test_wgrad_ops_gpu.py, which runs them).

    dW[co][r][s][ci] = sum over output pixels m = (n, oy, ox) of dy[m][co] * x[n][oy * stride + r - pad][ox * stride + s - pad][ci]

dy is NHWC (n, oh, ow, cout), x NHWC (n, h, w, cin); taps outside the image contribute nothing."""
import numpy as np
import torch
import torch.nn.functional as F

# the 11 instantiated tiles: (mt, nt) = 32-column sub-tiles of cout / cin per workgroup
TILES = [(mt, nt) for mt in (1, 2, 3, 5) for nt in (1, 2, 3) if (mt, nt) != (5, 3)]

# (n, h, w, k, stride, pad): the smallest maps at which each mechanism of the kernel's row arithmetic exists
GEOMS = [
    (2, 6, 6, 3, 1, 1),       # one ragged 64-row step
    (2, 13, 11, 3, 1, 1),     # M = 286: two splits, OH*OW > 64
    (5, 3, 3, 3, 1, 1),       # OH*OW = 9: 64 = 7 * 9 + 1, the frame base advances by 7 or 8 frames
    (40, 3, 3, 3, 1, 1),      # the same under split-K; the last split runs past frame N
    (3, 9, 3, 3, 1, 0),       # OW == 1
    (70, 3, 3, 3, 1, 0),      # OH*OW == 1
    (2, 15, 13, 3, 2, 1),     # stride 2 on an odd map
    (2, 8, 9, 3, 2, 0),       # stride 2, pad 0
    (2, 8, 9, 3, 1, 0),       # valid 3x3
    (2, 9, 7, 1, 2, 0),       # strided 1x1 (the ResNet downsample): general kernel with one tap
    (3, 9, 11, 1, 1, 0),      # pointwise, two splits
    (2, 4, 4, 1, 1, 0),       # pointwise, no split
    (1, 17, 19, 7, 2, 3),     # 7x7 filter
    (2, 9, 9, 5, 1, 2),       # 5x5 filter
]
CHANNELS = [(64, 96), (100, 164), (4, 8), (36, 44)]       # (cin, cout)
# 2 x 64 x 65 = 8320 rows of a 32 x 32-channel 1x1 problem: 33 slabs of 256 rows, reduced by splitk_reduce_kernel<16>
# (an odd slab count: the reduce's unpaired last slab)
MANY_SLABS = ((2, 64, 65, 1, 1, 0), 32, 32)

# exact cases at the heuristic tile: every geometry x every channel pair (the 7x7 / 5x5 filters without the widest pair,
# whose float64 reference is the slowest of the table and adds no address arithmetic the 3x3 cases lack; the 7x7 also at cin 8)
EXACT_CASES = [(g, cin, cout, (0, 0)) for g in GEOMS for cin, cout in CHANNELS if not (g[3] > 3 and (cin, cout) == (100, 164))]
EXACT_CASES += [((1, 17, 19, 7, 2, 3), 8, 44, (0, 0)), MANY_SLABS + ((0, 0),)]
# every tile at channels ragged under every tile: general / pointwise, without / with split-K
TILE_GEOMS = [(2, 6, 6, 3, 1, 1), (2, 13, 11, 3, 1, 1), (2, 4, 4, 1, 1, 0), (3, 9, 11, 1, 1, 0)]
TILE_CASES = [(g, 100, 164, t) for g in TILE_GEOMS for t in TILES]
# accumulation error: one general and one pointwise geometry, both under split-K
FLOAT_CASES = [((2, 13, 11, 3, 1, 1), 100, 164, (0, 0)), ((3, 9, 11, 1, 1, 0), 100, 164, (0, 0))]
ALL_CASES = EXACT_CASES + TILE_CASES + FLOAT_CASES


def case_id(case):
    g, cin, cout, (mt, nt) = case
    return "n%d_%dx%d_k%ds%dp%d-ci%d_co%d-t%dx%d" % (g + (cin, cout, mt, nt))


def out_hw(geom):
    n, h, w, k, stride, pad = geom
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def rows(geom):
    oh, ow = out_hw(geom)
    return geom[0] * oh * ow


def channel_scale(c):
    """2^(c mod 11 - 5) per channel: three decades, exact in every float format"""
    return np.ldexp(1.0, np.arange(c) % 11 - 5)


def exact_case(geom, cin, cout, seed):
    """(dy, x) float32 NHWC: integers in [-4, 4] times the channel's power of two.  Every product dy * x is an integer of at
    most 16 times 2^(e_co + e_ci), so every partial sum of an entry, in any order, is an integer below 16 * M times that
    unit: exact in fp32 while 16 * M <= 2^24 (asserted in tests/test_wgrad_plan_cpu.py)."""
    n, h, w, k, stride, pad = geom
    oh, ow = out_hw(geom)
    rng = np.random.default_rng(seed)
    dy = rng.integers(-4, 5, size=(n, oh, ow, cout)).astype(np.float64) * channel_scale(cout)
    x = rng.integers(-4, 5, size=(n, h, w, cin)).astype(np.float64) * channel_scale(cin)
    return torch.from_numpy(dy.astype(np.float32)), torch.from_numpy(x.astype(np.float32))


def float_case(geom, cin, cout, seed):
    """(dy, x) float32 NHWC: Gaussian dy, x = relu(N(0.5, 1)) (positive mean, as behind a ReLU), the same channel scales"""
    n, h, w, k, stride, pad = geom
    oh, ow = out_hw(geom)
    rng = np.random.default_rng(seed)
    dy = rng.standard_normal((n, oh, ow, cout)) * channel_scale(cout)
    x = np.maximum(rng.standard_normal((n, h, w, cin)) + 0.5, 0.0) * channel_scale(cin)
    return torch.from_numpy(dy.astype(np.float32)), torch.from_numpy(x.astype(np.float32))


def reference(dy, x, geom):
    """dW [cout][k][k][cin] in float64: unfold + einsum, straight from the definition"""
    n, h, w, k, stride, pad = geom
    oh, ow = out_hw(geom)
    cin, cout = x.shape[3], dy.shape[3]
    cols = F.unfold(x.double().permute(0, 3, 1, 2), k, padding=pad, stride=stride)      # (n, cin * k * k, oh * ow)
    cols = cols.reshape(n, cin, k, k, oh * ow)
    return torch.einsum("nlo,ncrsl->orsc", dy.double().reshape(n, oh * ow, cout), cols).contiguous()


def abs_reference(dy, x, geom):
    """A[co][r][s][ci]: the sum of the absolute products of an entry (the scale of its rounding error)"""
    return reference(dy.abs(), x.abs(), geom)


def loop_reference(dy, x, geom):
    """the same sum, pixel by pixel and tap by tap (tiny cases only): independent of unfold's layout and padding rules"""
    n, h, w, k, stride, pad = geom
    oh, ow = out_hw(geom)
    dy64, x64 = dy.double().numpy(), x.double().numpy()
    dw = np.zeros((dy.shape[3], k, k, x.shape[3]))
    for f in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for r in range(k):
                    for s in range(k):
                        iy, ix = oy * stride + r - pad, ox * stride + s - pad
                        if 0 <= iy < h and 0 <= ix < w:
                            dw[:, r, s, :] += np.outer(dy64[f, oy, ox], x64[f, iy, ix])
    return torch.from_numpy(dw)


def plan(L, geom, cin, cout, tile):
    """tbn_conv2d_wgrad_plan as a dict (host only)"""
    import ctypes as C
    n, h, w, k, stride, pad = geom
    out = (C.c_int * 8)()
    ws = L.tbn_conv2d_wgrad_plan(n, h, w, cin, cout, k, stride, pad, tile[0], tile[1], out)
    assert ws >= 0, L.tbn_last_error()
    keys = ("mt", "nt", "mode", "splits", "rows_per_split", "tiles_co", "tiles_ci", "reduce")
    d = dict(zip(keys, list(out)))
    d["ws_floats"] = ws
    return d
