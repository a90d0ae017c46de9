"""The 7x7 / stride 2 / pad 3 stem at operator level: tbn_stem_conv_fwd / tbn_stem_conv_wgrad (the launch sequence the
engine runs for conv1_7x7_s2, include/tbn_hip.h) against F.conv2d in fp64 and its autograd, for EVERY input-channel count
the plan admits (1..16) and BOTH input-image layouts (space-to-depth, row runs) -- the runtime-channel repack kernels,
every run-padding residue (7 cin rounded up to x4: 0..3 floats), 16-B and 8-B aligned runs, packed K that is no multiple
of 32, and maps far below the engine's 32 x 32 minimum.

Value comparisons: 1e-4 of the tensor maximum (TOL of tests/test_kernels_gpu.py).  The impulse tests are exact: a one-hot
operand makes every output a single product by 1.0 plus zeros, so one wrong tap, parity or padding offset fails bit-wise.
Every call runs on a NaN-filled workspace and writes into NaN-filled destinations: stale workspace contents, whatever lies
behind the bordered image, and any store outside the destination show up as NaN / a moved byte."""
import ctypes as C
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import call, lib, ptr  # noqa: E402

DEV = "cuda"
TOL = 1e-4
NAN = float("nan")
COUT = 64          # the engine's conv1
PAD = 16           # destination / dy column slice: [PAD, PAD + cout) of a buffer 2 * PAD wider

# (n, h, w), chosen for what they hit:
SHAPES = [
    (3, 17, 19),   # M = 270: ragged 128- and 256-row tiles, frame boundaries inside a tile; odd / odd
    (2, 16, 22),   # even / even
    (2, 15, 18),   # odd / even
    (1, 18, 13),   # even / odd, M = 63 < one 64-row weight-gradient step
    (5, 7, 7),     # output map (4 x 4) smaller than the filter
    (4, 32, 32),   # M = 1024: split-K and slab reduce of the weight gradient
]
CINS = list(range(1, 17))
# forward: the size heuristic and every candidate the autotuner may pick for the stem
FWD_TILES = [(0, 0, 0)] + [(mt, nt, sg) for mt in (1, 2) for nt in (1, 2) for sg in (1, 2)]
# weight gradient: the heuristic and six of the eleven admitted tiles
WGRAD_TILES = [(0, 0)] + [(mt, nt) for mt in (1, 2) for nt in (1, 2, 3)]


def st():
    return torch.cuda.current_stream().cuda_stream


def g(seed):
    return torch.Generator().manual_seed(seed)


def geometry(cin, h, w, layout):
    out = (C.c_int * 8)()
    call("tbn_stem_geometry", cin, h, w, layout, out)
    return list(out)


def workspace(cin, n, h, w, cout):
    """one NaN-fillable workspace that serves every layout of the case"""
    floats = max(lib().tbn_stem_workspace_floats(cin, h, w, layout, n, cout) for layout in (0, 1, 2))
    assert floats > 0
    return torch.empty(floats, device=DEV)


def rows(t):
    """(n, c, h, w) -> (n h w, c): the NHWC pixel rows the kernels write"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def case(cin, n, h, w, cout=COUT):
    """operands and the fp64 reference of one (cin, shape), computed once and shared by the tests (never modified)"""
    x = torch.randn(n, cin, h, w, generator=g(100 + cin))
    wt = torch.randn(cout, cin, 7, 7, generator=g(200 + cin)) / (49 * cin) ** 0.5
    bias = torch.randn(cout, generator=g(3))
    scale = torch.rand(cout, generator=g(5)) + 0.5
    shift = torch.randn(cout, generator=g(6))
    wr = wt.double().requires_grad_(True)
    y = F.conv2d(x.double(), wr, stride=2, padding=3)
    dy = torch.randn(y.shape, generator=g(4))
    y.backward(dy.double())
    y = y.detach()
    oh, ow = y.shape[2:]
    assert (oh, ow) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    c = dict(n=n, h=h, w=w, cin=cin, cout=cout, oh=oh, ow=ow, M=n * oh * ow, x=x, wt=wt,
             w_khwc=wt.permute(0, 2, 3, 1).contiguous(), bias=bias, scale=scale, shift=shift, dy=dy,
             y=rows(y), dw=wr.grad.permute(0, 2, 3, 1).contiguous())
    c["y_bias"] = c["y"] + bias.double()
    c["y_eval"] = F.relu(c["y"] * scale.double() + shift.double())
    c["s1"], c["s2"] = c["y"].sum(0), (c["y"] * c["y"]).sum(0)
    return c


class Checks:
    """errors and flags stay on the device until the end of a test: one synchronisation, every failing label reported"""

    def __init__(self):
        self.err, self.flag = [], []

    def close(self, label, got, want):
        self.err.append((label, (got.double() - want).abs().max() / want.abs().max()))

    def true(self, label, cond):
        self.flag.append((label, cond if torch.is_tensor(cond) else torch.tensor(bool(cond), device=DEV)))

    def finish(self):
        bad = []
        if self.err:
            e = torch.stack([v for _, v in self.err]).cpu()
            bad += [(lab, float(v)) for (lab, _), v in zip(self.err, e) if not v < TOL]      # NaN fails
            print("worst relative error %.2e over %d comparisons" % (float(e.max()), len(e)))
        if self.flag:
            f = torch.stack([v.reshape(()) for _, v in self.flag]).cpu()
            bad += [lab for (lab, _), v in zip(self.flag, f) if not bool(v)]
        assert not bad, bad[:12]


def run_fwd(c, dev, ws, layout, tile, epi, partial=None):
    """tbn_stem_conv_fwd into the column slice [PAD, PAD + cout) of a NaN-filled buffer, on a NaN-filled workspace"""
    mt, nt, stages = tile
    wide = torch.full((c["M"], c["cout"] + 2 * PAD), NAN, device=DEV)
    ws.fill_(NAN)
    call("tbn_stem_conv_fwd", ptr(dev["x"]), ptr(dev["w"]), ptr(dev["bias"]), wide.data_ptr() + PAD * 4, wide.shape[1],
         c["n"], c["h"], c["w"], c["cin"], c["cout"], layout, epi, ptr(dev["scale"]), ptr(dev["shift"]), ptr(partial),
         mt, nt, stages, ptr(ws), st())
    return wide


def outside_untouched(wide, cout):
    return torch.isnan(wide[:, :PAD]).all() & torch.isnan(wide[:, PAD + cout:]).all()


def to_dev(c):
    d = {k: c[k].to(DEV) for k in ("x", "bias", "scale", "shift")}
    d["w"] = c["w_khwc"].to(DEV)
    for k in ("y", "y_bias", "y_eval", "s1", "s2", "dw"):
        d[k] = c[k].to(DEV)
    return d


def fwd_checks(ck, c, dev, ws, layouts, tiles, epilogues):
    """every (epilogue, layout, tile): values against the fp64 reference, nothing outside the slice moved; returns the
    output slices for bit comparisons between layouts"""
    M, cout = c["M"], c["cout"]
    outs = {}
    for epi, layout, tile in itertools.product(epilogues, layouts, tiles):
        lab = "cin %d %s layout %d tile %s epilogue %d" % (c["cin"], (c["n"], c["h"], c["w"]), layout, tile, epi)
        part = None
        if epi == 1:
            # explicit tile: exactly ceil(M / (128 mt)) partial rows, all of them written (NaN otherwise); heuristic tile:
            # at most ceil(M / 128) rows, the rest stays zero
            mt = tile[0]
            part = (torch.full((-(-M // (128 * mt)), 2, cout), NAN, device=DEV) if mt
                    else torch.zeros(-(-M // 128), 2, cout, device=DEV))
        wide = run_fwd(c, dev, ws, layout, tile, epi, part)
        y = wide[:, PAD:PAD + cout]
        ck.close(lab, y, dev[("y_bias", "y", "y_eval")[epi]])
        ck.true(lab + ": outside the slice", outside_untouched(wide, cout))
        if epi == 1:
            ck.close(lab + ": sum", part[:, 0].double().sum(0), dev["s1"])
            ck.close(lab + ": sum of squares", part[:, 1].double().sum(0), dev["s2"])
        outs[(epi, layout, tile)] = y
    return outs


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cin", CINS)
def test_stem_forward(cin, shape):
    """both layouts and the rule, the heuristic tile and every autotune candidate, all three epilogues"""
    c = case(cin, *shape)
    dev, ws, ck = to_dev(c), workspace(cin, *shape, COUT), Checks()
    outs = fwd_checks(ck, c, dev, ws, (1, 2, 0), FWD_TILES, (0, 1, 2))
    ruled = geometry(cin, shape[1], shape[2], 0)[0]
    assert ruled == (1 if cin <= 3 else 2)
    for epi, tile in itertools.product((0, 1, 2), FWD_TILES):
        ck.true("cin %d %s tile %s epilogue %d: layout 0 is not bit-equal to layout %d" % (cin, shape, tile, epi, ruled),
                torch.equal(outs[(epi, 0, tile)], outs[(epi, ruled, tile)]))
    ck.finish()


@pytest.mark.parametrize("cout", [32, 96])
@pytest.mark.parametrize("cin", CINS)
def test_stem_forward_ragged_n_tile(cin, cout):
    """cout 32 under a 64-column tile, cout 96 under 64-column tiles: the last N tile is ragged"""
    shape = SHAPES[0]
    c = case(cin, *shape, cout)
    dev, ws, ck = to_dev(c), workspace(cin, *shape, cout), Checks()
    fwd_checks(ck, c, dev, ws, (1, 2), [(0, 0, 0), (1, 1, 0), (1, 2, 0), (2, 1, 0), (2, 2, 0)], (0, 1, 2))
    ck.finish()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cin", CINS)
def test_stem_wgrad(cin, shape):
    """both layouts and the rule, the heuristic tile and six explicit tiles; dweight starts as NaN, every call runs twice
    and must repeat bit for bit; dy is a column slice of a wider NaN-filled buffer"""
    c = case(cin, *shape)
    n, h, w = shape
    dev, ws, ck = to_dev(c), workspace(cin, *shape, COUT), Checks()
    dyw = torch.full((c["M"], COUT + 2 * PAD), NAN, device=DEV)
    dyw[:, PAD:PAD + COUT] = rows(c["dy"]).to(DEV)
    ruled = geometry(cin, h, w, 0)[0]
    outs = {}
    for layout, tile in itertools.product((1, 2, 0), WGRAD_TILES):
        lab = "cin %d %s layout %d tile %s" % (cin, shape, layout, tile)
        got = []
        for _ in range(2):
            dw = torch.full((COUT, 7, 7, cin), NAN, device=DEV)
            ws.fill_(NAN)
            call("tbn_stem_conv_wgrad", dyw.data_ptr() + PAD * 4, dyw.shape[1], ptr(dev["x"]), ptr(dw), n, h, w, cin, COUT,
                 layout, tile[0], tile[1], ptr(ws), st())
            got.append(dw)
        ck.close(lab, got[0], dev["dw"])
        ck.true(lab + ": the second run differs", torch.equal(got[0], got[1]))
        outs[(layout, tile)] = got[0]
    for tile in WGRAD_TILES:
        ck.true("cin %d %s tile %s: layout 0 is not bit-equal to layout %d" % (cin, shape, tile, ruled),
                torch.equal(outs[(0, tile)], outs[(ruled, tile)]))
    ck.finish()


IMPULSE_SHAPES = [(3, 17, 19), (2, 16, 22), (5, 7, 7)]


@pytest.mark.parametrize("cin", CINS)
def test_stem_forward_impulse_is_exact(cin):
    """a one-hot input: every output is one weight (times 1.0) or zero, so the result equals the fp32 F.conv2d of the same
    impulse bit for bit (that reference is exact as well: one product by 1.0 plus zeros)"""
    ck = Checks()
    for shape in IMPULSE_SHAPES:
        n, h, w = shape
        wt = torch.randn(COUT, cin, 7, 7, generator=g(300 + cin))
        c = dict(n=n, h=h, w=w, cin=cin, cout=COUT, M=n * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1))
        ws = workspace(cin, *shape, COUT)
        zero = torch.zeros(COUT, device=DEV)
        dev = dict(w=wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias=None, scale=zero, shift=zero)
        impulses = {
            "corner": (0, 0, 0, 0),
            "last pixel of the last frame": (n - 1, 0, h - 1, w - 1),
            "last channel": (min(1, n - 1), cin - 1, 0, w - 1),
            "interior odd / odd": (n // 2, cin // 2, min(5, h - 2) | 1, min(7, w - 2) | 1),
        }
        for name, pos in impulses.items():
            x = torch.zeros(n, cin, h, w)
            x[pos] = 1.0
            want = rows(F.conv2d(x, wt, stride=2, padding=3)).to(DEV)
            assert int((want != 0).sum()) > 0
            dev["x"] = x.to(DEV)
            for layout, tile in itertools.product((1, 2), [(0, 0, 0), (2, 1, 1)]):
                wide = run_fwd(c, dev, ws, layout, tile, 0)
                lab = "cin %d %s impulse at %s (%s) layout %d tile %s" % (cin, shape, pos, name, layout, tile)
                ck.true(lab, torch.equal(wide[:, PAD:PAD + COUT], want))
                ck.true(lab + ": outside the slice", outside_untouched(wide, COUT))
    ck.finish()


@pytest.mark.parametrize("cin", CINS)
def test_stem_wgrad_impulse_is_exact(cin):
    """a one-hot dy at (frame, channel co, oy, ox): dweight[co] is the 7 x 7 input patch of that output pixel, bit for bit,
    with zeros where the patch leaves the image; every other output channel is zero"""
    ck = Checks()
    for shape in [(3, 17, 19), (5, 7, 7), (4, 32, 32)]:
        n, h, w = shape
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        x = torch.randn(n, cin, h, w, generator=g(400 + cin))
        xpad = F.pad(x, (3, 3, 3, 3))
        xd, ws = x.to(DEV), workspace(cin, *shape, COUT)
        for ni, co, oy, ox in ((0, 0, 0, 0), (n - 1, COUT - 1, oh - 1, ow - 1), (n // 2, 37, oh // 2, ow // 2)):
            dy = torch.zeros(n, oh, ow, COUT)
            dy[ni, oy, ox, co] = 1.0
            dyd = dy.to(DEV)
            want = torch.zeros(COUT, 7, 7, cin)
            want[co] = xpad[ni, :, 2 * oy:2 * oy + 7, 2 * ox:2 * ox + 7].permute(1, 2, 0)
            want = want.to(DEV)
            for layout, tile in itertools.product((1, 2), [(0, 0), (1, 3)]):
                dw = torch.full((COUT, 7, 7, cin), NAN, device=DEV)
                ws.fill_(NAN)
                call("tbn_stem_conv_wgrad", ptr(dyd), COUT, ptr(xd), ptr(dw), n, h, w, cin, COUT, layout, tile[0], tile[1],
                     ptr(ws), st())
                ck.true("cin %d %s dy impulse at %s layout %d tile %s" % (cin, shape, (ni, co, oy, ox), layout, tile),
                        torch.equal(dw, want))
    ck.finish()


@pytest.mark.parametrize("cin", [1, 2, 3, 4, 10, 16])
def test_stem_entry_is_the_engines_conv1(cin):
    """what keeps the aid honest: conv1's raw output of a training forward of the whole backbone (2 frames of 64 x 64,
    heuristic plan) is bit-equal to tbn_stem_conv_fwd at the plan's tile with the statistics epilogue"""
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    n, h, w = 2, 64, 64
    net = BNInception(1000, cin).to(DEV)
    net.autotune = False
    net.train()
    x = torch.randn(n, cin, h, w, generator=g(7)).to(DEV)
    net(x)
    plan = net._plans[(n, h, w)]
    wsp = plan.pool[0][0].view(torch.float32)
    off, nrow, ncol, ld = C.c_long(), C.c_int(), C.c_int(), C.c_int()
    call("tbn_backbone_tensor_info", plan.handle, b"conv1_7x7_s2", 1, C.byref(off), C.byref(nrow), C.byref(ncol), C.byref(ld))
    y_engine = torch.as_strided(wsp, (nrow.value, ncol.value), (ld.value, 1), off.value).clone()
    assert (nrow.value, ncol.value) == (n * 32 * 32, 64)
    info = (C.c_int * 16)()
    call("tbn_backbone_launch_info", plan.handle, b"conv1_7x7_s2", 1, info)
    variant, mt, nt, stages = list(info)[:4]
    assert variant == 0 and mt in (1, 2) and 1 <= nt <= 4
    L = net._layers["conv1_7x7_s2"]
    wt = net.flat_weight.detach()[L["w_off"]:L["w_off"] + 64 * 49 * cin].clone()
    ws = workspace(cin, n, h, w, 64)
    ws.fill_(NAN)
    y = torch.full((n * 32 * 32, 64), NAN, device=DEV)
    part = torch.full((-(-n * 32 * 32 // (128 * mt)), 2, 64), NAN, device=DEV)
    call("tbn_stem_conv_fwd", ptr(x), ptr(wt), 0, ptr(y), 64, n, h, w, cin, 64, 0, 1, 0, 0, ptr(part), mt, nt, stages, ptr(ws),
         st())
    assert torch.isfinite(y_engine).all() and float(y_engine.abs().max()) > 0
    assert torch.equal(y, y_engine), (cin, (mt, nt, stages), float((y - y_engine).abs().max()))
    assert torch.isfinite(part).all()
