"""The forward / data-gradient half of csrc/conv_igemm.hip at operator level, through tbn_conv_launch / tbn_conv_launch_pair:
the generic 1- / 2-stage kernels, the LDS-halo, LDS-DMA and split-K tile families, the parity-phase launch of strided data
gradients and the pair launch, over the geometry table of tests/conv_check.py (each row the smallest map where one mechanism
of the address arithmetic exists; tests/test_conv_plan_cpu.py proves that on the host).

Exact cases (integer data times per-channel powers of two: every partial sum in any order is exact in fp32) are compared
bit for bit with the float64 reference, so every family, tile and stage count returns the same bits.  The input is a column
slice of a buffer 32 columns wider (in_ld = c + 32, the pointer 16 floats in), the output likewise; the surrounding
columns, 256 floats before and after each buffer and the rows behind the last pixel hold NaN, which any read outside the
slice would carry into the result and any write outside it would overwrite.  Float cases are held per element to TOL times
the element's absolute sum, sums over pixels (BN statistics, BN-backward reduce) per channel to their own absolute sums
(conv_check.stat_bounds / reduce_reference), and every partial row tbn_conv_partial_rows counts must have been written --
and no row behind them."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import ConvDesc, call, lib, ptr  # noqa: E402
from tests import conv_check as cc  # noqa: E402
from tests.test_conv_variants_gpu import ACCUM, DEV, HALO, RELU, SK4, st, tiles_for, variants_for  # noqa: E402

G = 256          # guard floats before and after every buffer
WIDE, OFF = 32, 16   # a slice sits OFF columns into a buffer WIDE columns wider
NAN = float("nan")


class Sliced:
    """(rows, c) values as a column slice of a (rows, c + WIDE) buffer between two guards, NaN everywhere else; `dense`: the
    plain (rows, c) buffer between the guards"""

    def __init__(self, rows, c, values=None, dense=False):
        self.rows, self.c = rows, c
        self.ld, self.off = (c, 0) if dense else (c + WIDE, OFF)
        self.flat = torch.full((2 * G + rows * self.ld,), NAN, device=DEV)
        if values is not None:
            self.view().copy_(values.reshape(rows, c))
        self.before = self.flat.clone()

    def view(self):
        return self.flat[G:G + self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.c]

    def ptr(self):
        return self.flat.data_ptr() + 4 * (G + self.off)

    def outside_untouched(self):
        """every float outside the slice holds the bits it held before the launch"""
        a, b = self.flat.clone(), self.before.clone()
        for t in (a, b):
            t[G:G + self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.c] = 0
        return torch.equal(a.view(torch.int32), b.view(torch.int32))


def make_desc(geom, cin, cout, dgrad, inp, weight, out, epilogue=0, flags=0, stages=0, bias=None, scale=None, shift=None,
              stat_partial=None, red=None, red_stats=None):
    """inp / out: Sliced buffers; red: [(y tensor, y_ld, col_begin, channels, partial tensor)] with the statistics of all cin
    producer channels in red_stats (4, cin)"""
    n, h, w, k, s, p = geom
    d = ConvDesc()
    d.inp, d.in_ld, d.weight, d.bias, d.out, d.out_ld = inp.ptr(), inp.ld, ptr(weight), ptr(bias), out.ptr(), out.ld
    d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = n, h, w, cin, cout, k, s, p
    d.dgrad, d.epilogue, d.flags, d.stages = int(dgrad), epilogue, flags, stages
    d.scale, d.shift, d.stat_partial = ptr(scale), ptr(shift), ptr(stat_partial)
    if red:
        d.nred = len(red)
        for i, (y, y_ld, c0, cc_, part) in enumerate(red):
            d.red[i].y, d.red[i].y_ld, d.red[i].col_begin, d.red[i].channels = ptr(y), y_ld, c0, cc_
            d.red[i].stat_offset, d.red[i].partial = c0, ptr(part)
        d.red_stats, d.red_stats_stride = ptr(red_stats), cin
    return d


class Case:
    """one (geometry, cin, cout) problem: data, float64 references (computed once) and the device operands"""

    def __init__(self, case, exact, seed):
        g, cin, cout = case
        self.case, self.geom, self.cin, self.cout, self.exact = case, g, cin, cout, exact
        n, h, w, k, s, p = g
        oh, ow = cc.out_hw(g)
        self.M, self.P = n * oh * ow, n * h * w
        d = (cc.exact_case if exact else cc.float_case)(g, cin, cout, seed)
        self.d = d
        self.y = cc.forward_reference(d["x"], d["w"], g).reshape(self.M, cout)
        self.dx = cc.dgrad_reference(d["dy"], d["w"], g).reshape(self.P, cin)
        self.ya = cc.forward_reference(d["x"].abs(), d["w"].abs(), g).reshape(self.M, cout)
        self.dxa = cc.dgrad_reference(d["dy"].abs(), d["w"].abs(), g).reshape(self.P, cin)
        self.wd = d["w"].to(DEV)
        self.ws = torch.empty(cout * k * k * cin, device=DEV)          # the data gradient's flipped weights
        self.x_in, self.dy_in = Sliced(self.P, cin, d["x"].to(DEV)), Sliced(self.M, cout, d["dy"].to(DEV))
        self.x_dense = Sliced(self.P, cin, d["x"].to(DEV), dense=True)
        self.dy_dense = Sliced(self.M, cout, d["dy"].to(DEV), dense=True)
        self.dev = {key: d[key].to(DEV) for key in d if key in ("bias", "scale", "shift")}
        # producer side of the data gradient: two BN layers of different pitch behind the cin input channels (one at cin 32)
        self.split = 32 if cin > 32 else cin
        self.yb, self.stats = cc.reduce_inputs(self.P, cin, seed + 1)
        self.statsd = self.stats.to(DEV).contiguous()
        self.y0 = torch.zeros(self.P, self.split + 8, device=DEV)
        self.y0[:, :self.split] = self.yb[:, :self.split].to(DEV)
        self.y1 = self.yb[:, self.split:].contiguous().to(DEV) if self.split < cin else None
        self.s1, self.s2, self.b1, self.b2 = cc.reduce_reference(self.dx, self.dxa, self.yb, self.stats)

    def fwd(self, out, inp=None, **kw):
        return make_desc(self.geom, self.cin, self.cout, False, inp or self.x_in, self.wd, out, **kw)

    def dgrad(self, out, inp=None, **kw):
        return make_desc(self.geom, self.cin, self.cout, True, inp or self.dy_in, self.wd, out, **kw)

    def partial_rows(self, d, mt, pair=0):
        return lib().tbn_conv_partial_rows(C.byref(d), mt, pair)

    def red_buffers(self, rows):
        """NaN-filled partial buffers of rows + 2 rows per segment, and the `red` list of make_desc"""
        segs = [(self.y0, self.y0.shape[1], 0, self.split)]
        if self.y1 is not None:
            segs.append((self.y1, self.y1.shape[1], self.split, self.cin - self.split))
        bufs = [torch.full((rows + 2, 2, c), NAN, device=DEV) for _, _, _, c in segs]
        return bufs, [sg + (b,) for sg, b in zip(segs, bufs)]

    def check_rows(self, bufs, rows, tag):
        """every counted partial row was written, and none behind them"""
        for b in bufs:
            assert bool(torch.isfinite(b[:rows]).all()), ("a counted partial row was not written", tag)
            assert bool(torch.isnan(b[rows:]).all()), ("a partial row beyond the count was written", tag)

    def check_reduce(self, bufs, rows, tag):
        """column sums of the partial rows (in float64) per channel against their own bounds; returns the worst ratio"""
        self.check_rows(bufs, rows, tag)
        s1 = torch.cat([b[:rows, 0].double().sum(0).cpu() for b in bufs])
        s2 = torch.cat([b[:rows, 1].double().sum(0).cpu() for b in bufs])
        r1, r2 = (s1 - self.s1).abs() / self.b1.clamp_min(1e-300), (s2 - self.s2).abs() / self.b2.clamp_min(1e-300)
        assert float(r1.max()) <= 1 and float(r2.max()) <= 1, (tag, float(r1.max()), float(r2.max()))
        return max(float(r1.max()), float(r2.max()))

    def check_stats(self, part, rows, tag):
        self.check_rows([part], rows, tag)
        b1, b2 = cc.stat_bounds(self.ya)
        s1, s2 = part[:rows, 0].double().sum(0).cpu(), part[:rows, 1].double().sum(0).cpu()
        r1 = (s1 - self.y.sum(0)).abs() / b1.clamp_min(1e-300)
        r2 = (s2 - (self.y * self.y).sum(0)).abs() / b2.clamp_min(1e-300)
        assert float(r1.max()) <= 1 and float(r2.max()) <= 1, (tag, float(r1.max()), float(r2.max()))
        return max(float(r1.max()), float(r2.max()))


@functools.lru_cache(maxsize=None)
def exact(case):
    return Case(case, True, seed=101)


@functools.lru_cache(maxsize=None)
def floating(case):
    return Case(case, False, seed=202)


def launch(d, mt, nt, ws=None):
    call("tbn_conv_launch", C.byref(d), mt, nt, ptr(ws), st())


def variants(geom, dgrad):
    """every (flags, stages, mt, nt) variants_for / tiles_for admit for the launch"""
    n, h, w, k, s, p = geom
    wk = cc.out_hw(geom)[1] if dgrad else w         # the width of the map the kernel reads
    return [(f, sg, mt, nt) for f, sg in variants_for(k, s, p, wk, dgrad) for mt, nt in tiles_for(f)]


@pytest.mark.parametrize("case", cc.EXACT_CASES, ids=cc.case_id)
def test_forward_exact_every_family_tile_and_pitch(case):
    """epilogue 0 with bias, + ReLU, accumulating (with and without bias: the general and the lean store loop), the eval
    epilogue with power-of-two scales, and the statistics epilogue's raw output: bit-equal to the reference in every family,
    tile and stage count, from a pitched input into a pitched output, nothing outside the slice touched; the accumulating
    forms read a dense input (in_ld == cin)"""
    P = exact(case)
    g, cin, cout = case
    b, base = P.d["bias"].double(), P.d["base"].double().reshape(P.M, cout)
    sc, sh = P.d["scale"].double(), P.d["shift"].double()
    refs = {key: v.float().to(DEV) for key, v in dict(
        bias=P.y + b, relu=torch.relu(P.y + b), acc=P.y + base, accb=P.y + b + base, ev=torch.relu(P.y * sc + sh), raw=P.y).items()}
    based = P.d["base"].to(DEV)
    for flags, stages, mt, nt in variants(g, False):
        tag = (case, flags, stages, mt, nt)
        kw = dict(flags=flags, stages=stages)
        forms = [("bias", dict(bias=P.dev["bias"]), None, None),
                 ("relu", dict(bias=P.dev["bias"], flags=flags | RELU), None, None),
                 ("acc", dict(flags=flags | ACCUM), based, P.x_dense),
                 ("accb", dict(bias=P.dev["bias"], flags=flags | ACCUM), based, P.x_dense),
                 ("ev", dict(epilogue=2, scale=P.dev["scale"], shift=P.dev["shift"]), None, None)]
        for name, extra, start, inp in forms:
            out = Sliced(P.M, cout, start)
            launch(P.fwd(out, inp=inp, **{**kw, **extra}), mt, nt)
            assert torch.equal(out.view(), refs[name]), (name, tag)
            assert out.outside_untouched(), (name, tag)
        out = Sliced(P.M, cout)
        probe = P.fwd(out, epilogue=1, **kw)
        rows = P.partial_rows(probe, mt)
        part = torch.full((rows + 2, 2, cout), NAN, device=DEV)
        launch(P.fwd(out, epilogue=1, stat_partial=part, **kw), mt, nt)
        assert torch.equal(out.view(), refs["raw"]) and out.outside_untouched(), ("stats", tag)
        P.check_stats(part, rows, tag)


@pytest.mark.parametrize("case", cc.EXACT_CASES, ids=cc.case_id)
def test_dgrad_exact_every_family_tile_and_pitch(case):
    """plain into a channel slice (pixels no output pixel read, and the parities a 1x1 / stride-2 layer leaves without a tap,
    exactly 0), accumulating on exact values and -- strided -- on a 3.0-filled buffer (untouched pixels keep exactly 3.0), and
    with the fused BN-backward reduce on two producer segments of different pitch: dz bit-equal, every counted partial row
    written and none behind, column sums per channel inside their bounds.  Stride 2 = every tile and both stage counts of
    conv_igemm_phases_kernel."""
    P = exact(case)
    g, cin, cout = case
    n, h, w, k, s, p = g
    dbase = P.d["dbase"].double().reshape(P.P, cin)
    refs = {key: v.float().to(DEV) for key, v in dict(plain=P.dx, acc=P.dx + dbase, three=P.dx + 3.0).items()}
    unread = torch.from_numpy(cc.unread_pixels(g)).repeat(n, 1, 1).reshape(-1).to(DEV)
    if k == 1 and s == 2:
        assert int(unread.sum()) >= P.P // 2          # the parities without a tap
    for flags, stages, mt, nt in variants(g, True):
        tag = (case, flags, stages, mt, nt)
        kw = dict(flags=flags, stages=stages)
        out = Sliced(P.P, cin)
        launch(P.dgrad(out, **kw), mt, nt, P.ws)
        assert torch.equal(out.view(), refs["plain"]) and out.outside_untouched(), ("plain", tag)
        assert float(out.view()[unread].abs().max() if bool(unread.any()) else 0.0) == 0.0, ("unread pixels", tag)
        out = Sliced(P.P, cin, P.d["dbase"].to(DEV))
        launch(P.dgrad(out, inp=P.dy_dense, flags=flags | ACCUM, stages=stages), mt, nt, P.ws)
        assert torch.equal(out.view(), refs["acc"]) and out.outside_untouched(), ("accumulate", tag)
        if s == 2:
            out = Sliced(P.P, cin, torch.full((P.P, cin), 3.0, device=DEV))
            launch(P.dgrad(out, flags=flags | ACCUM, stages=stages), mt, nt, P.ws)
            assert torch.equal(out.view(), refs["three"]) and out.outside_untouched(), ("accumulate on 3.0", tag)
            assert bool((out.view()[unread] == 3.0).all()), ("untouched pixels keep 3.0", tag)
        out = Sliced(P.P, cin)
        rows = P.partial_rows(P.dgrad(out, **kw), mt)
        assert rows == cc.rows_written(g, True, (32 if flags & SK4 else 128) * mt)
        bufs, red = P.red_buffers(rows)
        launch(P.dgrad(out, red=red, red_stats=P.statsd, **kw), mt, nt, P.ws)
        assert torch.equal(out.view(), refs["plain"]) and out.outside_untouched(), ("reduce", tag)
        P.check_reduce(bufs, rows, tag)


def test_halo_family_refuses_width_65():
    g = (1, 2, 65, 3, 1, 1)
    assert all(f != HALO for f, _ in variants_for(3, 1, 1, 65, False)) and any(f == HALO for f, _ in variants_for(3, 1, 1, 64, False))
    P = exact((g, 32, 32))
    out = Sliced(P.M, 32)
    for d, ws in ((P.fwd(out, flags=HALO), None), (P.dgrad(out, flags=HALO), P.ws)):
        rc = lib().tbn_conv_launch(C.byref(d), 1, 1, ptr(ws), st())
        assert rc < 0 and b"LDS-halo kernel does not handle this shape" in lib().tbn_last_error()
    torch.cuda.synchronize()
    assert out.outside_untouched() and bool(torch.isnan(out.view()).all())


def test_accumulating_downsample_gradient_refuses_the_fused_reduce():
    """a 1x1 / stride-2 data gradient visits one parity in four: accumulating, the reduce would miss the gradient already in the
    other pixels -- refused on the host; without the reduce, or without accumulation, it runs (the exact tests)"""
    case = ((2, 9, 6, 1, 2, 0), 64, 96)
    P = exact(case)
    out = Sliced(P.P, 64, P.d["dbase"].to(DEV))
    bufs, red = P.red_buffers(P.partial_rows(P.dgrad(out), 1))
    rc = lib().tbn_conv_launch(C.byref(P.dgrad(out, flags=ACCUM, red=red, red_stats=P.statsd)), 1, 1, ptr(P.ws), st())
    assert rc < 0 and b"cannot carry the fused BN-backward reduce" in lib().tbn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.flat.view(torch.int32), out.before.view(torch.int32)) and bool(torch.isnan(bufs[0]).all())


def test_pair_launch_exact():
    """tbn_conv_launch_pair on two members with different channel counts, variants 0 / 1 / 2 at tiles (1,1) .. (2,2): biased,
    statistics, eval, data gradient without and with the reduce -- bit-equal, pitched operands, partial rows as counted"""
    g, cha, chb = cc.PAIR_CASE
    A, B = exact((g,) + cha), exact((g,) + chb)
    sides = []
    for Pm in (A, B):
        b, sc, sh = Pm.d["bias"].double(), Pm.d["scale"].double(), Pm.d["shift"].double()
        sides.append({key: v.float().to(DEV) for key, v in dict(
            bias=Pm.y + b, ev=torch.relu(Pm.y * sc + sh), raw=Pm.y, dx=Pm.dx).items()})

    def pair(da, db, variant, mt, nt, ws=(None, None)):
        call("tbn_conv_launch_pair", C.byref(da), C.byref(db), variant, mt, nt, ptr(ws[0]), ptr(ws[1]), st())
    for variant in (0, 1, 2):
        for mt in (1, 2):
            for nt in (1, 2):
                tag = (variant, mt, nt)
                for name, mk in (("bias", lambda Pm, o: Pm.fwd(o, bias=Pm.dev["bias"])),
                                 ("ev", lambda Pm, o: Pm.fwd(o, epilogue=2, scale=Pm.dev["scale"], shift=Pm.dev["shift"]))):
                    oa, ob = Sliced(A.M, A.cout), Sliced(B.M, B.cout)
                    pair(mk(A, oa), mk(B, ob), variant, mt, nt)
                    for o, side in ((oa, sides[0]), (ob, sides[1])):
                        assert torch.equal(o.view(), side[name]) and o.outside_untouched(), (name, tag)
                oa, ob = Sliced(A.M, A.cout), Sliced(B.M, B.cout)
                rows = A.partial_rows(A.fwd(oa, epilogue=1), mt, pair=1)
                assert rows == cc.rows_written(g, False, 128 * mt)
                pa, pb = (torch.full((rows + 2, 2, c), NAN, device=DEV) for c in (A.cout, B.cout))
                pair(A.fwd(oa, epilogue=1, stat_partial=pa), B.fwd(ob, epilogue=1, stat_partial=pb), variant, mt, nt)
                for Pm, o, side, part in ((A, oa, sides[0], pa), (B, ob, sides[1], pb)):
                    assert torch.equal(o.view(), side["raw"]) and o.outside_untouched(), ("stats", tag)
                    Pm.check_stats(part, rows, tag)
                oa, ob = Sliced(A.P, A.cin), Sliced(B.P, B.cin)
                pair(A.dgrad(oa), B.dgrad(ob), variant, mt, nt, (A.ws, B.ws))
                for o, side in ((oa, sides[0]), (ob, sides[1])):
                    assert torch.equal(o.view(), side["dx"]) and o.outside_untouched(), ("dgrad", tag)
                oa, ob = Sliced(A.P, A.cin), Sliced(B.P, B.cin)
                rows = A.partial_rows(A.dgrad(oa), mt, pair=1)
                assert rows == cc.rows_written(g, True, 128 * mt)
                (ba, ra), (bb, rb) = A.red_buffers(rows), B.red_buffers(rows)
                pair(A.dgrad(oa, red=ra, red_stats=A.statsd), B.dgrad(ob, red=rb, red_stats=B.statsd), variant, mt, nt, (A.ws, B.ws))
                for Pm, o, side, bufs in ((A, oa, sides[0], ba), (B, ob, sides[1], bb)):
                    assert torch.equal(o.view(), side["dx"]) and o.outside_untouched(), ("reduce", tag)
                    Pm.check_reduce(bufs, rows, tag)


@pytest.mark.parametrize("case", cc.FLOAT_CASES, ids=cc.case_id)
def test_float_cases_inside_the_per_element_bound(case):
    """Gaussian data with channel scales over 2^10, every family and tile: forward, statistics epilogue (s1 / s2 per channel
    against their own absolute sums), eval epilogue and data gradient with the reduce, each element against TOL times its own
    absolute sum.  Eval: relu is 1-Lipschitz and fma(v, scale, shift) rounds once (2^-24 of |v scale| + |shift|, far inside
    TOL), so the bound is TOL * (A |scale| + |shift|)."""
    P = floating(case)
    g, cin, cout = case
    sc, sh = P.d["scale"].double(), P.d["shift"].double()
    ev_ref, ev_a = torch.relu(P.y * sc + sh), P.ya * sc.abs() + sh.abs()
    worst = dict(forward=0.0, stats=0.0, eval=0.0, dgrad=0.0, reduce=0.0)
    for flags, stages, mt, nt in variants(g, False):
        tag = (case, flags, stages, mt, nt)
        kw = dict(flags=flags, stages=stages)
        out = Sliced(P.M, cout)
        rows = P.partial_rows(P.fwd(out, epilogue=1, **kw), mt)
        part = torch.full((rows + 2, 2, cout), NAN, device=DEV)
        launch(P.fwd(out, epilogue=1, stat_partial=part, **kw), mt, nt)
        r = cc.float_ratio(out.view(), P.y, P.ya)
        assert r <= 1 and out.outside_untouched(), ("forward", tag, r)
        worst["forward"] = max(worst["forward"], r)
        worst["stats"] = max(worst["stats"], P.check_stats(part, rows, tag))
        out = Sliced(P.M, cout)
        launch(P.fwd(out, epilogue=2, scale=P.dev["scale"], shift=P.dev["shift"], **kw), mt, nt)
        r = cc.float_ratio(out.view(), ev_ref, ev_a)
        assert r <= 1 and out.outside_untouched(), ("eval", tag, r)
        worst["eval"] = max(worst["eval"], r)
    for flags, stages, mt, nt in variants(g, True):
        tag = (case, flags, stages, mt, nt)
        kw = dict(flags=flags, stages=stages)
        out = Sliced(P.P, cin)
        rows = P.partial_rows(P.dgrad(out, **kw), mt)
        bufs, red = P.red_buffers(rows)
        launch(P.dgrad(out, red=red, red_stats=P.statsd, **kw), mt, nt, P.ws)
        r = cc.float_ratio(out.view(), P.dx, P.dxa)
        assert r <= 1 and out.outside_untouched(), ("dgrad", tag, r)
        worst["dgrad"] = max(worst["dgrad"], r)
        worst["reduce"] = max(worst["reduce"], P.check_reduce(bufs, rows, tag))
    print(cc.case_id(case), "worst error / bound (TOL %.1e of the absolute sum):" % cc.TOL,
          " ".join("%s %.3f" % kv for kv in worst.items()))


def test_one_repeat_of_one_launch_per_family_is_bit_identical():
    """determinism: the split-K tile kernel and the epilogue sums reduce in a fixed order"""
    P = floating(cc.FLOAT_CASES[0])
    S = floating(cc.FLOAT_CASES[2])
    runs = [(P, f, sg, dg) for f, sg in variants_for(3, 1, 1, 11, False) for dg in (False, True)] + [(S, 0, 2, True)]
    for Q, flags, stages, dg in runs:
        got = []
        for _ in range(2):
            out = Sliced(Q.P if dg else Q.M, Q.cin if dg else Q.cout)
            if dg:
                rows = Q.partial_rows(Q.dgrad(out, flags=flags, stages=stages), 2)
                bufs, red = Q.red_buffers(rows)
                launch(Q.dgrad(out, flags=flags, stages=stages, red=red, red_stats=Q.statsd), 2, 2, Q.ws)
            else:
                rows = Q.partial_rows(Q.fwd(out, epilogue=1, flags=flags, stages=stages), 2)
                bufs = [torch.full((rows + 2, 2, Q.cout), NAN, device=DEV)]
                launch(Q.fwd(out, epilogue=1, stat_partial=bufs[0], flags=flags, stages=stages), 2, 2)
            got.append([out.flat.clone()] + [b[:rows].clone() for b in bufs])
        for a, b in zip(*got):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (flags, stages, dg)
