"""Host-side checks of the forward / data-gradient operator tests (no GPU): the references of tests/conv_check.py against
explicit loops, the exactness of the exact cases, the float bound against an emulated fp32 sum, a CENSUS of the geometry
table (each row reaches the mechanism it names), the partial-row counts of the built library against the launch rules
restated in Python, the refusals of the C-ABI entries ahead of any launch, and the comparison rules against two wrong
references the older yardstick accepts."""
import ctypes as C

import numpy as np
import pytest
import torch

from attention_based_tbn_amd._lib import ConvDesc, lib
from tests import conv_check as cc
from tests.test_conv_variants_gpu import tiles_for, variants_for

HALO, DMA, SK4 = cc.HALO, cc.DMA, cc.SK4
BAD = 0x1000   # a pointer no refused call dereferences


def desc(geom, cin, cout, dgrad, flags=0, **kw):
    n, h, w, k, stride, pad = geom
    d = ConvDesc()
    d.inp, d.weight, d.out = BAD, BAD, BAD
    d.in_ld, d.out_ld = (cout, cin) if dgrad else (cin, cout)
    d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = n, h, w, cin, cout, k, stride, pad
    d.dgrad, d.flags = int(dgrad), flags
    for key, v in kw.items():
        setattr(d, key, v)
    return d


@pytest.mark.parametrize("geom", [(2, 5, 4, 3, 2, 1), (3, 4, 3, 3, 1, 0), (2, 3, 5, 1, 2, 0), (2, 4, 3, 3, 1, 2), (2, 5, 4, 3, 2, 0),
                                  (2, 1, 6, 3, 2, 2), (3, 3, 1, 3, 1, 1), (2, 4, 6, 3, 2, 2)])
def test_references_agree_with_explicit_loops(geom):
    """F.conv2d and its autograd against the pixel-by-pixel, tap-by-tap sums: bit-equal on exact data, to float64 rounding on
    float data; the data gradient as a forward convolution of the zero-inserted dy (the emulation's route) likewise"""
    d = cc.exact_case(geom, 8, 12, seed=5)
    y, dx = cc.forward_reference(d["x"], d["w"], geom), cc.dgrad_reference(d["dy"], d["w"], geom)
    assert y.dtype == torch.float64 and y.shape == d["dy"].shape and dx.shape == d["x"].shape
    assert torch.equal(y, cc.loop_forward(d["x"], d["w"], geom)) and float(y.abs().max()) > 0
    assert torch.equal(dx, cc.loop_dgrad(d["dy"], d["w"], geom)) and float(dx.abs().max()) > 0
    z, wf, gf = cc.dgrad_as_forward(d["dy"], d["w"], geom)
    assert torch.equal(cc.forward_reference(z, wf, gf), dx)
    unread = torch.from_numpy(cc.unread_pixels(geom))
    assert float(dx[:, unread].abs().max() if bool(unread.any()) else 0.0) == 0.0
    f = cc.float_case(geom, 8, 12, seed=6)
    assert float(f["x"].min()) == 0.0
    for ref, loop, a in ((cc.forward_reference(f["x"], f["w"], geom), cc.loop_forward(f["x"], f["w"], geom),
                          cc.forward_reference(f["x"].abs(), f["w"].abs(), geom)),
                         (cc.dgrad_reference(f["dy"], f["w"], geom), cc.loop_dgrad(f["dy"], f["w"], geom),
                          cc.dgrad_reference(f["dy"].abs(), f["w"].abs(), geom))):
        assert bool(((ref - loop).abs() <= 128 * 2.0 ** -53 * a).all()) and bool((ref.abs() <= a * (1 + 1e-12)).all())


@pytest.mark.parametrize("case", cc.EXACT_CASES + [(cc.PAIR_CASE[0],) + ch for ch in cc.PAIR_CASE[1:]], ids=cc.case_id)
def test_exact_cases_are_exact_in_fp32(case):
    """256 K (+ the epilogue's terms) <= 2^24 units, every reference value an integer number of its channel's unit within
    that count, and float32(ref64) == ref64 elementwise -- for the plain, biased, accumulated and eval-folded forms"""
    g, cin, cout = case
    d = cc.exact_case(g, cin, cout, seed=11)
    for dgrad in (False, True):
        assert 256 * cc.k_terms(g, cin, cout, dgrad) <= 2 ** 24
        assert 256 * cc.k_terms(g, cin, cout, dgrad) + cc.EXTRA_UNITS <= 2 ** 24
    y, dx = cc.forward_reference(d["x"], d["w"], g), cc.dgrad_reference(d["dy"], d["w"], g)
    uo, ui = torch.from_numpy(cc.unit_scale(cout)) / 4, torch.from_numpy(cc.unit_scale(cin)) / 4
    b, base, sc, sh = d["bias"].double(), d["base"].double(), d["scale"].double(), d["shift"].double()
    forms = [(y, uo, 0), (y + b, uo, 16), (torch.relu(y + b), uo, 16), (y + b + base, uo, 32),
             (torch.relu(y * sc + sh), uo * sc, 16), (dx, ui, 0), (dx + d["dbase"].double(), ui, 16)]
    for i, (ref, unit, extra) in enumerate(forms):
        assert torch.equal(ref.float().double(), ref), i
        units = ref / unit
        assert float(units.frac().abs().max()) == 0, i
        assert float(units.abs().max()) <= 256 * cc.k_terms(g, cin, cout, i >= 5) + extra, i
    assert float(y.abs().max()) > 0 and float(dx.abs().max()) > 0
    unread = torch.from_numpy(cc.unread_pixels(g))
    if bool(unread.any()):
        assert float(dx[:, unread].abs().max()) == 0.0
    assert float(d["x"].abs().max()) == 4 and float((d["w"].double() * 16).frac().abs().max()) == 0


def test_float_bound_holds_for_the_emulated_fp32_reference():
    """a sequential fp32 sum of the float case's own products against float64 (16 channels over every scale): in the kernels' K
    order a decade inside TOL, in the worst order (the measurement TOL was taken from) inside TOL / 4 with little to spare"""
    sel = list(range(0, 96, 6))
    worst, korder = cc.measure_reference_error("worst", sel), cc.measure_reference_error("k", sel)
    print("emulated fp32 / A: worst order %s, K order %s, TOL %.2e" % (worst, korder, cc.TOL))
    for key in ("forward", "dgrad"):
        assert 0 < korder[key] <= cc.TOL / 10
        assert korder[key] < worst[key] <= cc.TOL / 4
    assert max(worst.values()) >= cc.TOL / 8                      # the margin is the stated factor 4, not more than 8
    assert 2.0 ** -23 <= cc.TOL                                   # reduce_reference: two fp32 roundings of xhat
    from tests.bf16x_emu import ACC_REL
    assert max(korder.values()) <= ACC_REL                        # the project's constant holds for these cases' K order


def pick_tile(M, cout, K):
    """tbn_conv_pick_tile restated"""
    best, pick = 1e300, (1, 1)
    for mt in (1, 2):
        for nt in (1, 2, 3, 4):
            blocks = float(-(-M // (128 * mt)) * -(-cout // (32 * nt)))
            rounds = float(int((blocks + 255) / 256))
            cost = rounds * ((K / 32.0) * (mt * nt * 1024.0 + 350.0) + 4000.0)
            cost *= 1.0 + 0.01 / (mt * nt)
            if cost < best:
                best, pick = cost, (mt, nt)
    return pick


def test_geometry_table_reaches_every_mechanism_it_names():
    props = set()
    for g in cc.GEOMS:
        n, h, w, k, s, p = g
        oh, ow = cc.out_hw(g)
        assert oh >= 1 and ow >= 1
        for dgrad in (False, True):
            M = cc.rows(g, dgrad)
            side = "dgrad" if dgrad else "fwd"
            if M < 32:
                props.add("M below one split-K tile")
            if 32 < M < 128:
                props.add("M below one 128-row tile")
            if M > 256 and M % 128 and M % 256:
                props.add("M ragged against 128 and 256")
            if s == 1 and n >= 3 and (h, w) in ((3, 3), (5, 3)) and cc.frame_boundaries_in_tile(g, dgrad, 32):
                props.add("frame boundary inside a tile, %dx%d" % (h, w))
                assert len(cc.frame_boundaries_in_tile(g, dgrad, 128)) == n - 1
            # the map the kernel walks: the output pixels (forward), the input pixels (data gradient)
            mh, mw = (h, w) if dgrad else (oh, ow)
            if mw == 1 and mh > 1:
                props.add("OW == 1 " + side)
            if mh == 1 and mw > 1:
                props.add("OH == 1 " + side)
            if mh * mw == 1:
                props.add("OH*OW == 1 " + side)
        halo = (k, s, p) == (3, 1, 1)
        fams = {f for f, _ in variants_for(k, s, p, w, dgrad=False)}
        assert (HALO in fams) == (halo and w <= 64) and {0, DMA, SK4} <= fams
        dfams = {f for f, _ in variants_for(k, s, p, ow, dgrad=True)}
        assert dfams == ({0} if s == 2 else fams)
        if halo and w == 64:
            props.add("halo limit")
        if halo and w == 65:
            props.add("past the halo limit")
        if halo and w + 1 > w * h:
            props.add("halo reach beyond a frame")
        if halo and w == 1:
            props.add("narrower than the halo reach")
        if (k, s) == (3, 1):
            props.add("3x3 / stride 1 / pad %d" % p)
        if (k, s, p) == (1, 1, 0):
            props.add("pointwise")
        if s == 2:
            ph = cc.phases(g)
            sizes = [q["M"] for q in ph]
            assert sum(sizes) == n * h * w
            # parity_tap: 3x3 taps per axis -- pad 1: 1 | 2, pad 0 and 2: 2 | 1; 1x1: 1 | 0
            per_axis = [len(cc.parity_taps(par, k, p)) for par in (0, 1)]
            assert per_axis == {(3, 0): [2, 1], (3, 1): [1, 2], (3, 2): [2, 1], (1, 0): [1, 0]}[(k, p)]
            assert [q["taps"] for q in ph] == [per_axis[a] * per_axis[b] for a in (0, 1) for b in (0, 1)]
            assert sum(q["taps"] * q["M"] for q in ph) > 0
            tag = "%dx%d / stride 2 / pad %d" % (k, k, p)
            if h % 2 == 1 and w % 2 == 0 and h > 1:
                assert len(set(sizes)) == 2 and ph[0]["M"] > ph[2]["M"]
                props.add(tag + ", odd x even")
            if h % 2 == 1 and w % 2 == 1 and min(h, w) > 1:
                assert len(set(sizes)) == 4
                props.add("four parity sizes")
            if h == 1:
                assert [q["M"] > 0 for q in ph] == [True, True, False, False]
                props.add(tag + ", one-row map")
            if w == 1:
                assert [q["M"] > 0 for q in ph] == [True, False, True, False]
                props.add("one-column map under stride 2")
            if k == 1:
                assert [q["launches"] for q in ph] == [True, False, False, False]
                if sum(q["M"] > 0 and q["taps"] == 0 for q in ph) == 3:
                    props.add("three parities with pixels and no tap")
            else:
                assert [q["launches"] for q in ph] == [q["M"] > 0 for q in ph]
            if max(q["M"] for q in ph if q["launches"]) > 128:
                props.add("two M tiles in a phase" + (" of the 1x1" if k == 1 else ""))
        unread = cc.unread_pixels(g)
        if unread.any():
            assert s == 2
            if p == 0 and k == 3 and unread[-1].all() and unread[:, -1].all():
                props.add("unread last row and column")
            elif p == 0 and k == 3 and unread[:, -1].all():
                props.add("unread last column")
    need = {"M below one split-K tile", "M below one 128-row tile", "M ragged against 128 and 256",
            "frame boundary inside a tile, 3x3", "frame boundary inside a tile, 5x3",
            "OW == 1 fwd", "OW == 1 dgrad", "OH == 1 fwd", "OH == 1 dgrad", "OH*OW == 1 fwd", "OH*OW == 1 dgrad",
            "halo limit", "past the halo limit", "halo reach beyond a frame", "narrower than the halo reach",
            "3x3 / stride 1 / pad 0", "3x3 / stride 1 / pad 1", "3x3 / stride 1 / pad 2", "pointwise",
            "3x3 / stride 2 / pad 0, odd x even", "3x3 / stride 2 / pad 1, odd x even", "3x3 / stride 2 / pad 2, odd x even",
            "1x1 / stride 2 / pad 0, odd x even", "3x3 / stride 2 / pad 1, one-row map", "3x3 / stride 2 / pad 2, one-row map",
            "1x1 / stride 2 / pad 0, one-row map", "one-column map under stride 2", "four parity sizes",
            "three parities with pixels and no tap", "two M tiles in a phase", "two M tiles in a phase of the 1x1",
            "unread last column", "unread last row and column"}
    assert props >= need, sorted(need - props)
    # the table the GPU test runs: every geometry, every channel pair, every tile of every family somewhere
    assert {c[0] for c in cc.EXACT_CASES} == set(cc.GEOMS) and len(set(cc.EXACT_CASES)) == len(cc.EXACT_CASES)
    assert {c[1:] for c in cc.EXACT_CASES} == set(cc.CHANNELS)
    assert all(c in cc.EXACT_CASES for c in cc.SHORT_K) and all(c[0] in cc.GEOMS for c in cc.FLOAT_CASES)
    # channels ragged under the wide tiles; K of one and two chunks for the four waves of the split-K tile kernel
    assert {co % (32 * nt) != 0 for _, co in cc.CHANNELS for nt in (2, 3, 4)} == {True, False}
    assert all(any(c % (32 * nt) for ci, co in cc.CHANNELS for c in (ci, co)) for nt in (2, 3, 4))
    assert sorted(cc.k_terms(g, ci, co, False) // 32 for g, ci, co in cc.SHORT_K) == [1, 2]
    seen = set()
    for g, ci, co in cc.EXACT_CASES:
        for dgrad in (False, True):
            wk = cc.out_hw(g)[1] if dgrad else g[2]
            for flags, stages in variants_for(g[3], g[4], g[5], wk, dgrad):
                seen |= {(dgrad, g[4] == 2 and dgrad, flags, stages, t) for t in tiles_for(flags)}
    want = {(dg, False, f, st, t) for dg in (False, True) for f, st in ((0, 1), (0, 2), (HALO, 0), (DMA, 0), (SK4, 0))
            for t in tiles_for(f)} | {(True, True, 0, st, t) for st in (1, 2) for t in tiles_for(0)}
    assert seen == want
    assert len(tiles_for(0)) == 8 and len(tiles_for(SK4)) == 4


@pytest.mark.parametrize("geom", cc.GEOMS, ids=lambda g: "n%d_%dx%d_k%ds%dp%d" % g)
def test_partial_rows_counted_are_the_rows_a_launch_writes(geom):
    """tbn_conv_partial_rows (every family's tile height, single and pair launches, forward statistics and the
    data-gradient reduce) and tbn_conv2d_stat_tiles against the M tiles of the launch restated in Python: for a strided data
    gradient the tiles of the parity phases that LAUNCH -- a parity with pixels and no tap (1x1 / stride 2) writes no row"""
    L = lib()
    n, h, w, k, s, p = geom
    for cin, cout in cc.CHANNELS:
        for mt in (1, 2):
            for flags, pair in ((0, 0), (HALO, 0), (DMA, 0), (SK4, 0), (0, 1), (SK4, 1)):
                tile_rows = (32 if flags == SK4 and not pair else 128) * mt
                got = L.tbn_conv_partial_rows(C.byref(desc(geom, cin, cout, False, flags)), mt, pair)
                assert got == cc.rows_written(geom, False, tile_rows), ("fwd", cin, cout, mt, flags, pair)
                if s == 2 and (flags or pair):
                    continue       # a strided data gradient is the parity-phase launch of the generic kernel
                got = L.tbn_conv_partial_rows(C.byref(desc(geom, cin, cout, True, flags)), mt, pair)
                assert got == cc.rows_written(geom, True, tile_rows), ("dgrad", cin, cout, mt, flags, pair)
        M = cc.rows(geom, False)
        mt, nt = pick_tile(M, cout, cc.k_terms(geom, cin, cout, False))
        tiles = L.tbn_conv2d_stat_tiles(n, h, w, cin, cout, k, s, p)
        assert tiles == cc.rows_written(geom, False, 128 * mt) == L.tbn_conv_partial_rows(C.byref(desc(geom, cin, cout, False)), mt, 0)
    if s == 2:
        launched = [q for q in cc.phases(geom) if q["launches"]]
        assert cc.rows_written(geom, True, 128) == sum(-(-q["M"] // 128) for q in launched) >= 1


def test_entries_refuse_a_bad_input_pitch_before_any_launch():
    """in_ld below the channel count the kernels read per pixel, or not a multiple of 4 floats (their float4 loads): refused by
    every C-ABI conv entry on the host -- no device is present here, so a call that got further would fail differently"""
    L = lib()
    g = (2, 8, 8, 3, 1, 1)

    def fails(rc, needle):
        assert rc < 0, rc
        assert needle in L.tbn_last_error().decode(), L.tbn_last_error()

    def fwd(in_ld):
        return L.tbn_conv2d_fwd(BAD, in_ld, BAD, None, BAD, 64, 2, 8, 8, 32, 64, 3, 1, 1, 0, 0, None, None, None, None)

    def fwd_tile(in_ld):
        return L.tbn_conv2d_fwd_tile(BAD, in_ld, BAD, None, BAD, 64, 2, 8, 8, 32, 64, 3, 1, 1, 0, 0, None, 1, 1, None)

    def dgrad(dout_ld):
        return L.tbn_conv2d_dgrad(BAD, dout_ld, BAD, BAD, 32, 2, 8, 8, 32, 64, 3, 1, 1, 0, BAD, None)

    for f, who, c in ((fwd, "conv2d_fwd", 32), (fwd_tile, "conv2d_fwd_tile", 32), (dgrad, "conv2d_dgrad", 64)):
        for ld in (c - 4, c + 2, 0, -c):
            fails(f(ld), "%s: in_ld %d (at least the %d input channels, a multiple of 4)" % (who, ld, c))
    for dg, c in ((False, 32), (True, 64)):
        for ld in (c - 4, c + 2, 0):
            fails(L.tbn_conv_launch(C.byref(desc(g, 32, 64, dg, in_ld=ld)), 1, 1, BAD, None),
                  "conv_launch: in_ld %d (at least the %d input channels" % (ld, c))
            fails(L.tbn_conv_launch_pair(C.byref(desc(g, 32, 64, dg, in_ld=ld)), C.byref(desc(g, 32, 64, dg)), 1, 1, 1, BAD, BAD,
                                         None), "conv_launch: in_ld %d" % ld)


def test_the_comparison_is_not_blind():
    """two wrong results the older yardstick (1e-4 of the tensor's maximum) cannot both see: one tap dropped at one border
    pixel, and one small-scale channel off by 1e-4 of the global maximum.  The exact and the per-element rules reject both."""
    g, cin, cout = (2, 7, 7, 3, 1, 1), 32, 32
    # one tap dropped at one border pixel: pixel (0, 0, 6) loses tap (r, s) = (2, 0), i.e. input pixel (1, 5)
    for make, exact in ((cc.exact_case, True), (cc.float_case, False)):
        d = make(g, cin, cout, seed=3)
        ref = cc.forward_reference(d["x"], d["w"], g)
        a = cc.forward_reference(d["x"].abs(), d["w"].abs(), g)
        assert cc.float_ratio(ref.float(), ref, a) <= 1.0 and (not exact or cc.exact_ok(ref.float(), ref))
        wrong = ref.clone()
        wrong[0, 0, 6] -= d["w"].double()[:, 2, 0, :] @ d["x"].double()[0, 1, 5]
        assert int((wrong != ref).sum()) >= cout // 2
        assert cc.float_ratio(wrong.float(), ref, a) > 1e3
        if exact:
            assert not cc.exact_ok(wrong.float(), ref)
        # the same for the data gradient: input pixel (1, 0, 0) loses what output pixel (0, 0) sent it through tap (1, 1)
        dref = cc.dgrad_reference(d["dy"], d["w"], g)
        da = cc.dgrad_reference(d["dy"].abs(), d["w"].abs(), g)
        dwrong = dref.clone()
        dwrong[1, 0, 0] -= d["dy"].double()[1, 0, 0] @ d["w"].double()[:, 1, 1, :]
        assert cc.float_ratio(dref.float(), dref, da) <= 1.0 and cc.float_ratio(dwrong.float(), dref, da) > 1e3
        if exact:
            assert cc.exact_ok(dref.float(), dref) and not cc.exact_ok(dwrong.float(), dref)
    # a small-scale channel off by 0.9e-4 of the global maximum in every pixel: the old yardstick accepts it
    d = cc.float_case(g, cin, cout, seed=3)
    ref = cc.forward_reference(d["x"], d["w"], g)
    a = cc.forward_reference(d["x"].abs(), d["w"].abs(), g)
    small = int(np.argmin(cc.channel_scale(cout)))
    wrong = ref.clone()
    wrong[..., small] += 0.9e-4 * float(ref.abs().max())
    assert cc.old_yardstick(wrong, ref) < 1e-4
    assert float(ref[..., small].abs().max()) < 1e-2 * float(ref.abs().max())
    assert cc.float_ratio(wrong.float(), ref, a) > 10
    # and the per-channel sums: the same offset reaches s1 of that channel only
    b1, b2 = cc.stat_bounds(a)
    s1_err = (wrong - ref).reshape(-1, cout).sum(0).abs()
    assert float(s1_err[small]) > 10 * float(b1[small]) and float(b2.min()) > 0
    # an element without any term must be exactly zero
    z, za = torch.zeros(2, 3), torch.zeros(2, 3)
    assert cc.float_ratio(z.float(), z.double(), za.double()) == 0.0
    assert cc.float_ratio(z.float() + 1e-30, z.double(), za.double()) == float("inf")
