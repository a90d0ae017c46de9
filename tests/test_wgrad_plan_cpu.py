"""Host-side checks of the weight-gradient operator tests (no GPU): the two float64 references of tests/wgrad_check.py
against an explicit pixel / tap loop, and a CENSUS of the GPU test's own case table through tbn_conv2d_wgrad_plan -- which
kernel instantiation, split-K plan and reduce each case runs, and which edges of the kernel's row arithmetic it reaches.  A
change to the planner that silently takes a tile, a mode, the split-K path or a reduce variant out of the GPU test's reach
fails here."""
import ctypes as C

import pytest
import torch

from attention_based_tbn_amd._lib import lib
from tests import wgrad_check as wc


@pytest.mark.parametrize("geom", [(2, 5, 4, 3, 2, 1), (3, 4, 3, 3, 1, 0), (2, 3, 5, 1, 2, 0), (1, 6, 7, 5, 1, 2)])
def test_references_agree_with_an_explicit_loop(geom):
    """unfold + einsum against the pixel-by-pixel, tap-by-tap sum: bit-equal on exact data (every partial sum is exact in
    float64 too), to float64 rounding on Gaussian data; abs_reference likewise, and it bounds |reference| entry by entry"""
    dy, x = wc.exact_case(geom, 8, 12, seed=5)
    ref = wc.reference(dy, x, geom)
    assert ref.shape == (12, geom[3], geom[3], 8) and ref.dtype == torch.float64
    assert torch.equal(ref, wc.loop_reference(dy, x, geom))
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) > 0
    assert torch.equal(wc.abs_reference(dy, x, geom), wc.loop_reference(dy.abs(), x.abs(), geom))
    dy, x = wc.float_case(geom, 8, 12, seed=6)
    ref, a = wc.reference(dy, x, geom), wc.abs_reference(dy, x, geom)
    assert float(x.min()) == 0.0 and float(x.double().mean()) > 0
    assert ((ref - wc.loop_reference(dy, x, geom)).abs() <= 64 * 2.0 ** -53 * a).all()
    assert ((a - wc.loop_reference(dy.abs(), x.abs(), geom)).abs() <= 64 * 2.0 ** -53 * a).all()
    assert (ref.abs() <= a).all()


def test_case_table_holds_what_the_operator_tests_promise():
    """the table itself: every geometry x channel pair of the issue at the heuristic tile (bar the widest pair under the
    5x5 / 7x7 filters), every tile on four geometries, exact data exact in fp32 (16 * M <= 2^24), channel scales over 2^10"""
    for table in (wc.EXACT_CASES, wc.TILE_CASES, wc.FLOAT_CASES):
        assert len({wc.case_id(c) for c in table}) == len(table)
    assert len(wc.TILES) == 11 and (5, 3) not in wc.TILES
    for g in wc.GEOMS:
        for ch in wc.CHANNELS:
            assert (g, ch[0], ch[1], (0, 0)) in wc.EXACT_CASES or (g[3] > 3 and ch == (100, 164))
    assert {(c[0], c[3]) for c in wc.TILE_CASES} == {(g, t) for g in wc.TILE_GEOMS for t in wc.TILES}
    for g, cin, cout, _ in wc.ALL_CASES:
        assert cin % 4 == 0 and cout % 4 == 0 and 16 * wc.rows(g) <= 2 ** 24
    s = wc.channel_scale(164)
    assert s.min() == 2.0 ** -5 and s.max() == 2.0 ** 5
    dy, x = wc.exact_case((2, 6, 6, 3, 1, 1), 36, 44, seed=1)
    assert dy.dtype == torch.float32 and float((dy.double() * 32).frac().abs().max()) == 0 and float(dy.abs().max()) == 4 * 32
    assert float((x.double() * 32).frac().abs().max()) == 0


def test_census_of_the_gpu_case_table():
    L = lib()
    seen, reduces, props = set(), set(), set()
    for case in wc.ALL_CASES:
        g, cin, cout, tile = case
        n, h, w, k, stride, pad = g
        q = wc.plan(L, g, cin, cout, tile)
        M, (oh, ow) = wc.rows(g), wc.out_hw(g)
        assert tile == (0, 0) or (q["mt"], q["nt"]) == tile, case
        assert (q["mt"], q["nt"]) in wc.TILES
        assert q["mode"] == (2 if (k, stride, pad) == (1, 1, 0) else 0)
        assert q["rows_per_split"] % 64 == 0 and (q["splits"] - 1) * q["rows_per_split"] < M <= q["splits"] * q["rows_per_split"]
        assert q["tiles_co"] == -(-cout // (32 * q["mt"])) and q["tiles_ci"] == -(-cin // (32 * q["nt"]))
        assert q["ws_floats"] == (q["splits"] * cout * k * k * cin if q["splits"] > 1 else 0)
        assert (q["reduce"] == 0) == (q["splits"] == 1) and q["reduce"] in (0, 4, 16)
        # the workspace the GPU test allocates (the public size query: worst case over the tiles) covers the tile run
        assert q["ws_floats"] <= L.tbn_conv2d_wgrad_workspace_floats(n, h, w, cin, cout, k, stride, pad)
        split = q["splits"] > 1
        seen.add((q["mt"], q["nt"], q["mode"], split))
        reduces.add(q["reduce"])
        if q["mode"] == 0:
            ohw = oh * ow
            if ohw < 64 and 64 % ohw != 0:
                props.add("short frames, r64 != 0")
                if split:
                    props.add("short frames, r64 != 0, split-K")
            if ow == 1 and oh > 1:
                props.add("OW == 1")
            if ohw == 1:
                props.add("OH*OW == 1")
            if split and q["splits"] * q["rows_per_split"] - M >= ohw:
                props.add("last split runs a whole frame past frame N")
            if stride == 2 and (h % 2 == 1 or w % 2 == 1):
                props.add("stride 2, odd map")
            if k == 1 and stride == 2:
                props.add("strided 1x1")
            if k == 3 and pad == 0:
                props.add("valid 3x3")
            if k > 3:
                props.add("filter above 3x3")
        if M < 64:
            props.add("fewer rows than one step")
        if cout % (32 * q["mt"]):
            props.add("ragged co tile")
        if cin % (32 * q["nt"]):
            props.add("ragged ci tile")
        if cin % 32 and cout % 32:
            props.add("channels not multiples of 32")
    want = {(mt, nt, mode, split) for mt, nt in wc.TILES for mode in (0, 2) for split in (False, True)}
    assert seen >= want, sorted(want - seen)
    assert reduces == {0, 4, 16}
    need = {"short frames, r64 != 0", "short frames, r64 != 0, split-K", "OW == 1", "OH*OW == 1",
            "last split runs a whole frame past frame N", "stride 2, odd map", "strided 1x1", "valid 3x3", "filter above 3x3",
            "fewer rows than one step", "ragged co tile", "ragged ci tile", "channels not multiples of 32"}
    assert props >= need, sorted(need - props)
    # the reduce variant with 16 slab lanes: the many-slab case, with an odd slab count
    q = wc.plan(L, *wc.MANY_SLABS, (0, 0))
    assert (q["mt"], q["nt"], q["mode"], q["splits"], q["rows_per_split"], q["reduce"]) == (1, 1, 2, 33, 256, 16)
    # both float cases run split-K
    assert all(wc.plan(L, g, ci, co, t)["splits"] > 1 for g, ci, co, t in wc.FLOAT_CASES)
    assert {wc.plan(L, g, ci, co, t)["mode"] for g, ci, co, t in wc.FLOAT_CASES} == {0, 2}


def test_plan_query_agrees_with_the_existing_entries():
    """the plan the query reports is the plan the existing callers get: the public workspace size is the worst case of the
    query over the tiles, and the heuristic tile is the one tests/test_kernels_gpu.py::test_wgrad_every_heuristic_tile
    documents (pick_wtile, the cout == 160 rule, 5x3 -> 5x2) and the engine's layers run"""
    L = lib()
    table = {32: 1, 64: 2, 96: 3, 160: 5}
    for (k, pad), mode in (((3, 1), 0), ((1, 0), 2)):
        for cout in (32, 64, 96, 160):
            for cin in (32, 64, 96):
                q = wc.plan(L, (2, 6, 6, k, 1, pad), cin, cout, (0, 0))
                want = (table[cout], 2 if (cout, cin) == (160, 96) else table[cin])
                assert (q["mt"], q["nt"], q["mode"], q["splits"]) == want + (mode, 1)
    # narrow extents take 32-wide tiles, wide ones 64-wide unless that pads the input channels by 12 % or more (100, 160, 224)
    for cin, cout, want in ((4, 8, (1, 1)), (36, 44, (1, 1)), (100, 164, (2, 1)), (160, 192, (2, 1)), (224, 128, (2, 1)),
                            (1056, 384, (2, 2))):
        q = wc.plan(L, (2, 8, 8, 1, 1, 0), cin, cout, (0, 0))
        assert (q["mt"], q["nt"]) == want, (cin, cout, q)
    geoms = wc.GEOMS + [wc.MANY_SLABS[0], (8, 28, 28, 3, 1, 1), (16, 56, 56, 3, 1, 1), (32, 28, 28, 1, 1, 0)]
    for g in geoms:
        for cin, cout in wc.CHANNELS + [(32, 32), (192, 160)]:
            worst = max(wc.plan(L, g, cin, cout, t)["ws_floats"] for t in wc.TILES)
            assert worst == L.tbn_conv2d_wgrad_workspace_floats(g[0], g[1], g[2], cin, cout, g[3], g[4], g[5]), (g, cin, cout)
            # an explicit request for the heuristic's tile is the heuristic's plan
            q0 = wc.plan(L, g, cin, cout, (0, 0))
            assert wc.plan(L, g, cin, cout, (q0["mt"], q0["nt"])) == q0
    # the split-K plans two tests of tests/test_kernels_gpu.py rely on (a split-K path; at least 16 slabs)
    assert wc.plan(L, (8, 28, 28, 3, 1, 1), 64, 64, (0, 0))["splits"] > 1
    assert wc.plan(L, (16, 56, 56, 3, 1, 1), 64, 96, (0, 0))["splits"] >= 16
    # Linear layers are 1x1 convs over an (m, 1, 1, k) image
    q = wc.plan(L, (70, 1, 1, 1, 1, 0), 36, 44, (0, 0))
    assert q["mode"] == 2 and L.tbn_linear_wgrad_workspace_floats(70, 36, 44) == L.tbn_conv2d_wgrad_workspace_floats(70, 1, 1, 36, 44, 1, 1, 0)


def test_plan_query_and_tile_entry_refuse_before_any_device_call():
    L = lib()
    bad = 0x1000   # never dereferenced: validation fails first
    out = (C.c_int * 8)()

    def fails(rc, needle):
        assert rc < 0, rc
        assert needle in L.tbn_last_error().decode(), L.tbn_last_error()

    def plan(n=2, h=6, w=6, cin=36, cout=44, k=3, stride=1, pad=1, mt=0, nt=0, o=out):
        return L.tbn_conv2d_wgrad_plan(n, h, w, cin, cout, k, stride, pad, mt, nt, o)

    def tile(dy=bad, dy_ld=44, x=bad, x_ld=36, dw=bad, n=2, h=6, w=6, cin=36, cout=44, k=3, stride=1, pad=1, mt=0, nt=0):
        return L.tbn_conv2d_wgrad_tile(dy, dy_ld, x, x_ld, dw, n, h, w, cin, cout, k, stride, pad, mt, nt, None, None)
    assert plan() == 0
    fails(plan(o=None), "conv2d_wgrad_plan: null out")
    for kw in (dict(dy=None), dict(x=None), dict(dw=None)):
        fails(tile(**kw), "conv2d_wgrad_tile: null pointer")
    for f, who in ((plan, "conv2d_wgrad_plan"), (tile, "conv2d_wgrad_tile")):
        for mt, nt in ((4, 1), (5, 3), (0, 2), (2, 0), (1, 4), (1, 5), (6, 1), (-1, 1), (1, -1)):
            fails(f(mt=mt, nt=nt), "%s: tile %dx%d (mt 1 | 2 | 3 | 5, nt 1..3 without 5x3, or 0x0)" % (who, mt, nt))
        fails(f(cin=34), who + ": cin 34 / cout 44 must be multiples of 4")
        fails(f(cout=42), who + ": cin 36 / cout 42 must be multiples of 4")
        fails(f(cin=0), who + ": cin 0")
        fails(f(n=0), who + ": bad shape")
        fails(f(h=2, pad=0), who + ": bad shape")
        fails(f(stride=0), who + ": bad shape")
    fails(tile(dy_ld=40), "conv2d_wgrad_tile: dout_ld 40 (at least cout, a multiple of 4)")
    fails(tile(dy_ld=46), "conv2d_wgrad_tile: dout_ld 46")
    fails(tile(x_ld=32), "conv2d_wgrad_tile: in_ld 32 (at least cin, a multiple of 4)")
    fails(tile(x_ld=38), "conv2d_wgrad_tile: in_ld 38")
    # the launcher's own limits, ahead of the launch: 32-bit buffer extents, and the 24-bit multiplies of the row arithmetic
    fails(tile(n=2, h=64, w=64, x_ld=1 << 18), "wgrad: operand extent >= 2 GiB")
    fails(tile(n=2, h=64, w=64, dy_ld=1 << 18), "wgrad: operand extent >= 2 GiB")
    fails(tile(n=1, h=3, w=3, x_ld=1 << 22), "wgrad: feature map too large for the 24-bit row arithmetic")
    fails(tile(n=1, h=2, w=1 << 23, k=1, pad=0), "wgrad: operand extent >= 2 GiB")
    fails(tile(n=3, h=9, w=11, k=1, pad=0), "wgrad: split-K needs a workspace")     # (this helper passes none)
