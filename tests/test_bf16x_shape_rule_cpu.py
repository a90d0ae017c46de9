"""The split-bf16 shape rule (csrc/tbn_kernels.h: bf16x_layer_kind, bf16x_3x3_map_ok) seen through the C ABI, without a GPU:
which (ksize, stride, pad, cin, map width) the kernels of conv_bf16x.hip take, as tbn_conv_weight_planes_bytes and the
refusals of tbn_conv_launch report it.  No call here launches anything: a launch the rule ACCEPTS is given the tile (3, 1),
which the launcher refuses after it has classified the shape ("unsupported bf16x tile"); one the rule rejects is refused
with the geometry message before that.  The pointers are never dereferenced."""
import ctypes as C

import pytest

BF16X6, BF16X3, PLANES = 32, 64, 128
UNSUPPORTED = -3
ACCEPTED = "unsupported bf16x%d tile 3x1"
PRECHECK = "need stride 1 and cin a multiple of 32"
ONLY_3X3 = "kernel handles 3x3 / stride 1 / pad 1 layers on maps at most 64 wide"
ON_PLANES = "kernels on weight planes (flag 128) handle 3x3 / stride 1 / pad 1 layers on maps at most 64 wide and 1x1"


def _launch(flags, k, stride, pad, cin, w):
    from attention_based_tbn_amd._lib import ConvDesc, lib
    bad = 0x1000
    d = ConvDesc()
    d.inp, d.in_ld, d.weight, d.out, d.out_ld = bad, cin, bad, bad, 64
    d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = 1, 4, w, cin, 64, k, stride, pad
    d.flags = flags
    rc = lib().tbn_conv_launch(C.byref(d), 3, 1, None, None)
    return rc, lib().tbn_last_error().decode()


def test_weight_planes_exist_for_exactly_the_layers_the_rule_takes():
    from attention_based_tbn_amd._lib import lib
    L = lib()
    for np_, per in ((6, 6), (3, 4)):
        assert L.tbn_conv_weight_planes_bytes(64, 1, 32, np_) == 64 * 32 * per
        assert L.tbn_conv_weight_planes_bytes(64, 3, 32, np_) == 64 * 9 * 32 * per
        assert L.tbn_conv_weight_planes_bytes(64, 3, 96, np_) == 64 * 9 * 96 * per
        for k in (1, 3):
            assert L.tbn_conv_weight_planes_bytes(64, k, 48, np_) == 0      # cin not a multiple of 32
            assert L.tbn_conv_weight_planes_bytes(64, k, 0, np_) == 0
        for k in (0, 2, 5, 7):
            assert L.tbn_conv_weight_planes_bytes(64, k, 32, np_) == 0      # no split-bf16 kernel for this filter
    assert L.tbn_conv_weight_planes_bytes(64, 3, 32, 4) == 0
    # the split refuses the same arguments before it looks at the pointers' contents
    for k, cin in ((5, 32), (3, 48)):
        assert L.tbn_conv_split_weights(0x1000, 64, k, cin, 6, 0x1000, None) < 0
        assert "bf16x" in L.tbn_last_error().decode()


@pytest.mark.parametrize("flag,np_", [(BF16X6, 6), (BF16X3, 3)])
def test_launch_refusals_follow_the_rule(flag, np_):
    f = flag | PLANES
    # on weight planes: 3x3 / stride 1 / pad 1 up to 64 wide, 1x1 / stride 1 / pad 0 at any width
    for geom in ((3, 1, 1, 32, 64), (3, 1, 1, 32, 11), (1, 1, 0, 32, 64), (1, 1, 0, 32, 65), (1, 1, 0, 96, 200)):
        rc, msg = _launch(f, *geom)
        assert rc == UNSUPPORTED and ACCEPTED % np_ in msg, (geom, rc, msg)
    for geom in ((3, 1, 1, 32, 65), (3, 1, 0, 32, 64), (1, 1, 1, 32, 11)):       # too wide, wrong padding
        rc, msg = _launch(f, *geom)
        assert rc == UNSUPPORTED and ON_PLANES in msg and "bf16x%d" % np_ in msg, (geom, rc, msg)
    for geom in ((3, 2, 1, 32, 12), (1, 2, 0, 32, 12), (1, 1, 0, 48, 11), (3, 1, 1, 16, 11)):   # stride 2, cin % 32 != 0
        rc, msg = _launch(f, *geom)
        assert rc == UNSUPPORTED and PRECHECK in msg and "bf16x" in msg, (geom, rc, msg)
    # a 5x5 filter reaches no split-bf16 kernel in either form: the generic launcher refuses filters larger than 3x3
    # before the bf16x classifier sees them (as it always did), so this refusal carries its text and code, not a bf16x one
    for flags in (f, flag):
        rc, msg = _launch(flags, 5, 1, 2, 32, 11)
        assert rc < 0 and "filters larger than 3x3" in msg, (flags, rc, msg)
    # weights split while staging (no flag 128): the 3x3 kernel only
    for geom in ((3, 1, 1, 32, 64), (3, 1, 1, 64, 11)):
        rc, msg = _launch(flag, *geom)
        assert rc == UNSUPPORTED and ACCEPTED % np_ in msg, (geom, rc, msg)
    for geom in ((3, 1, 1, 32, 65), (1, 1, 0, 32, 11), (3, 2, 1, 32, 12), (3, 1, 0, 32, 11)):
        rc, msg = _launch(flag, *geom)
        assert rc == UNSUPPORTED and ONLY_3X3 in msg and "bf16x%d" % np_ in msg, (geom, rc, msg)
