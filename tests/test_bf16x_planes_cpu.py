"""CPU checks of the pointwise split-bf16 math and the weight-plane records (tests/bf16x_pw_emu.py): the error of the emulated
1x1 bf16x6 / bf16x3 products against fp64 on the shapes the GPU tests use, the cancellation problem, the record layout, and
the parts of the C-ABI that need the library but no GPU (sizes, capability bit, binding of the appended struct fields)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.bf16x_emu import ACC_REL, X3_REL, split
from tests.bf16x_pw_emu import PW_CASES, plane_records, pw_abs_conv, pw_cancel_problem, pw_emulated

TOL = 1e-4   # the operator tolerance of tests/test_conv_variants_gpu.py (of the tensor's maximum)


def _problem(case, seed=61):
    """inputs distributed as tests/test_conv_variants_gpu.py Problem draws them"""
    n, h, w, cin, cout = case
    x = torch.randn(n, cin, h, w, generator=torch.Generator().manual_seed(seed))
    wt = torch.randn(cout, cin, 1, 1, generator=torch.Generator().manual_seed(seed + 1)) / cin ** 0.5
    return x, wt


@pytest.mark.parametrize("case", PW_CASES)
def test_emulated_pointwise_bf16x6_at_the_operator_tolerance(case):
    x, wt = _problem(case)
    y64 = F.conv2d(x.double(), wt.double())
    err = (pw_emulated(x, wt, 6).double() - y64).abs()
    rel = float(err.max() / y64.abs().max())
    print(case, "bf16x6 max err / max |y| %.2e, err / (|x| conv |w|) %.2e" % (rel, float((err / pw_abs_conv(x, wt)).max())))
    assert rel < TOL


@pytest.mark.parametrize("case", PW_CASES)
def test_emulated_pointwise_bf16x3_inside_its_derived_bound(case):
    x, wt = _problem(case)
    y64 = F.conv2d(x.double(), wt.double())
    scale = pw_abs_conv(x, wt)
    err = (pw_emulated(x, wt, 3).double() - y64).abs()
    print(case, "bf16x3 err / (|x| conv |w|) %.2e (bound %.2e)" % (float((err / scale).max()), X3_REL + ACC_REL))
    assert bool((err <= (X3_REL + ACC_REL) * scale).all())


def test_pointwise_cancellation_problem():
    x, wt, want = pw_cancel_problem(2, 9, 11, 64, 96)
    assert float(want.abs().min()) > 1e-5    # a product far from zero (one tap: 1 / 9 of the 3x3 problem's)
    assert float(pw_emulated(x, wt, 3).abs().max()) == 0.0
    y6 = pw_emulated(x, wt, 6).double()
    assert float(((y6 - want).abs() / want.abs()).max()) < 1e-6


def test_plane_records_hold_the_exact_split():
    w = torch.randn(40, 3, 3, 64, generator=torch.Generator().manual_seed(5))
    for nplanes in (3, 2):
        recs = plane_records(w, nplanes)
        assert recs.shape == (40 * 9 * 2, nplanes, 32) and recs.dtype == torch.int16
        back = recs.view(torch.bfloat16).float()
        # record r, plane p = plane p of the 32 weights from float index 32 r
        for p, plane in enumerate(split(w)[:nplanes]):
            assert torch.equal(back[:, p, :].reshape(-1), plane.reshape(-1))
    hi, mid, lo = split(w)
    assert torch.equal(hi + mid + lo, w)


def test_plane_sizes_capability_and_struct_binding():
    from attention_based_tbn_amd._lib import BackboneParams, ConvDesc, lib
    L = lib()
    assert L.tbn_capabilities() & 2 and L.tbn_capabilities() & 1
    assert L.tbn_version() & 0xffff == 102
    assert L.tbn_conv_weight_planes_bytes(96, 3, 64, 6) == 96 * 9 * 64 * 6
    assert L.tbn_conv_weight_planes_bytes(96, 1, 64, 3) == 96 * 64 * 4
    assert L.tbn_conv_weight_planes_bytes(96, 1, 48, 6) == 0 and L.tbn_conv_weight_planes_bytes(96, 1, 64, 4) == 0
    # appended after `flags`: positional construction of the first ten fields keeps working, the pointer defaults to NULL
    prm = BackboneParams(1, 2, 3, 4, 5, 6, 0.1, 1e-5, 7, 8)
    assert prm.flags == 8 and not prm.weight_planes
    assert BackboneParams._fields_[-1][0] == "weight_planes" and BackboneParams._fields_[-2][0] == "flags"
    assert [f[0] for f in ConvDesc._fields_[-4:]] == ["out2", "out2_ld", "out2_col_begin", "out2_raw"]
    # the backbone-level size: every k in {1, 3} / stride 1 / cin % 32 == 0 conv of the layer table, 6 | 4 bytes per weight
    from attention_based_tbn_amd._lib import ConvInfo, call
    plan = C.c_void_p()
    call("tbn_backbone_plan_create", 3, 1, 64, 64, C.byref(plan))
    info, floats = ConvInfo(), 0
    for i in range(L.tbn_backbone_num_convs(plan)):
        call("tbn_backbone_conv_info", plan, i, C.byref(info))
        if info.ksize in (1, 3) and info.stride == 1 and info.cin % 32 == 0:
            floats += info.cout * info.ksize ** 2 * info.cin
    assert L.tbn_backbone_weight_planes_bytes(plan, 6) == 6 * floats
    assert L.tbn_backbone_weight_planes_bytes(plan, 3) == 4 * floats
    assert L.tbn_backbone_weight_planes_bytes(plan, 5) == 0
    L.tbn_backbone_plan_destroy(plan)


def test_conv_math_layers_interface_without_a_gpu():
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    net = BNInception(in_channels=3)
    keys = list(net.state_dict().keys())
    assert net.conv_math_layers == "3x3"
    with pytest.raises(ValueError):
        net.conv_math_layers = "1x1"
    assert net.conv_math_layers == "3x3"
    net.conv_math_layers = "all"
    assert net.conv_math_layers == "all" and list(net.state_dict().keys()) == keys
    net.eval()
    assert net._engine_flags() & 32 == 0            # conv_math "f32": ignored
    net.conv_math = "bf16x6"
    assert net._engine_flags() & (8 | 32) == (8 | 32)
    net.train()
    assert net._engine_flags() & (8 | 16 | 32) == 0   # ignored in training mode
