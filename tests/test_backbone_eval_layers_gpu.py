"""Per-layer parity of the backbone engine's EVAL forward (tbn_backbone_forward, training = 0) at ragged input sizes, in fp32
and in the split-bf16 math modes (conv_math / conv_math_layers of BNInception; TBN_BACKBONE_CONV_BF16X6 / _BF16X3 / _BF16X_ALL
of include/tbn_hip.h).  Reference: the fp64 eval forward of oracle.bninception.BNInception (the graph of reference
core/models/bn_inception_audio.py:58-404,437-1003), every post-ReLU activation captured by forward hooks.

The other eval checks look at pooled features or logits, after a global mean has diluted a wrong border pixel or column.  Here
every part of every GEMM -- the up-to-four segments a merged 1x1 group writes in one launch, the raw pool_proj segment and
its average pool + BN apply included -- is read back from the workspace (tbn_backbone_tensor_info kind 0) and compared with
the activation of the same module as max |error| / max |activation|.  The two stem convs whose z cannot be located (kind 0 is
refused: their max pool is fused in training) are compared through their max pool's output, the input buffer of the next
conv (kind 3).  The engine gives every activation buffer its own workspace region, so an eval-size workspace holds all of them
after the pass.

Bounds: fp32 and bf16x6 -- TOL = 1e-4 per layer, the operator tolerance of tests/test_conv_variants_gpu.py, at every depth (no
yardstick taken from the fp32 run: its own worst layer sits at 2e-6, and a defect in the shared segment code would move
such a yardstick along with the run under test); bf16x3 -- the 2.5e-4 gate of tests/test_model_bf16x_gpu.py per layer.
Observed worst layers over the five sizes: fp32 2.1e-6, bf16x6 3.1e-6 (3x3 and all), bf16x3 2.7e-5.
Launch counts: with "all" one split-bf16 launch per eligible GEMM at that input size, in fp32 none."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_conv_variants_gpu import TOL  # noqa: E402
from tests.test_model_bf16x_all_gpu import _pointwise_gemms  # noqa: E402
from tests.test_model_bf16x_gpu import _count, _eligible_layers, _profiled  # noqa: E402
from tests.test_model_gpu import DEV  # noqa: E402

X3_GATE = 2.5e-4
SETTINGS = [("f32", "3x3"), ("bf16x6", "3x3"), ("bf16x6", "all"), ("bf16x3", "all")]
FUSED = {"conv1_7x7_s2": ("pool1_3x3_s2", "conv2_3x3_reduce"), "conv2_3x3": ("pool2_3x3_s2", "inception_3a_1x1")}


def _rows(t):
    """NCHW -> (pixels, channels) in the engine's NHWC order, fp64 on the device"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).to(DEV)


def _oracle_activations(o64, x):
    """{conv name: its post-ReLU activation, pool name: its output} of the fp64 eval forward, as device rows"""
    acts, hooks = {}, []
    convs = [n for n, m in o64.named_children() if isinstance(m, torch.nn.Conv2d)]
    relus = [n for n, m in o64.named_children() if isinstance(m, torch.nn.ReLU)]
    assert len(convs) == len(relus) == 69
    for cname, rname in zip(convs, relus):
        hooks.append(getattr(o64, rname).register_forward_hook(
            lambda mod, inp, out, k=cname: acts.__setitem__(k, _rows(out.detach()))))
    for pname, _ in FUSED.values():
        hooks.append(getattr(o64, pname).register_forward_hook(
            lambda mod, inp, out, k=pname: acts.__setitem__(k, _rows(out.detach()))))
    with torch.no_grad():
        o64(x.double())
    for h in hooks:
        h.remove()
    assert len(acts) == 71
    return convs, acts


@pytest.mark.parametrize("cin_hw", [(3, 64, 64), (3, 97, 97), (10, 70, 129), (1, 128, 256), (3, 224, 224),
                                    (2, 64, 64), (6, 70, 129)])   # channel counts no modality uses: the runtime-channel stem repacks
def test_every_layer_of_the_eval_forward_vs_fp64_oracle(cin_hw):
    from oracle.bninception import BNInception as OBN
    from oracle.fill import fill_state_dict
    from attention_based_tbn_amd._lib import TbnHipError, call, lib
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    L = lib()
    cin, H, W = cin_hw
    N = 2 if H >= 224 else 3
    ora = OBN(1000, cin)
    sd = fill_state_dict(ora.state_dict(), 42)
    ora.load_state_dict(sd)
    o64 = copy.deepcopy(ora).double().eval()
    net = BNInception(1000, cin).to(DEV)
    net.load_state_dict(sd)
    net.eval()
    x = torch.randn(N, cin, H, W, generator=torch.Generator().manual_seed(1))
    convs, acts = _oracle_activations(o64, x)
    xd = x.to(DEV)
    with torch.no_grad():
        net(xd)                                        # tunes the eval plan
    plan = net._plans[(N, H, W)]
    assert len(plan.pool) == 1
    ws = plan.pool[0][0].view(torch.float32)
    want3, want1 = len(_eligible_layers(L, plan, W)), len(_pointwise_gemms(L, plan))
    assert want3 > 0 and want1 >= 11

    def tensor(name, kind):
        off, rows, cols, ld = C.c_long(), C.c_int(), C.c_int(), C.c_int()
        call("tbn_backbone_tensor_info", plan.handle, name.encode(), kind, C.byref(off), C.byref(rows), C.byref(cols),
             C.byref(ld))
        return torch.as_strided(ws, (rows.value, cols.value), (ld.value, 1), off.value)

    def layer_errors():
        errs = {}
        for name in convs:
            want = acts[name]
            try:
                got = tensor(name, 0)
            except TbnHipError:
                pool, consumer = FUSED[name]           # z cannot be located: compare its max pool's output
                want, got = acts[pool], tensor(consumer, 3)
            assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
            errs[name] = float((got.double() - want).abs().max() / want.abs().max())
        return errs

    e32 = None
    for mode, layers in SETTINGS:
        net.conv_math, net.conv_math_layers = mode, layers
        ws.zero_()                                     # nothing survives from the previous setting
        with torch.no_grad():
            prof = _profiled(L, lambda: net(xd))
        assert len(plan.pool) == 1 and plan.pool[0][0].data_ptr() == ws.data_ptr()
        errs = layer_errors()
        assert len(errs) == 69
        if mode == "f32":
            e32 = errs
            assert _count(prof, "bf16x") == 0, prof
        elif layers == "3x3":
            assert _count(prof, "conv_bf16x6_kernel<") == want3 and _count(prof, "bf16x") == want3, prof
        else:
            assert _count(prof, "conv_%s_pw_kernel<" % mode) == want1, prof
            assert _count(prof, "conv_%s_planes_kernel<" % mode) == want3, prof
            assert _count(prof, "bf16x") == want1 + want3, prof
        worst = max(errs, key=errs.get)
        print("EVAL_LAYERS %s x %d frames, %s / %s: worst layer %s %.2e (fp32 there %.2e); %d 3x3 + %d pointwise launches eligible"
              % (cin_hw, N, mode, layers, worst, errs[worst], e32[worst], want3, want1))
        bound = X3_GATE if mode == "bf16x3" else TOL
        for name, e in errs.items():
            assert e < bound, (cin_hw, mode, layers, name, e, bound, e32[name])
    net.conv_math = "f32"
