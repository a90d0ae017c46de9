"""The split-bf16 convolution math mode (BNInception.conv_math / TBNModel.conv_math, TBN_BACKBONE_CONV_BF16X6 / _BF16X3 of
include/tbn_hip.h) at the engine and model level: which launches it reroutes, golden parity of the eval forward in
bf16x6 and bf16x3 at the north star's 1e-3, the interface, and BASELINE config 5's operating point against the CPU oracle.
Reference: model.eval() / torch.no_grad() forward of core/tools/test.py:67-87."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util import assert_close, build_oracle, load_case, rel_err  # noqa: E402
from tests.test_model_gpu import DEV, EVAL_CASES, build_product, to_dev  # noqa: E402

GOLDEN_EVAL = EVAL_CASES + ["crop_repeat_eval"]     # every golden case tests/test_model_gpu.py runs in eval mode


def _entries(L):
    out = {}
    name = C.create_string_buffer(160)
    for i in range(L.tbn_profile_num_entries()):
        cnt, ms, fl = C.c_long(), C.c_double(), C.c_double()
        L.tbn_profile_entry(i, name, 160, C.byref(cnt), C.byref(ms), C.byref(fl))
        out[name.value.decode()] = cnt.value
    L.tbn_profile_reset()
    return out


def _count(entries, sub):
    return sum(v for k, v in entries.items() if sub in k)


def _profiled(L, fn):
    L.tbn_profile_reset()
    L.tbn_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.tbn_profile_enable(0)
    return _entries(L)


def _eligible_layers(L, plan, width):
    """names of the convs the engine is documented to reroute, from tbn_backbone_conv_info and the map each layer reads:
    the stem halves the input, two ceil-mode 3x3 / stride 2 pools follow (conv2_* reads the first pool's output, the
    inception_3* blocks the second's), inception_3c / 4e halve again (reference bn_inception_audio.py:58-404)"""
    from attention_based_tbn_amd._lib import ConvInfo
    w1 = (width + 6 - 7) // 2 + 1
    w2 = -(-(w1 - 3) // 2) + 1
    w3 = -(-(w2 - 3) // 2) + 1
    w4 = (w3 - 1) // 2 + 1
    w5 = (w4 - 1) // 2 + 1
    maps = {"conv2": w2, "inception_3": w3, "inception_4": w4, "inception_5": w5}
    names, info = [], ConvInfo()
    for i in range(L.tbn_backbone_num_convs(plan.handle)):
        assert L.tbn_backbone_conv_info(plan.handle, i, C.byref(info)) == 0
        name = info.name.decode()
        if info.ksize == 3 and info.stride == 1 and info.pad == 1 and info.cin % 32 == 0:
            mw = [v for k, v in maps.items() if name.startswith(k)]
            assert len(mw) == 1, name
            if mw[0] <= 64:
                names.append(name)
    return names


@pytest.mark.parametrize("cin,hw", [(3, (224, 224)), (1, (256, 420))])
def test_engine_routes_the_3x3_unit_stride_layers(cin, hw):
    """eval forward with TBN_BACKBONE_CONV_BF16X6: one bf16x6 launch per 3x3 / stride 1 / pad 1 layer on a map at most 64
    wide (RGB 224 x 224: all 27; audio 256 x 420: conv2_3x3 works on a 64 x 105 map and stays on the fp32 kernel), none in a
    training forward with the same setting, none with the mode off."""
    from attention_based_tbn_amd._lib import lib
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    L = lib()
    torch.manual_seed(5)
    net = BNInception(1000, cin).to(DEV)
    x = torch.randn(4, cin, *hw, device=DEV)
    net.eval()
    with torch.no_grad():
        ref = net(x)                                   # tunes the eval plan
        plan = net._plans[(4,) + hw]
        names = _eligible_layers(L, plan, hw[1])
        want = len(names)
        print("layers on the split-bf16 kernel at %d x %d: %d" % (hw + (want,)), "(conv2_3x3 %s)" % ("in" if "conv2_3x3" in names else "out"))
        assert want > 0
        fp, nbytes = plan.fingerprint(), len(plan.export_choices())
        e = _profiled(L, lambda: net(x))
        assert _count(e, "bf16x") == 0, e
        net.conv_math = "bf16x6"
        holder = []
        e = _profiled(L, lambda: holder.append(net(x)))
        assert _count(e, "bf16x6") == want and _count(e, "bf16x3") == 0, e
        assert plan.fingerprint() == fp and len(plan.export_choices()) == nbytes        # the plan does not change
        print("bf16x6 vs f32 pooled features: rel_err %.2e" % rel_err(holder[0], ref))
        assert rel_err(holder[0], ref) < 1e-4
        net.conv_math = "bf16x3"
        e = _profiled(L, lambda: net(x))
        assert _count(e, "bf16x3") == want and _count(e, "bf16x6") == 0, e
    net.conv_math = "bf16x6"
    net.train()
    e = _profiled(L, lambda: net(x))
    assert sum(e.values()) > 0 and _count(e, "bf16x") == 0, e


@pytest.mark.parametrize("name", GOLDEN_EVAL)
def test_golden_parity_in_bf16x6_and_bf16x3(name):
    """both modes at assert_close's 1e-3 against the golden outputs.  bf16x3 is only offered by the Python property while
    it keeps a 4x margin to that on fixture-size inputs: its rel_err against the golden outputs is asserted below 2.5e-4
    here (the gate itself, not a recorded figure); the BF16X_RECORD lines are what profiles/bf16x_eval.md records."""
    cfg, modality, meta, data, inp, target = load_case(name)
    model, crit = build_product(cfg, modality, meta)
    model.eval()
    dinp = to_dev(inp)
    with torch.no_grad():
        f32 = {k: v.clone() for k, v in model(dinp).items()}
        for mode in ("bf16x6", "bf16x3"):
            model.conv_math = mode
            out = model(dinp)
            for k, v in out.items():
                want = data["out_" + k]
                assert tuple(v.shape) == want.shape, k
                e = assert_close(v, want, (mode, k))
                if mode == "bf16x3":
                    assert e < 2.5e-4, (name, k, e)
                print("BF16X_RECORD %s %s %s: vs golden %.3e, vs f32 %.3e" % (name, mode, k, e, rel_err(v, f32[k])))


def test_interface():
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    from attention_based_tbn_amd.core.models.dataparallel import DataParallel
    cfg, modality, meta, data, inp, target = load_case("cfg5_all_mha_eval")
    model, crit = build_product(cfg, modality, meta)
    keys = list(model.state_dict().keys())
    assert model.conv_math == "f32"
    bases = [getattr(model, "Base_" + m) for m in modality]
    assert len(bases) == 3 and all(b.conv_math == "f32" for b in bases)
    with pytest.raises(ValueError):
        model.conv_math = "bf16x9"
    with pytest.raises(ValueError):
        bases[0].conv_math = "bf16x9"
    assert all(b.conv_math == "f32" for b in bases)
    model.conv_math = "bf16x6"
    assert model.conv_math == "bf16x6" and all(b.conv_math == "bf16x6" for b in bases)
    assert list(model.state_dict().keys()) == keys
    dp = DataParallel(model)
    dp.conv_math = "bf16x3"
    assert dp.conv_math == "bf16x3" and all(b.conv_math == "bf16x3" for b in bases)

    # training ignores the mode: bit-identical output and gradients
    torch.manual_seed(3)
    net = BNInception(1000, 3).to(DEV).train()
    x = torch.randn(6, 3, 96, 96, device=DEV)

    def train_step():
        net.zero_grad()
        rm, rv = net.running_mean.clone(), net.running_var.clone()
        out = net(x)
        out.square().mean().backward()
        net.running_mean.copy_(rm)
        net.running_var.copy_(rv)
        return out.detach().clone(), net.flat_weight.grad.clone(), net.bn_weight_rest.grad.clone()

    a = train_step()
    net.conv_math = "bf16x6"
    b = train_step()
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_config5_eval_chunk_in_bf16x6_vs_oracle():
    """BASELINE config 5 as tests/test_operating_points_gpu.py runs it in f32 (B = 11 clips = 275 frames per modality: one
    full eval_chunk of 256 frames plus a 19-frame remainder), in bf16x6, against the CPU oracle's eval forward."""
    from attention_based_tbn_amd.config import load_config, get_modality
    from tests.test_operating_points_gpu import _meta
    cfg = load_config(["data.audio.audio_length=1.279"])
    modality = get_modality(cfg)
    assert modality == ["RGB", "Flow", "Audio"] and cfg.test.num_segments == 25 and cfg.model.attention.type == "mha"
    meta = _meta(cfg, modality, 1505)
    B, n = 11, cfg.test.num_segments
    g = torch.Generator().manual_seed(9)
    mean = torch.tensor([0.408, 0.459, 0.502]).view(1, 1, 3, 1, 1)
    inp = {"RGB": torch.rand(B, n, 3, 224, 224, generator=g) - mean,
           "Flow": torch.rand(B, n, 10, 224, 224, generator=g) - 0.502,
           "Audio": (torch.randn(B, n, 1, 256, 256, generator=g) * 3 - 6).clamp_(-13.8155, 8.0)}
    model, _ = build_product(cfg, modality, meta)
    model.eval()
    model.conv_math = "bf16x6"
    for m in modality:
        assert getattr(model, "Base_" + m).eval_chunk == 256
    with torch.no_grad():
        out = model(to_dev(inp))
    t0 = time.time()
    oracle, _ = build_oracle(cfg, modality, meta)
    oracle.eval()
    with torch.no_grad():
        want = oracle(inp)
    print("oracle eval forward of 275 frames x 3 modalities: %.1f s" % (time.time() - t0))
    assert set(want) == set(out) == {"verb", "noun", "weights"}
    for k in want:
        e = assert_close(out[k], want[k], ("bf16x6", k))
        print("BF16X_RECORD config-5 bf16x6 vs oracle: %s relative error %.2e" % (k, e))
