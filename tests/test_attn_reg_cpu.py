"""The attention-weight regularisers as far as a machine without a GPU can see them: the header, the exported symbols with
the header's signatures, the refusal of CPU tensors, and get_loss on CPU tensors -- the torch fallback, bit for bit what
the formulas of reference core/models/model.py:299-332 give."""
import ctypes as C
import json
import os
import re

import pytest
import torch
import torch.nn as nn
from torch.distributions import Categorical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tbn_attn_reg_fwd", "tbn_attn_reg_bwd")
CTYPE = {"int": C.c_int, "float": C.c_float, "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p}


def header():
    with open(os.path.join(ROOT, "include", "tbn_hip.h")) as f:
        return f.read()


def test_header_declares_the_entries_the_switch_values_and_the_reference_lines():
    h = header()
    for s in SYMBOLS:
        assert re.search(r"^int %s\(" % s, h, re.M), s
    for name, val in (("TBN_ATTN_PRIOR_NONE", 0), ("TBN_ATTN_PRIOR_KL", 1), ("TBN_ATTN_PRIOR_MSE", 2),
                      ("TBN_ATTN_PRIOR_SMOOTHL1", 3), ("TBN_ATTN_RED_SUM", 0), ("TBN_ATTN_RED_MEAN", 1),
                      ("TBN_ATTN_RED_BATCHMEAN", 2), ("TBN_CAP_ATTN_REG", 16)):
        assert re.search(r"^#define %s %d$" % (name, val), h, re.M), name
    for cite in ("model.py:299-332", "contrast_loss.py:4-25"):
        assert cite in h, cite


def test_library_exports_the_entries_with_the_headers_signatures():
    from attention_based_tbn_amd._lib import SIGNATURES, lib
    L = lib()
    h = header()
    for s in SYMBOLS:
        assert s in SIGNATURES and hasattr(L, s), s
        proto = re.search(r"^int %s\((.*?)\);" % s, h, re.M | re.S).group(1)
        params = [" ".join(p.split()[:-1]) for p in proto.replace("\n", " ").split(",")]
        res, args = SIGNATURES[s]
        assert res is C.c_int and [CTYPE[p] for p in params] == list(args), (s, params)
    assert L.tbn_capabilities() & 16


def test_operator_refuses_cpu_tensors():
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd._lib import TbnHipError
    w = torch.softmax(torch.randn(3, 8), 1)
    with pytest.raises(TbnHipError, match="attn_regularisers"):
        ops.attn_regularisers(w, None, use_entropy=True)
    with pytest.raises(TbnHipError, match="attn_regularisers"):
        ops.attn_regularisers(w, w, prior_kind="kl", prior_reduction="batchmean", use_contrast=True, use_entropy=True,
                              mults=(0.25, 0.25, 0.25), training=True, entropy_thresh=0.2)


def test_entropy_written_out_is_categoricals():
    """tests/test_attn_reg_gpu.py states Categorical(probs=x + 1e-6).entropy() with the clamp constant explicit (its float64
    reference of the rebound cases clamps at float32's eps): with float64's own eps the formula is Categorical's"""
    x = torch.softmax(2.0 * torch.randn(7, 25, generator=torch.Generator().manual_seed(3)), 1).double()
    q = x + 1e-6
    p = q / q.sum(-1, keepdim=True)
    eps = float(torch.finfo(torch.float64).eps)
    a = -(p * torch.log(p.clamp(min=eps, max=1 - eps))).sum(-1)
    b = Categorical(probs=x + 1e-6, validate_args=False).entropy()
    assert float((a - b).abs().max()) < 1e-14


@pytest.mark.parametrize("epoch,training", [(0, True), (20, True), (20, False)])
def test_get_loss_on_cpu_tensors_is_the_torch_formulas_bit_for_bit(epoch, training):
    """the fallback is untouched: CPU weights never reach the operator (train_cfg3_mha: kl prior + contrast + entropy)"""
    from attention_based_tbn_amd.config import load_config, get_modality
    from attention_based_tbn_amd.core.models import build_model
    with open(os.path.join(ROOT, "tests", "golden", "keys_train_cfg3_mha.json")) as f:
        meta = json.load(f)
    cfg = load_config(meta["overrides"])
    att = cfg.model.attention
    assert att.use_prior and att.use_contrast and att.use_entropy and att.wt_loss == "kl"
    model, crit, _ = build_model(cfg, get_modality(cfg), torch.device("cpu"))
    assert model.fused_attention_losses is True
    model.train(training)
    g = torch.Generator().manual_seed(3)
    B, n, T = 2, 3, 8
    w = torch.softmax(3.0 * torch.randn(B * n, 1, T, generator=g), 2).requires_grad_(True)
    prior = torch.softmax(torch.randn(B, n, T, 1, generator=g), 2)
    preds = {"verb": torch.randn(B, 125, generator=g), "noun": torch.randn(B, 352, generator=g), "weights": w}
    target = {"class": {"verb": torch.randint(0, 125, (B,), generator=g), "noun": torch.randint(0, 352, (B,), generator=g)},
              "weights": prior}
    loss, bs = model.get_loss(crit, target, preds, epoch=epoch)
    assert bs == B and list(loss.keys()) == ["total", "all_class", "verb", "noun", "prior", "contrast", "entropy"]
    (gw,) = torch.autograd.grad(loss["total"], w)

    w2 = w.detach().clone().requires_grad_(True)
    zero = training and epoch + 1 < att.decay_step
    pm, cm, em = (0, 0, 0) if zero else (att.wt_decay, att.contrast_decay, att.entropy_decay)
    ce = nn.CrossEntropyLoss()
    total = 0
    all_class = 0
    for k in ("verb", "noun"):
        all_class += ce(preds[k], target["class"][k])
    total += all_class
    x = torch.log(w2.squeeze(1) + 1e-7)
    lp = nn.KLDivLoss(reduction=att.loss_reduction)(x, prior.reshape(B * n, -1))
    total += pm * lp
    hi = x.detach() >= att.contrast_thresh
    lc = (x.masked_fill(hi, 0) - x.masked_fill(~hi, 0)).sum(dim=1).mean()
    total += cm * lc
    le = Categorical(probs=x + 1e-6, validate_args=False).entropy().mean()
    if training and em > 0:
        em = em * (le.detach() >= att.entropy_thresh).to(le.dtype)
    total += em * le
    (gw2,) = torch.autograd.grad(total, w2)
    for got, want in ((loss["prior"], lp), (loss["contrast"], lc), (loss["entropy"], le), (loss["total"], total),
                      (loss["all_class"], all_class)):
        assert torch.equal(got.detach(), want.detach())
    assert torch.equal(gw, gw2)
