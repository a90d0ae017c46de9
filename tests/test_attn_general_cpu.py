"""The general attention core and the attention-weight softmax, as far as a machine without a GPU can see them: the
header, the exported symbols, the capability bit, the refusal of CPU tensors, and the source of core/models/attention.py
(no vendor-library call left in it)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tbn_mha_fwd", "tbn_mha_bwd", "tbn_attn_weights_fwd", "tbn_attn_weights_bwd")


def test_header_declares_the_entries_and_the_capability_bit():
    with open(os.path.join(ROOT, "include", "tbn_hip.h")) as f:
        h = f.read()
    for s in SYMBOLS:
        assert re.search(r"^int %s\(" % s, h, re.M), s
    assert re.search(r"^#define TBN_CAP_ATTN_GENERAL 8$", h, re.M)
    for cite in ("attention.py:48-57", "attention.py:60-91", ":94-145"):      # the reference code each entry replaces
        assert cite in h, cite


def test_library_exports_the_entries_and_sets_the_bit():
    from attention_based_tbn_amd._lib import SIGNATURES, lib
    L = lib()
    for s in SYMBOLS:
        assert s in SIGNATURES and hasattr(L, s), s
    assert L.tbn_capabilities() & 8
    assert L.tbn_version() & 0xffff == 102


def test_ops_refuse_cpu_tensors():
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd._lib import TbnHipError
    q, kv = torch.zeros(2, 8), torch.zeros(6, 8)
    with pytest.raises(TbnHipError, match="mha_core"):
        ops.mha_core(q, kv, kv, None, 2, 1, 3, 2)
    with pytest.raises(TbnHipError, match="attn_weights"):
        ops.attn_weights(torch.zeros(2, 3))
    with pytest.raises(TbnHipError, match="attn_weights"):
        ops.attn_weights(torch.zeros(2, 3), torch.ones(2, 3), 0.5, True, torch.ones(3, 4))


def test_attention_module_source_names_no_vendor_op():
    with open(os.path.join(ROOT, "attention_based_tbn_amd", "core", "models", "attention.py")) as f:
        src = f.read()
    for banned in ("torch.bmm", "torch.matmul", "F.softmax", "F.gumbel_softmax", "F.dropout", "torch.nn.functional"):
        assert banned not in src, banned
