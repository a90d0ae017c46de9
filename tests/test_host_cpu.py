"""CPU-only tests of the host side: C-ABI library loads and exports every declared symbol, config
tree, product sampler bit-exactness, checkpoint-key contract, loud failure without a GPU, and the
RCCL data-parallel wrapper rehearsed on gloo with 2 processes."""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_header_symbol():
    from attention_based_tbn_amd import _lib
    handle = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tbn_hip.h")).read()
    declared = set(re.findall(r"\b(tbn_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 40
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert getattr(handle, name) is not None
    assert handle.tbn_version() >= 100
    # every capability bit the header names is one this build reports
    caps = {name: int(v) for name, v in re.findall(r"^#define (TBN_CAP_[A-Z0-9_]+) (\d+)$", header, re.M)}
    assert caps["TBN_CAP_BN_BATCH_OPS"] == 128 and len(caps) == 8 and sum(caps.values()) == 255
    assert handle.tbn_capabilities() == 255


def test_engine_layer_table_matches_reference_graph():
    """69 convs, names/shapes as the reference graph; fused 1x1 groups (1x1 | 3x3_reduce | double_3x3_reduce |
    pool_proj of an average-pool block) adjacent in the flat arrays"""
    from attention_based_tbn_amd.core.models.bn_inception import BNInception, reference_conv_order
    net = BNInception(1000, 3)
    assert len(net._layers) == 69 and list(reference_conv_order()) == net._order
    L = net._layers
    assert (L["conv1_7x7_s2"]["cin"], L["conv1_7x7_s2"]["cout"], L["conv1_7x7_s2"]["k"]) == (3, 64, 7)
    assert (L["inception_4e_double_3x3_2"]["cin"], L["inception_4e_double_3x3_2"]["cout"],
            L["inception_4e_double_3x3_2"]["stride"]) == (256, 256, 2)
    a, b, c = L["inception_4a_1x1"], L["inception_4a_3x3_reduce"], L["inception_4a_double_3x3_reduce"]
    assert b["c_off"] == a["c_off"] + a["cout"] and c["c_off"] == b["c_off"] + b["cout"]
    assert b["w_off"] == a["w_off"] + a["cout"] * a["cin"]
    d = L["inception_4a_pool_proj"]        # rides in the same GEMM: the 3x3 average pool commutes with the 1x1 conv
    assert d["c_off"] == c["c_off"] + c["cout"] and d["w_off"] == c["w_off"] + c["cout"] * c["cin"]
    e, f = L["inception_5b_double_3x3_reduce"], L["inception_5b_pool_proj"]   # max-pool block: pool stays in front
    assert f["c_off"] != e["c_off"] + e["cout"]
    n_params = sum(p.numel() for n, p in net.named_parameters() if not n.startswith("last_linear"))
    assert n_params == 10_272_064 + 0 or n_params > 10_000_000  # ~10.27 M
    macs = sum(v["cout"] * v["cin"] * v["k"] ** 2 for v in L.values())
    assert macs == net.flat_weight.numel()


@pytest.mark.parametrize("name", ["cfg1_audio_only", "cfg3_rgb_audio_mha_T13", "cfg5_all_mha_eval", "unimodal_attn",
                                  "proto_attn", "train_cfg3_mha"])
def test_state_dict_keys_match_reference(name):
    from attention_based_tbn_amd.config import load_config, get_modality
    from attention_based_tbn_amd.core.models import build_model
    from oracle.fill import fill_state_dict
    with open(os.path.join(GOLDEN, f"keys_{name}.json")) as f:
        meta = json.load(f)
    cfg = load_config(meta["overrides"])
    model, crit, _ = build_model(cfg, get_modality(cfg), torch.device("cpu"))
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["keys"]
    filled = fill_state_dict(sd, 3)
    model.load_state_dict(filled)
    back = model.state_dict()
    assert all(torch.equal(back[k], filled[k]) for k in filled)
    # trainable set under partialbn == reference's (by reference names)
    if cfg.model.freeze_base and cfg.model.freeze_mode == "partialbn":
        for m in get_modality(cfg):
            base = getattr(model, "Base_" + m)
            assert base.bn_weight_first.requires_grad and not base.bn_weight_rest.requires_grad
            assert f"Base_{m}.conv1_7x7_s2_bn.weight" in meta["trainable"]
            assert f"Base_{m}.conv2_3x3_reduce_bn.weight" not in meta["trainable"]
    with pytest.raises(RuntimeError):
        bad = dict(filled)
        bad.pop("classifier.verb.weight")
        model.load_state_dict(bad)


def test_product_fails_loudly_on_cpu():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    from attention_based_tbn_amd import ops
    net = BNInception(1000, 3)
    with pytest.raises(TbnHipError):
        net(torch.zeros(1, 3, 64, 64))
    with pytest.raises(TbnHipError):
        ops.linear(torch.zeros(4, 32), torch.zeros(32, 32))
    import attention_based_tbn_amd
    src = open(os.path.join(os.path.dirname(attention_based_tbn_amd.__file__), "ops.py")).read()
    assert "oracle" not in src  # the product never routes through the checker


def test_no_product_module_imports_oracle():
    pkg = os.path.join(ROOT, "attention_based_tbn_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), os.path.join(dp, f)


def test_config_overrides_and_reference_dir_equivalence():
    from attention_based_tbn_amd.config import load_config
    cfg = load_config(["model.attention.enable=False", "train.optim.lr=1e-3", "gpu_ids=[0,1]",
                       "data.audio.audio_length=1.279"])
    assert cfg.model.attention.enable is False and cfg.train.optim.lr == 1e-3 and cfg.gpu_ids == [0, 1]
    assert list(cfg.model.num_classes.keys()) == ["verb", "noun"] and "attn_heads" in cfg.pretty()
    assert round(cfg.data.audio.audio_length * 25 / 4) == 8
    with pytest.raises(ValueError):
        load_config(["nonsense"])


def test_product_sampler_bit_exact_vs_reference_golden():
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import SegmentSampler
    with open(os.path.join(GOLDEN, "sampler.json")) as f:
        g = json.load(f)
    for case in g["cases"]:
        nseg = case["num_segments"]
        cfg = load_config([f"data.sampling={case['sampling']}", f"train.num_segments={nseg}",
                           f"val.num_segments={nseg}", f"test.num_segments={nseg}"])
        sampler = SegmentSampler(cfg, case["modality"], case["mode"])
        np.random.seed(case["seed"])
        for row, want in zip(g["rows"], case["indices"]):
            got = sampler(row["start_frame"], row["stop_frame"])
            for m in case["modality"]:
                assert got[m].dtype == np.int64 and got[m].tolist() == want[m]
    s = SegmentSampler(load_config(), ["RGB", "Flow"], "train")
    assert s.flow_frames(np.array([10, 20, 30])).tolist() == [10, 11, 12, 13, 14, 20, 21, 22, 23, 24, 30, 31, 32, 33, 34]


def test_trim_audio_window_matches_oracle():
    from attention_based_tbn_amd.core.dataset import trim_audio_window
    from oracle.stft import trim_audio
    a = np.arange(200000, dtype=np.float32)
    for frame in (0, 10, 120, 400, 499):
        for sec in (1.279, 2.1):
            start, length = trim_audio_window(len(a), frame, sec)
            seg, _ = trim_audio(a, frame, sec)
            assert length == len(seg) and seg[0] == a[start]


def test_trim_audio_short_clip_branch_matches_oracle():
    """reference core/dataset/dataset.py:441-451 (round-5 verdict, row a18): a clip SHORTER than `audio_length` is
    zero-padded and then sliced with the un-updated `max_len` -- start = max_len - min_len < 0, an empty slice of the
    padded array.  The product's `trim_audio` (NumPy arrays and torch tensors) must return exactly what the oracle's
    restatement returns for short, barely-long-enough and long clips, at every clamping case; `Spectrogram` refuses the
    empty sample like the reference's librosa call."""
    import torch
    from attention_based_tbn_amd.core.dataset import Spectrogram, trim_audio, trim_audio_window
    from oracle.stft import trim_audio as oracle_trim
    for n in (0, 1, 1000, 30694, 30695, 30696, 50399, 50400, 50401, 200000):
        a = (np.arange(n, dtype=np.float32) + 1.0) * 0.5
        for frame in (0, 1, 37, 120, 400, 499, 6000):
            for sec in (1.279, 2.1):
                want, _ = oracle_trim(a, frame, sec)
                got = trim_audio(a, frame, sec)
                got_t = trim_audio(torch.from_numpy(a), frame, sec)
                assert got.shape == want.shape and np.array_equal(got, want), (n, frame, sec, got.shape, want.shape)
                assert np.array_equal(got_t.numpy(), want), (n, frame, sec)
                start, length = trim_audio_window(n, frame, sec)
                if n >= length:
                    assert len(want) == length and start >= 0 and np.array_equal(a[start:start + length], want)
                else:
                    assert start == n - length < 0 and len(want) == 0          # the reference's quirk: an EMPTY sample
    spec = Spectrogram()
    with pytest.raises(Exception):        # no GPU here: a CPU tensor is refused before anything else (no CPU fallback)
        spec(torch.zeros(1, 0))


_DP_WORKER = r'''
import os, sys, torch, torch.distributed as dist, torch.nn as nn
sys.path.insert(0, sys.argv[1])
from attention_based_tbn_amd.core.models.dataparallel import DataParallel
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank = dist.get_rank()
case = os.environ["DP_CASE"]                        # avg | drop1 (rank 1 drops the optional branch) | dropall
torch.manual_seed(100 + rank)                       # different init per rank -> broadcast must fix it
class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(8, 4); self.b = nn.Linear(4, 2)
        self.c = nn.Linear(8, 4)                    # the "audio" branch: may be dropped per replica
        self.register_buffer("stat", torch.full((3,), float(rank)))
        self.register_buffer("count", torch.full((2,), rank, dtype=torch.long))
        self.drop = False
    def maybe_unused_parameter_prefixes(self): return ["c."] if case != "avg" else []
    if os.environ.get("DP_REPORT", "1") == "1":     # the module reports its draw: exchanged right after forward
        def optional_parameters_used(self): return not self.drop
    def forward(self, x):
        u = torch.zeros(x.shape[0], 4) if self.drop else self.c(x)
        return self.b(torch.relu(self.a(x)) + u)
    def get_loss(self, criterion, target, preds, epoch=0): return {"total": criterion(preds, target)}, preds.shape[0]
DataParallel.SMALL = 16                             # a.weight / c.weight (32 elements) take the "large tensor" route
model = DataParallel(Toy(), overlap=os.environ["DP_OVERLAP"] == "1")
ref = Toy(); ref.load_state_dict(model.module.state_dict())
assert float(model.module.stat[0]) == 0.0 and int(model.module.count[1]) == 0   # buffers came from rank 0 (both dtypes)
g = torch.Generator().manual_seed(7)
X = torch.randn(8, 8, generator=g); Y = torch.randn(8, 2, generator=g)
xs, ys = X[rank * 4:(rank + 1) * 4], Y[rank * 4:(rank + 1) * 4]   # clips sharded by rank, no data-path collective
# one entry per consecutive step: (rank 0 drops, rank 1 drops).  "flip": the decision changes from step to step --
# dropped on one rank, on both, on the other, on none -- so presence flags, _pending and _fired must reset every step
steps = {"avg": [(False, False)], "drop1": [(False, True)], "dropall": [(True, True)],
         "flip": [(False, True), (True, True), (True, False), (False, False), (True, True)]}[case]
for it, drops in enumerate(steps):
    model.zero_grad(set_to_none=True); ref.zero_grad(set_to_none=True)
    model.module.drop = drops[rank]
    loss, bs = model.get_loss(nn.MSELoss(), ys, model(xs), epoch=3)
    loss["total"].backward()
    outs = []
    for r in range(2):                              # full-batch reference on every rank, same per-shard decisions
        ref.drop = drops[r]
        outs.append(ref(X[r * 4:(r + 1) * 4]))
    nn.MSELoss()(torch.cat(outs), Y).backward()
    for (n, p), (_, q) in zip(model.module.named_parameters(), ref.named_parameters()):
        if q.grad is None:                          # nobody produced it: the optimiser must see None
            assert drops == (True, True) and n.startswith("c.") and p.grad is None, (it, n)
        else:
            assert p.grad is not None and torch.allclose(p.grad, q.grad, atol=1e-6), (it, n)
    assert model._pending == [] and model._fired == set() and not model._callback_queued and bs == 4
if case != "avg":
    # TWO training forwards before ONE backward, with opposite draws ("nobody" first, "everybody" second): the count the
    # ranks exchanged after the first forward no longer describes the backward -> the wrapper must fall back to the
    # presence flags (ADVICE round 3: the stale "nobody" would have turned the produced gradients into None)
    model.zero_grad(set_to_none=True); ref.zero_grad(set_to_none=True)
    model.module.drop = True
    model(xs)
    model.module.drop = False
    loss, _ = model.get_loss(nn.MSELoss(), ys, model(xs), epoch=3)
    assert model._presence is None and model._forwards_pending == 2
    loss["total"].backward()
    ref.drop = False
    nn.MSELoss()(torch.cat([ref(X[:4]), ref(X[4:])]), Y).backward()
    for (n, p), (_, q) in zip(model.module.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and torch.allclose(p.grad, q.grad, atol=1e-6), ("two forwards", n)
    assert model._forwards_pending == 0 and model._pending == [] and not model._callback_queued
    if os.environ.get("DP_REPORT", "1") == "1":
        # a draw that contradicts the gradients (reported "nobody", produced by everybody) must fail loudly, not hang
        model.zero_grad(set_to_none=True)
        model.module.drop = True
        out = model(xs)                                 # exchanged: 0 of 2 replicas
        model.module.drop = False
        extra = model.module.c(xs).sum() * 0.0          # ... yet the optional branch takes part in the backward
        try:
            (nn.MSELoss()(out, ys) + extra).backward()
            raise SystemExit("mismatching draw was not detected")
        except RuntimeError as e:
            assert "does not match the gradients" in str(e), e
        assert model._pending == [] and not model._callback_queued and model._forwards_pending == 0
        # ONE rank contradicts the draw (rank 1 alone produces the gradients nobody announced): it follows the peers'
        # schedule, raises at once and drops the gradients that were not reduced; rank 0 completes its backward and
        # learns it from the flag in the packed buffer at its next forward -- every rank fails loudly, nobody hangs
        model.zero_grad(set_to_none=True)
        model.module.drop = True
        out = model(xs)
        model.module.drop = False
        loss1 = nn.MSELoss()(out, ys)
        if rank == 1:
            loss1 = loss1 + model.module.c(xs).sum() * 0.0
        try:
            loss1.backward()
            raised = False
        except RuntimeError as e:
            raised = "does not match the gradients" in str(e)
        assert raised == (rank == 1), raised
        assert all(p.grad is None for n, p in model.module.named_parameters() if n.startswith("c."))
        assert model._pending == [] and not model._callback_queued
        if rank == 0:
            try:
                model(xs)
                raise SystemExit("the peer's mismatch flag was not seen")
            except RuntimeError as e:
                assert "peer rank" in str(e), e
with model.no_sync():                               # gradients stay local: rank-dependent data -> rank-dependent gradients
    model.zero_grad(set_to_none=True); model.module.drop = False
    nn.MSELoss()(model(xs), ys).backward()
    mine = model.module.a.weight.grad.clone()
both = [torch.empty_like(mine) for _ in range(2)]
dist.all_gather(both, mine)
assert not torch.allclose(both[0], both[1]) and model._pending == [] and not model._callback_queued
sd = model.state_dict(); assert all(k.startswith("module.") for k in sd)
print("DP_OK", rank)
dist.destroy_process_group()                        # orderly shutdown: a rank that just exits while c10d's threads still run can abort in teardown
'''


@pytest.mark.parametrize("overlap,case", [(True, "avg"), (False, "avg"), (True, "drop1"), (False, "drop1"),
                                          (True, "dropall"), (True, "flip"), (False, "flip"), (True, "flip-noreport"),
                                          (True, "drop1-noreport")])
def test_dataparallel_gradient_average_gloo_world2(tmp_path, overlap, case):
    """2 gloo ranks: gradients equal the full-batch ones; with an optional branch (the audio-dropout rule, reference
    model.py:215-222, drawn per replica) dropped on ONE rank the collective schedule still matches and the result is
    the full-batch gradient; dropped on every rank its gradients come back as None; "flip" runs five CONSECUTIVE steps
    whose drop decision changes every step (one rank, both, the other, none, both): the wrapper's per-step state
    (presence flags, pending collectives, fired hooks, the queued callback, the exchanged draw) must reset between them.
    By default the module reports its draw (`optional_parameters_used`) and the ranks exchange it after forward (all /
    none / some replicas -> hook-overlapped / skipped / zero-filled reduction); "-noreport" runs the fallback in which the
    wrapper only learns it from the presence flags at the end of backward"""
    script = tmp_path / "dp_worker.py"
    script.write_text(_DP_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", DP_OVERLAP=str(int(overlap)), DP_CASE=case.replace("-noreport", ""),
                   DP_REPORT="0" if case.endswith("-noreport") else "1")
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"DP_OK {r}" in o, o


_ACC_WORKER = r'''
import os, sys, copy, torch, torch.distributed as dist, torch.nn as nn
sys.path.insert(0, sys.argv[1])
from attention_based_tbn_amd.core.models.dataparallel import DataParallel
from attention_based_tbn_amd.core.utils.train_step import TrainStep
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank = dist.get_rank()
k, clip = int(os.environ["ACC_K"]), float(os.environ["ACC_CLIP"])
class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(8, 16); self.b = nn.Linear(16, 2)
    def forward(self, x): return self.b(torch.relu(self.a(x)))
    def get_loss(self, criterion, target, preds, epoch=0): return {"total": criterion(preds, target) * 50.0}, preds.shape[0]
torch.manual_seed(5)
DataParallel.SMALL = 64                             # a.weight (128 elements) takes the "large tensor" route
model = DataParallel(Toy())
ref = copy.deepcopy(model.module)
opt = torch.optim.SGD(model.parameters(), 0.05, momentum=0.9, weight_decay=1e-3)
ropt = torch.optim.SGD(ref.parameters(), 0.05, momentum=0.9, weight_decay=1e-3)
calls = []
real = dist.all_reduce
def counting(t, *a, **kw):
    calls.append(t.numel())
    return real(t, *a, **kw)
dist.all_reduce = counting
step = TrainStep(model, opt, nn.MSELoss(), accumulator_step=k, clip_grad=clip if clip > 0 else None)
g = torch.Generator().manual_seed(11)
clipped = 0
for it in range(7):
    X = torch.randn(8, 8, generator=g); Y = torch.randn(8, 2, generator=g)
    n0 = len(calls)
    loss, bs = step(it, X[rank * 4:(rank + 1) * 4], Y[rank * 4:(rank + 1) * 4], epoch=0)
    exchanged = len(calls) > n0
    # the reference loop body, literally (core/tools/train.py:66-94), on the full batch in one process
    if (it + 1) % k == 0:
        ropt.zero_grad()
    rl = ref.get_loss(nn.MSELoss(), Y, ref(X))[0]["total"] / k
    rl.backward()
    if clip > 0:
        tn = torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)
        clipped += int(tn > clip)
    stepping = (it + 1) % k == k - 1
    if stepping:
        ropt.step()
    # gradient exchange: every iteration when the clip needs the global accumulated gradient, else on stepping ones only
    assert exchanged == (clip > 0 or stepping), (it, exchanged)
    assert step.synced[-1] == exchanged
    if exchanged:
        assert len(calls) - n0 == 2, calls[n0:]     # a.weight from its hook + the packed small tensors
        for (n, p), q in zip(model.module.named_parameters(), ref.parameters()):
            assert torch.allclose(p.grad, q.grad, rtol=1e-4, atol=2e-5), (it, n)
    for (n, p), q in zip(model.module.named_parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-4, atol=2e-5), (it, n, float((p - q).abs().max()))
        mb, rb = opt.state[p].get("momentum_buffer"), ropt.state[q].get("momentum_buffer")
        assert (mb is None) == (rb is None) and (mb is None or torch.allclose(mb, rb, rtol=1e-4, atol=2e-5)), (it, n)
assert clip == 0 or clipped >= 3, clipped           # the clip really bit (also on re-clipped accumulated gradients)
print("ACC_OK", rank)
dist.destroy_process_group()                        # orderly shutdown: a rank that just exits while c10d's threads still run can abort in teardown
'''


@pytest.mark.parametrize("k,clip", [(1, 2.0), (2, 0.0), (2, 2.0), (3, 0.0), (3, 2.0)])
def test_accumulation_schedule_gloo_world2(tmp_path, k, clip):
    """`TrainStep` (reference core/tools/train.py:66-94) under data parallelism, 2 gloo ranks, seven iterations at
    accumulator_step = k against the reference loop body run literally on the full batch in one process: parameters and
    momentum buffers agree after every iteration; without clipping the gradient all-reduce happens on the stepping
    iterations only (`DataParallel.no_sync()` elsewhere), with clipping on every iteration (the clip coefficient is a
    function of the GLOBAL accumulated gradient)"""
    script = tmp_path / "acc_worker.py"
    script.write_text(_ACC_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", ACC_K=str(k), ACC_CLIP=str(clip))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"ACC_OK {r}" in o, o


_ACC_OPT_WORKER = r'''
import os, sys, copy, torch, torch.distributed as dist, torch.nn as nn
sys.path.insert(0, sys.argv[1])
from attention_based_tbn_amd.core.models.dataparallel import DataParallel
from attention_based_tbn_amd.core.utils.train_step import TrainStep
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank = dist.get_rank()
k, clip, report = int(os.environ["ACC_K"]), float(os.environ["ACC_CLIP"]), os.environ["ACC_REPORT"] == "1"
class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(8, 16); self.b = nn.Linear(16, 2)
        self.c = nn.Linear(8, 16)                   # the "audio" branch: each replica may drop it in any iteration
        self.drop = False
    def maybe_unused_parameter_prefixes(self): return ["c."]
    if report:
        def optional_parameters_used(self): return not self.drop
    def forward(self, x):
        h = torch.relu(self.a(x))
        return self.b(h if self.drop else h + self.c(x))
    def get_loss(self, criterion, target, preds, epoch=0): return {"total": criterion(preds, target) * 50.0}, preds.shape[0]
torch.manual_seed(5)
DataParallel.SMALL = 64                             # a.weight / c.weight (128 elements) take the "large tensor" route
model = DataParallel(Toy())
ref = copy.deepcopy(model.module)
opt = torch.optim.SGD(model.parameters(), 0.05, momentum=0.9, weight_decay=1e-3)
ropt = torch.optim.SGD(ref.parameters(), 0.05, momentum=0.9, weight_decay=1e-3)
step = TrainStep(model, opt, nn.MSELoss(), accumulator_step=k, clip_grad=clip if clip > 0 else None)
g = torch.Generator().manual_seed(11)
# (rank 0 drops, rank 1 drops) per iteration: one rank, nobody keeps it, both keep it, the other rank, ... -- windows in
# which only an EARLIER iteration produced the optional gradient (on one rank, on both) are all in here for k = 2 and 3
drops = [(False, True), (True, True), (False, False), (True, False), (True, True), (True, True), (False, True),
         (True, True), (False, False), (True, True), (True, False)]
for it, dr in enumerate(drops):
    X = torch.randn(8, 8, generator=g); Y = torch.randn(8, 2, generator=g)
    model.module.drop = dr[rank]
    loss, bs = step(it, X[rank * 4:(rank + 1) * 4], Y[rank * 4:(rank + 1) * 4], epoch=0)
    # the reference loop body (core/tools/train.py:66-94) in ONE process: nn.DataParallel adds the replicas' gradients of
    # their own chunk's loss into the master .grad on every backward -- each replica with its own draw
    if (it + 1) % k == 0:
        ropt.zero_grad()
    total = 0
    for r in range(2):
        ref.drop = dr[r]
        total = total + ref.get_loss(nn.MSELoss(), Y[r * 4:(r + 1) * 4], ref(X[r * 4:(r + 1) * 4]))[0]["total"] / 2
    (total / k).backward()
    if clip > 0:
        torch.nn.utils.clip_grad_norm_([p for p in ref.parameters() if p.grad is not None], clip)
    stepping = (it + 1) % k == k - 1
    if stepping:
        ropt.step()
    if step.synced[-1]:                             # gradients were exchanged: they are the reference's accumulated ones
        for (n, p), q in zip(model.module.named_parameters(), ref.parameters()):
            assert (p.grad is None) == (q.grad is None), (it, n, p.grad is None, q.grad is None)
            assert p.grad is None or torch.allclose(p.grad, q.grad, rtol=1e-4, atol=2e-5), (it, n, float((p.grad - q.grad).abs().max()))
    for (n, p), q in zip(model.module.named_parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-4, atol=2e-5), (it, n, float((p - q).abs().max()))
        mb, rb = opt.state[p].get("momentum_buffer"), ropt.state[q].get("momentum_buffer")
        assert (mb is None) == (rb is None) and (mb is None or torch.allclose(mb, rb, rtol=1e-4, atol=2e-5)), (it, n)
    assert model._pending == [] and not model._callback_queued and (step.synced[-1] != model._unsynced)
assert len(step.synced) == len(drops)
print("ACCOPT_OK", rank)
dist.destroy_process_group()                        # orderly shutdown: a rank that just exits while c10d's threads still run can abort in teardown
'''


@pytest.mark.parametrize("k,clip,report", [(2, 0.0, True), (3, 0.0, True), (2, 2.0, True), (3, 2.0, True), (2, 0.0, False),
                                           (3, 2.0, False), (1, 2.0, True)])
def test_accumulation_with_optional_branch_gloo_world2(tmp_path, k, clip, report):
    '''round-5 advisor: `TrainStep` with accumulator_step = k under data parallelism when a replica may DROP an optional
    branch in any iteration (the audio-dropout rule, reference core/models/model.py:215-222, one draw per replica and
    forward).  The reference keeps accumulating into .grad and steps on it (core/tools/train.py:71-94): a gradient an
    earlier iteration of the window produced must survive a later iteration in which this rank -- or every rank --
    dropped the branch, with and without clipping (per-iteration exchange) and with and without the module reporting its
    draw.  Eleven iterations against the reference loop replayed in one process, parameters / momentum after each.
    (Six of the seven cases fail on the round-5 wrapper, which zero-filled / dropped what had accumulated.)'''
    script = tmp_path / "accopt_worker.py"
    script.write_text(_ACC_OPT_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", ACC_K=str(k), ACC_CLIP=str(clip), ACC_REPORT=str(int(report)))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"ACCOPT_OK {r}" in o, o


_BUCKET_WORKER = r'''
import os, sys, copy, torch, torch.distributed as dist, torch.nn as nn
sys.path.insert(0, sys.argv[1])
from attention_based_tbn_amd.core.models.dataparallel import DataParallel, PlanSync
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank = dist.get_rank()
class FlatFn(torch.autograd.Function):
    # a stand-in for the backbone's autograd node (core/models/bn_inception.py _BackboneFn): ONE flat weight tensor whose
    # gradient becomes final slice by slice, top down, and is announced through `grad_bucket_fn` from INSIDE backward
    @staticmethod
    def forward(ctx, x, w, module):
        ctx.save_for_backward(x, w); ctx.module = module
        return x @ w.view(12, 8).t()
    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dw = (g.t() @ x).reshape(-1)
        waits, fn = [], ctx.module.grad_bucket_fn
        if fn is not None:
            for lo, hi in ((56, 96), (24, 56)):            # what the engine's bucket_cb reports: suffixes of the flat tensor
                wt = fn(ctx.module.flat, dw, lo, hi)
                if wt is not None: waits.append(wt)
        for wt in waits: wt()
        return g @ w.view(12, 8), dw, None
class Toy(nn.Module):
    def __init__(self, tag):
        super().__init__()
        self.flat = nn.Parameter(torch.randn(96) * 0.3); self.head = nn.Linear(12, 2)
        self.grad_bucket_fn = None                         # DataParallel installs its _on_grad_bucket here
        self.plan_sync = None
    def forward(self, x): return self.head(torch.relu(FlatFn.apply(x, self.flat, self)))
class Two(nn.Module):
    def __init__(self):
        super().__init__()
        self.m1 = Toy(1); self.m2 = Toy(2)
    def forward(self, x): return self.m1(x) + self.m2(x * 0.5)
torch.manual_seed(3)
DataParallel.SMALL = 32                             # the 32-element slices travel alone, the heads (24 + 2) are packed
model = DataParallel(Two())
assert model.module.m1.grad_bucket_fn is not None and isinstance(model.module.m1.plan_sync, PlanSync)
ref = copy.deepcopy(model.module)
for m in ref.modules():
    if hasattr(m, "grad_bucket_fn"): m.grad_bucket_fn = None
calls = []
real = dist.all_reduce
def counting(t, *a, **kw):
    calls.append(t.numel())
    return real(t, *a, **kw)
dist.all_reduce = counting
g = torch.Generator().manual_seed(9)
X = torch.randn(8, 8, generator=g); Y = torch.randn(8, 2, generator=g)
def step(zero):
    if zero:
        model.zero_grad(set_to_none=True); ref.zero_grad(set_to_none=True)
    n0 = len(calls); model.bucket_log.clear()
    nn.MSELoss()(model(X[rank * 4:(rank + 1) * 4]), Y[rank * 4:(rank + 1) * 4]).backward()
    nn.MSELoss()(ref(X), Y).backward()
    for (n, p), q in zip(model.module.named_parameters(), ref.parameters()):
        assert torch.allclose(p.grad, q.grad, atol=1e-6), (n, float((p.grad - q.grad).abs().max()))
    assert model._pending == [] and model._bucketed == {} and not model._callback_queued
    return calls[n0:]
# fresh gradients: per flat tensor two buckets from inside its backward (top slice first; the second module's node runs
# first: reverse of forward); the remaining prefixes (24 elements each) only at the END of backward, behind every bucket of
# every module -- collectives execute in issue order, and a prefix is final only when its module's whole backward has run,
# so issued from the hook it would hold up the next module's buckets -- then the packed small tensors (two heads:
# 2 x (24 + 2) elements) last.  Same sequence on both ranks by construction.
c = step(True)
assert c == [40, 32, 40, 32, 24, 24, 52], c
assert model.bucket_log == [(96, 56, 96), (96, 24, 56), (96, 56, 96), (96, 24, 56)], model.bucket_log
# accumulating into an existing .grad (no zero_grad): a bucket would average only the NEW part -> the whole tensor takes
# the ordinary hook path, after the local accumulation
c = step(False)
assert c == [96, 96, 52] and model.bucket_log == [], (c, model.bucket_log)
# under no_sync nothing is exchanged at all, and the next synchronised backward on the accumulated sums takes the hook path
model.zero_grad(set_to_none=True); ref.zero_grad(set_to_none=True)
with model.no_sync():
    n0 = len(calls)
    nn.MSELoss()(model(X[rank * 4:(rank + 1) * 4]), Y[rank * 4:(rank + 1) * 4]).backward()
    assert calls[n0:] == [] and model.bucket_log == []
nn.MSELoss()(ref(X), Y).backward()
c = step(False)
assert c == [96, 96, 52], c
# overlap=False (diagnostic): every collective at the end of backward, no buckets
model.overlap = False
c = step(True)
assert sorted(c) == [52, 96, 96] and model.bucket_log == [], c
model.overlap = True
# plan exchange keys (PlanSync.check): equal keys pass, different keys raise on EVERY rank (round-5 advisor)
sync = model.module.m1.plan_sync
sync.check((3, 96, 224, 224, 1), torch.device("cpu"))
try:
    sync.check((3, 96 + rank, 224, 224, 1), torch.device("cpu"))
    raise SystemExit("differing plan keys were not detected")
except RuntimeError as e:
    assert "different problems" in str(e), e
print("BUCKET_OK", rank)
dist.destroy_process_group()                        # orderly shutdown: a rank that just exits while c10d's threads still run can abort in teardown
'''


def test_gradient_buckets_and_plan_keys_gloo_world2(tmp_path):
    '''round-5 verdict item 2: a backbone's flat weight gradient is exchanged in buckets that complete at different times
    (engine callback tbn_backbone_grads.bucket_cb -> BNInception.grad_bucket_fn -> DataParallel._on_grad_bucket; the
    reference reduces per backward: core/models/model_builder.py:73-75, SURVEY 8e "bucketed, launched as backward produces
    them").  Two gloo ranks, a stand-in autograd node that announces its slices like the engine does: the collective ORDER
    (buckets top-down from inside each node's backward, the remaining prefix from the hook, packed small tensors last) is
    asserted element count by element count, the averaged result equals the full-batch gradient; accumulation / no_sync /
    overlap=False fall back to whole-tensor collectives.  Also PlanSync.check (advisor): differing plan keys raise on
    every rank instead of pairing a blob with the wrong plan.'''
    script = tmp_path / "bucket_worker.py"
    script.write_text(_BUCKET_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"BUCKET_OK {r}" in o, o


def test_torch_fp32_cpu_norm_of_a_backbone_sized_gradient_is_low():
    """Pins the claim behind the float64 replay of tests/test_trainstep_gpu.py::_reference_loop (round-5 commit 206762b,
    round-5 verdict "Parity" item 4): torch's fp32 CPU 2-norm of a 10-M-element tensor -- what clip_grad_norm_ computes
    for a backbone's flat weight gradient (reference core/tools/train.py:84-91) -- accumulates the squares sequentially in
    fp32 and comes out LOW, by 3e-4 (normal data) to 7.5e-3 (equal magnitudes) of the true norm, whatever the thread
    count; the clip coefficient inherits the error.  A blocked sum (fp32 inside 4096-element blocks, fp64 across them:
    the shape of the HIP kernel's fp64-finalised partials, csrc/train_ops.hip) agrees with float64 to 1e-6.  So a float64
    replay is the exact statement of the reference's arithmetic and the fp32 CPU replay the less accurate side -- that is
    why the accumulation test compares against float64, not a loosened tolerance."""
    import torch
    n = 10_240_000                        # about the floats of a backbone flat weight tensor (10.24 M), a multiple of 4096
    g = torch.Generator().manual_seed(0)
    cases = {"normal": torch.randn(n, generator=g) * 0.02,
             "equal magnitudes": torch.full((n,), 0.0224) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float(),
             "heavy tailed": torch.randn(n, generator=g) * 0.02 * torch.rand(n, generator=g) ** 4}
    for name, t in cases.items():
        n64 = float(torch.linalg.vector_norm(t.double()))
        p = torch.nn.Parameter(t.clone())
        p.grad = t.clone()
        n32 = float(torch.nn.utils.clip_grad_norm_([p], 1e9))        # what the reference loop calls
        deficit = (n64 - n32) / n64
        assert 1e-4 < deficit < 2e-2, (name, n32, n64, deficit)      # systematically LOW, far beyond the 2e-6 the test asserts
        blocks = (t * t).view(-1, 4096).sum(1)                       # fp32 within a block ...
        blocked = float(blocks.double().sum().sqrt())                # ... fp64 across blocks
        assert abs(blocked - n64) / n64 < 1e-6, (name, blocked, n64)


def test_shipped_library_and_models_read_no_environment_knobs():
    """round-5 verdict item 7: A/B knobs exist only in a -DTBN_EXPERIMENT=1 build.  The shipped libtbn_hip.so does not even IMPORT
    getenv (every knob folds to its default at compile time: csrc/tbn_common.h), says so in tbn_version() (bit 16 clear), and the
    Python product reads the environment in exactly two documented places: the library override for diagnostic builds
    (TBN_LIB, _lib.py) and the opt-in plan cache (TBN_PLAN_CACHE, bn_inception.py) -- core/models/model.py reads none."""
    import re
    import subprocess
    from attention_based_tbn_amd import _lib
    if os.environ.get("TBN_LIB"):
        pytest.skip("TBN_LIB points at a diagnostic / experiment build")
    assert _lib.lib().tbn_version() & 0x10000 == 0
    syms = subprocess.run(["nm", "-D", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in syms and "tbn_env_int" not in syms, [l for l in syms.splitlines() if "env" in l]
    pkg = os.path.join(ROOT, "attention_based_tbn_amd")
    hits = []
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f != "build.py":
                for i, line in enumerate(open(os.path.join(d, f)), 1):
                    if re.search(r"os\.environ|getenv", line):
                        hits.append((os.path.relpath(os.path.join(d, f), pkg), re.findall(r"TBN_[A-Z_]+", line)))
    assert all(f in ("_lib.py", os.path.join("core", "models", "bn_inception.py")) for f, _ in hits), hits
    assert {k for _, ks in hits for k in ks} <= {"TBN_LIB", "TBN_PLAN_CACHE"}, hits


def test_plan_create_accepts_exactly_the_sizes_the_reference_graph_accepts():
    """inception_3c / 4e concatenate stride-2 conv branches (floor) with a ceil-mode max pool: for some input sizes
    the reference's torch.cat raises.  The engine plan must refuse those sizes (it would otherwise write a pooled
    slice of the wrong extent) and accept all others.  Host-only: plan_create needs no GPU."""
    import ctypes as C
    import torch
    from attention_based_tbn_amd._lib import lib
    from oracle.bninception import BNInception as OBN
    L = lib()
    m = OBN(1000, 3).eval()
    seen = set()
    for h in range(32, 120, 11):
        for w in (32, 57, 75, 80, 91, 112):
            hd = C.c_void_p()
            rc = L.tbn_backbone_plan_create(3, 1, h, w, C.byref(hd))
            try:
                with torch.no_grad():
                    m.features(torch.zeros(1, 3, h, w))
                ok = True
            except RuntimeError:
                ok = False
            assert (rc == 0) == ok, (h, w, rc, ok)
            seen.add(ok)
            if rc == 0:
                L.tbn_backbone_plan_destroy(hd)
            else:
                assert b"not a valid BN-Inception size" in L.tbn_last_error()
    assert seen == {True, False}


def test_c_abi_rejects_bad_arguments_before_touching_the_gpu():
    """argument validation happens on the host, ahead of any launch: every call below must fail with a negative
    status and a message -- and must not need a GPU to do so"""
    import ctypes as C
    from attention_based_tbn_amd._lib import OptTensor, lib
    L = lib()
    bad = 0x1000   # never dereferenced: validation fails first

    def fails(rc, needle):
        assert rc < 0, rc
        msg = L.tbn_last_error().decode()
        assert needle in msg, msg

    h = C.c_void_p()
    fails(L.tbn_backbone_plan_create(3, 1, 16, 16, C.byref(h)), "unsupported shape")
    fails(L.tbn_backbone_plan_create(3, 1, 75, 91, C.byref(h)), "not a valid BN-Inception size")
    # one engine call addresses at most 2 GiB per tensor: refused when the plan is made, not at some launch mid-pass
    fails(L.tbn_backbone_plan_create(1, 512, 256, 256, C.byref(h)), "at most 2 GiB per tensor")
    fails(L.tbn_backbone_plan_create(3, 700, 224, 224, C.byref(h)), "at most 2 GiB per tensor")
    assert L.tbn_backbone_plan_create(1, 511, 256, 256, C.byref(h)) == 0      # the largest audio batch of one call
    L.tbn_backbone_plan_destroy(h)
    # frames pipeline: box / crop outside their parent, stack not dividing the frame count
    fails(L.tbn_frames_to_tensor(bad, 4, 64, 64, 3, 10, 10, 60, 60, 32, 32, 0, 0, 32, 32, 0, 1, None, None, 0, 1, bad, None),
          "outside the 64x64 frame")
    fails(L.tbn_frames_to_tensor(bad, 4, 64, 64, 3, 0, 0, 64, 64, 32, 32, 8, 8, 32, 32, 0, 1, None, None, 0, 1, bad, None),
          "outside the resized")
    fails(L.tbn_frames_to_tensor(bad, 7, 64, 64, 1, 0, 0, 64, 64, 64, 64, 0, 0, 64, 64, 0, 10, None, None, 0, 1, bad, None),
          "bad frame stack")
    # optimiser: too many tensors in one call, unaligned pointer, null gradient
    many = (OptTensor * 49)(*[OptTensor(bad, bad, bad, 4)] * 49)
    fails(L.tbn_opt_sgd_step(many, 49, 0.1, 0.9, 0.0, None, None), "tensors per call")
    one = (OptTensor * 1)(OptTensor(bad, bad + 2, bad, 4))
    fails(L.tbn_opt_sgd_step(one, 1, 0.1, 0.9, 0.0, None, None), "4-byte aligned")
    one = (OptTensor * 1)(OptTensor(bad, 0, bad, 4))
    fails(L.tbn_opt_sqnorm_partials(one, 1, bad, None), "null pointer")
    # metrics: k larger than the number of classes
    fails(L.tbn_topk_correct(bad, 10, bad, 4, 10, 11, bad, None, None, None), "bad shape")
    # conv: K not a multiple of 32 (cin = 10, 3x3)
    fails(L.tbn_conv2d_fwd(bad, 10, bad, bad, bad, 64, 2, 8, 8, 10, 64, 3, 1, 1, 0, 0, None, None, None, None),
          "multiples of 32")
    # stem entries: null pointers, channel count, cout, layout, epilogue operands, tiles
    geo = (C.c_int * 8)()
    fails(L.tbn_stem_geometry(3, 32, 32, 0, None), "null out")
    fails(L.tbn_stem_geometry(0, 32, 32, 0, geo), "outside 1..16")
    fails(L.tbn_stem_geometry(17, 32, 32, 0, geo), "outside 1..16")
    fails(L.tbn_stem_geometry(3, 32, 32, 3, geo), "layout 3")
    fails(L.tbn_stem_geometry(3, 0, 32, 0, geo), "bad shape")
    assert L.tbn_stem_workspace_floats(0, 32, 32, 0, 1, 64) == 0 and L.tbn_stem_workspace_floats(3, 32, 32, 0, 1, 40) == 0

    def stem_fwd(x=bad, wt=bad, out=bad, out_ld=64, n=2, h=17, w=19, cin=3, cout=64, layout=0, epi=0, scale=None, shift=None,
                 part=None, mt=0, nt=0, stages=0, ws=bad):
        return L.tbn_stem_conv_fwd(x, wt, None, out, out_ld, n, h, w, cin, cout, layout, epi, scale, shift, part, mt, nt, stages,
                                   ws, None)

    def stem_wgrad(dy=bad, dy_ld=64, x=bad, dw=bad, n=2, h=17, w=19, cin=3, cout=64, layout=0, mt=0, nt=0, ws=bad):
        return L.tbn_stem_conv_wgrad(dy, dy_ld, x, dw, n, h, w, cin, cout, layout, mt, nt, ws, None)
    for kw in (dict(x=None), dict(wt=None), dict(out=None), dict(ws=None)):
        fails(stem_fwd(**kw), "stem_conv_fwd: null pointer")
    for kw in (dict(dy=None), dict(x=None), dict(dw=None), dict(ws=None)):
        fails(stem_wgrad(**kw), "stem_conv_wgrad: null pointer")
    for f, who in ((stem_fwd, "stem_conv_fwd"), (stem_wgrad, "stem_conv_wgrad")):
        fails(f(cin=0), who + ": cin 0 outside 1..16")
        fails(f(cin=17), who + ": cin 17 outside 1..16")
        fails(f(cout=40), who + ": cout 40 must be a multiple of 32")
        fails(f(layout=3), who + ": layout 3")
        fails(f(layout=-1), who + ": layout -1")
        fails(f(h=0), who + ": bad shape")
        fails(f(n=0), who + ": bad shape")
        fails(f(ws=bad + 4), who + ": the workspace must be 16-B aligned")
        fails(f(n=1 << 20, h=224, w=224), "exceeds 2 GiB")
    fails(stem_fwd(epi=1), "stats epilogue needs stat_partial")
    fails(stem_fwd(epi=2), "eval epilogue needs scale/shift")
    fails(stem_fwd(epi=2, scale=bad), "eval epilogue needs scale/shift")
    fails(stem_fwd(epi=3), "bad epilogue")
    fails(stem_fwd(out_ld=32), "out_ld 32 below cout 64")
    fails(stem_fwd(mt=3, nt=1), "tile 3x1")
    fails(stem_fwd(mt=1, nt=0), "tile 1x0")
    fails(stem_fwd(stages=3), "stages 3")
    fails(stem_wgrad(dy_ld=62), "dy_ld 62")
    fails(stem_wgrad(mt=4, nt=1), "tile 4x1")
    fails(stem_wgrad(mt=5, nt=3), "tile 5x3")
    fails(stem_wgrad(mt=0, nt=2), "tile 0x2")
    # the conv weight gradient with an explicit tile, and its host-only plan query: the same tile rule, pitches, multiples of 4
    # (every refusal of the two: tests/test_wgrad_plan_cpu.py)
    def conv_wgrad(dy=bad, dy_ld=64, x=bad, x_ld=32, dw=bad, mt=0, nt=0):
        return L.tbn_conv2d_wgrad_tile(dy, dy_ld, x, x_ld, dw, 2, 8, 8, 32, 64, 3, 1, 1, mt, nt, None, None)
    for kw in (dict(dy=None), dict(x=None), dict(dw=None)):
        fails(conv_wgrad(**kw), "conv2d_wgrad_tile: null pointer")
    for mt, nt in ((4, 1), (5, 3), (0, 2), (2, 0), (1, 4)):
        fails(conv_wgrad(mt=mt, nt=nt), "conv2d_wgrad_tile: tile %dx%d (mt 1 | 2 | 3 | 5, nt 1..3 without 5x3, or 0x0)" % (mt, nt))
        fails(L.tbn_conv2d_wgrad_plan(2, 8, 8, 32, 64, 3, 1, 1, mt, nt, geo), "conv2d_wgrad_plan: tile %dx%d" % (mt, nt))
    fails(conv_wgrad(dy_ld=60), "dout_ld 60")
    fails(conv_wgrad(x_ld=28), "in_ld 28")
    fails(conv_wgrad(x_ld=34), "in_ld 34")
    # batched training BN: the launchers' shape rules (bn_multi.hip) and null pointers, before any launch
    from attention_based_tbn_amd._lib import BnBwdDesc, BnFwdDesc, BnSeg

    def bn_fwd(n=1, **kw):
        d = BnFwdDesc()
        for k in ("y", "partial", "gamma", "beta", "running_mean", "running_var", "save_mean", "save_rstd", "scale", "shift"):
            setattr(d, k, bad)
        d.y_ld, d.p, d.c, d.pld, d.nparts, d.nseg = 32, 8, 32, 32, 1, 1
        d.seg[0] = BnSeg(bad, 32, 0)
        seg = kw.pop("seg", None)
        for k, v in kw.items():
            setattr(d, k, v)
        for i, sg in enumerate(seg or ()):
            d.seg[i] = sg
        arr = (BnFwdDesc * 5)(*[d] * 5)
        return L.tbn_bn_fwd_batch(arr, n, 0.1, 1e-5, None)

    def bn_bwd(n=1, **kw):
        d = BnBwdDesc()
        for k in ("y", "dy", "scale", "shift", "mean", "rstd", "partial", "coef", "dgamma", "dbeta", "dbias"):
            setattr(d, k, bad)
        d.y_ld, d.p, d.c, d.nseg = 32, 8, 32, 1
        d.dz[0] = BnSeg(bad, 32, 0)
        seg = kw.pop("seg", None)
        for k, v in kw.items():
            setattr(d, k, v)
        for i, sg in enumerate(seg or ()):
            d.dz[i] = sg
        arr = (BnBwdDesc * 5)(*[d] * 5)
        return L.tbn_bn_bwd_batch(arr, n, None)
    for f, who in ((bn_fwd, "bn_fwd"), (bn_bwd, "bn_bwd")):
        fails(f(n=0), who + "_multi: 0 layers")
        fails(f(n=5), who + "_multi: 5 layers")
        fails(f(n=-1), who + "_multi: -1 layers")
        for kw in (dict(c=30), dict(c=1028, y_ld=1028, pld=1028), dict(c=0), dict(p=0), dict(y_ld=28), dict(y_ld=34), dict(nseg=0),
                   dict(nseg=4, seg=[BnSeg(bad, 32, 0), BnSeg(bad, 32, 8), BnSeg(bad, 32, 16)])):
            if who == "bn_bwd":
                kw.pop("pld", None)
            fails(f(**kw), who + "_multi: bad P / C / pitch")
        fails(f(seg=[BnSeg(bad, 34, 0)]), who + "_multi: segment pitch/offset must be x4")
        fails(f(nseg=2, seg=[BnSeg(bad, 32, 0), BnSeg(bad, 32, 18)]), who + "_multi: segment pitch/offset must be x4")
        fails(f(seg=[BnSeg(0, 32, 0)]), who + "_batch: null pointer in segment 0 of member 0")
        fails(f(nseg=3, seg=[BnSeg(bad, 32, 0), BnSeg(bad, 32, 8), BnSeg(0, 32, 16)]), who + "_batch: null pointer in segment 2")
        fails(f(n=4, y=None), who + "_batch: null pointer in member 0")
    fails(bn_fwd(pld=28), "bn_fwd_multi: bad P / C / pitch")
    fails(bn_fwd(pld=34), "bn_fwd_multi: bad P / C / pitch")
    fails(bn_fwd(nparts=0), "bn_fwd_multi: bad P / C / pitch")
    fails(bn_bwd(ext_parts=-1), "bn_bwd_multi: bad P / C / pitch")
    for k in ("partial", "gamma", "beta", "save_mean", "save_rstd", "scale", "shift"):
        fails(bn_fwd(**{k: None}), "bn_fwd_batch: null pointer in member 0")
    fails(bn_fwd(running_var=None), "running_mean without running_var")
    for k in ("dy", "scale", "shift", "mean", "rstd", "partial", "coef"):
        fails(bn_bwd(**{k: None}), "bn_bwd_batch: null pointer in member 0")
    fails(L.tbn_bn_fwd_batch(None, 1, 0.1, 1e-5, None), "bn_fwd_batch: null pointer")
    fails(L.tbn_bn_bwd_batch(None, 1, None), "bn_bwd_batch: null pointer")
    nparts = C.c_int(0)
    fails(L.tbn_bn_stats_partials(None, 32, 8, 32, bad, C.byref(nparts), None), "bn_stats_partials: null pointer")
    fails(L.tbn_bn_stats_partials(bad, 32, 8, 32, bad, None, None), "bn_stats_partials: null pointer")
    for y_ld, p_, c_ in ((28, 8, 32), (34, 8, 32), (32, 0, 32), (32, 8, 30), (1028, 8, 1028), (32, 8, 0)):
        fails(L.tbn_bn_stats_partials(bad, y_ld, p_, c_, bad, C.byref(nparts), None), "bn_stats: P >= 1, C a multiple of 4")
    assert L.tbn_bn_bwd_partial_floats(0, 32) == 0 and L.tbn_bn_bwd_partial_floats(8, 30) == 0
    assert L.tbn_bn_bwd_partial_floats(8, 1028) == 0 and L.tbn_bn_bwd_partial_floats(8, 0) == 0
    # rows per reduce workgroup: max(64, ceil(p / 512)) rounded up to the 256 / (c / 4) row lanes
    assert L.tbn_bn_bwd_partial_floats(5000, 1024) == 79 * 2 * 1024 and L.tbn_bn_bwd_partial_floats(5000, 4) == 20 * 2 * 4
    assert L.tbn_bn_bwd_partial_floats(100000, 32) == 447 * 2 * 32 and L.tbn_bn_bwd_partial_floats(1, 100) == 200
    # descriptor entry points (round 3): host-side validation of every form they can express
    from attention_based_tbn_amd._lib import ConvDesc

    def desc(**kw):
        d = ConvDesc()
        d.inp, d.in_ld, d.weight, d.out, d.out_ld = bad, 32, bad, bad, 32
        d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = 1, 8, 8, 32, 32, 3, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    fails(L.tbn_conv_launch(C.byref(desc(epilogue=1)), 1, 1, None, None), "stat_partial")
    fails(L.tbn_conv_launch(C.byref(desc(epilogue=2)), 1, 1, None, None), "scale/shift")
    fails(L.tbn_conv_launch(C.byref(desc(nred=1)), 1, 1, None, None), "belongs to a data gradient")
    fails(L.tbn_conv_launch(C.byref(desc(dgrad=1)), 1, 1, None, None), "flipped-weight workspace")
    fails(L.tbn_conv_launch(C.byref(desc(inp=0)), 1, 1, None, None), "null pointer")
    # partial rows: 128-row tiles (32 for the split-K tile variant), per parity phase for a strided data gradient
    assert L.tbn_conv_partial_rows(C.byref(desc(n=3, h=14, w=14)), 1, 0) == 5
    assert L.tbn_conv_partial_rows(C.byref(desc(n=3, h=14, w=14, flags=16)), 1, 0) == 19
    assert L.tbn_conv_partial_rows(C.byref(desc(n=3, h=14, w=14, flags=16)), 1, 1) == 5      # a pair uses 128-row tiles
    assert L.tbn_conv_partial_rows(C.byref(desc(n=2, h=15, w=15, stride=2, dgrad=1)), 1, 0) == 4   # 8x8, 8x7, 7x8, 7x7 phases


def test_stem_geometry_matches_the_closed_forms():
    """tbn_stem_geometry (host only) against the closed forms of the layout comments in csrc/pool.hip, for every channel
    count the plan admits and sizes of every parity, down to maps smaller than the filter: the space-to-depth image is
    (ceil(h/2)+3) x (ceil(w/2)+3) pixels of 4 cin floats with K = 64 cin; the row-runs image (2(oh-1)+8) x (2(ow-1)+8)
    pixels of cin floats with runs of rl = 7 cin rounded up to x4 and K = 7 rl rounded up to x32.  The rule (layout 0)
    takes row runs exactly when their K is the smaller one: from 4 channels on."""
    import ctypes as C
    from attention_based_tbn_amd._lib import lib
    L = lib()
    header = open(os.path.join(ROOT, "include", "tbn_hip.h")).read()
    assert re.search(r"^#define TBN_CAP_STEM_OPS 64$", header, re.M)
    assert L.tbn_capabilities() & 64 and (L.tbn_version() & 0xffff) == 102
    up = lambda v, m: (v + m - 1) // m * m
    out = (C.c_int * 8)()
    residues, switch = set(), []
    for cin in range(1, 17):
        rl = up(7 * cin, 4)
        residues.add(rl - 7 * cin)
        want = {
            1: lambda h, w: [1, (h + 1) // 2 + 3, (w + 1) // 2 + 3, 4 * cin, 16 * cin, 64 * cin, 64 * cin],
            2: lambda h, w: [2, 2 * ((h - 1) // 2) + 8, 2 * ((w - 1) // 2) + 8, cin, rl, up(7 * rl, 32), 7 * rl],
        }
        rule = 2 if up(7 * rl, 32) < 64 * cin else 1
        assert rule == (1 if cin <= 3 else 2)
        switch.append(rule)
        for h, w in ((17, 19), (16, 22), (15, 18), (18, 13), (7, 7), (32, 32), (1, 1), (2, 1), (224, 224), (70, 129)):
            for layout in (0, 1, 2):
                assert L.tbn_stem_geometry(cin, h, w, layout, out) == 0
                exp = want[layout or rule](h, w)
                exp.append(exp[1] * exp[2] * exp[3])
                assert list(out) == exp, (cin, h, w, layout, list(out), exp)
                assert exp[5] % 32 == 0 and exp[4] % 4 == 0 and exp[5] >= exp[6]
                # the workspace holds the four regions (each rounded up to 256 B); the slabs are at least nothing
                n, cout = 3, 64
                floor = sum(up(v, 64) for v in (n * exp[7], cout * exp[5], cout * exp[6]))
                assert L.tbn_stem_workspace_floats(cin, h, w, layout, n, cout) >= floor
    assert residues == {0, 1, 2, 3} and switch == [1] * 3 + [2] * 13


def test_launch_info_reports_the_plan_choices_per_mode():
    """tbn_backbone_launch_info on a fresh plan (host only): size-heuristic tiles for both modes, no data-gradient
    entries in eval mode or for the stem, an error for an unknown layer"""
    import ctypes as C
    from attention_based_tbn_amd._lib import lib
    L = lib()
    h = C.c_void_p()
    assert L.tbn_backbone_plan_create(3, 4, 96, 96, C.byref(h)) == 0
    buf = (C.c_int * 16)()
    for training in (0, 1):
        assert L.tbn_backbone_launch_info(h, b"inception_4a_3x3", training, buf) == 0
        v = list(buf)
        assert v[0] == 0 and v[1] in (1, 2) and 1 <= v[2] <= 4 and v[4] == 0          # untuned: generic kernel, no pairing
        assert (v[8:] == [0] * 8) == (training == 0) or v[9] >= 1
    assert L.tbn_backbone_launch_info(h, b"conv1_7x7_s2", 1, buf) == 0 and list(buf)[8:] == [0] * 8   # the stem has no data gradient
    assert L.tbn_backbone_launch_info(h, b"no_such_layer", 1, buf) < 0 and b"unknown conv" in L.tbn_last_error()
    L.tbn_backbone_plan_destroy(h)


def test_warmup_scheduler_and_build_optimizer_known_answers():
    """reference core/tools/train.py:190-217,291-295: SGD + MultiStepLR(+ GradualWarmupScheduler) / Adam.  The warm-up
    class restates the third-party `warmup_scheduler` package (absent from the image: parity unpinned) -- known answers:
    multiplier 1 ramps 0 -> base over `epochs`, then the wrapped MultiStepLR counts from the end of the warm-up; multiplier
    m ramps base -> m * base and the wrapped scheduler continues from m * base."""
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.utils import FusedSGD, GradualWarmupScheduler, build_optimizer
    net = torch.nn.Linear(4, 2)
    cfg = load_config(["train.warmup.enable=True", "train.warmup.epochs=4", "train.warmup.multiplier=1",
                       "train.scheduler.lr_steps=[3]", "train.optim.lr=0.1"])
    opt, sched, warm = build_optimizer(cfg, net)
    assert isinstance(opt, FusedSGD) and isinstance(warm, GradualWarmupScheduler) and warm.after_scheduler is sched
    assert opt.param_groups[0]["momentum"] == cfg.train.optim.momentum
    lrs = []
    for epoch in range(9):
        lrs.append(opt.param_groups[0]["lr"])
        warm.step(epoch + 1)                       # train.py:293
    # step(e) for e <= 4: base * e / 4; step(5): hand-over (lr = the wrapped scheduler's, 0.1); step(6), step(7): the wrapped
    # MultiStepLR at epochs 2, 3 -> its milestone 3 is reached by step(7)
    want = [0.0, 0.025, 0.05, 0.075, 0.1, 0.1, 0.1, 0.01, 0.01]
    assert all(abs(a - b) < 1e-12 for a, b in zip(lrs, want)), lrs
    cfg2 = load_config(["train.warmup.enable=True", "train.warmup.epochs=2", "train.warmup.multiplier=3",
                        "train.scheduler.lr_steps=[100]", "train.optim.lr=0.1"])
    opt2, _, warm2 = build_optimizer(cfg2, net)
    seq = []
    for epoch in range(5):
        seq.append(round(opt2.param_groups[0]["lr"], 12))
        warm2.step(epoch + 1)
    # (step(3) is the hand-over: the package returns the wrapped scheduler's LAST lr, which still is the un-multiplied 0.1 -- a
    # quirk of the published algorithm for multiplier > 1, restated as is; the reference's configs use multiplier 1)
    assert seq == [0.1, 0.2, 0.3, 0.1, 0.3], seq
    cfg3 = load_config(["train.optim.type=adam", "train.optim.lr=0.001", "train.optim.weight_decay=0.0001"])
    opt3, s3, w3 = build_optimizer(cfg3, net)
    assert isinstance(opt3, torch.optim.Adam) and s3 is None and w3 is None and opt3.param_groups[0]["betas"] == (0.9, 0.999)
    with pytest.raises(ValueError):
        GradualWarmupScheduler(opt, 0.5, 3)
    opt4, s4, w4 = build_optimizer(load_config([]), net)
    assert isinstance(opt4, FusedSGD) and w4 is None and s4.milestones == {20: 1}


def test_plan_export_import_round_trip_and_fingerprint():
    """tbn_backbone_plan_export / _import / _fingerprint on the host (no GPU): a blob moves every launch choice of a plan
    into another plan of the same problem (fingerprints and launch_info become equal), a modified choice changes the
    fingerprint, and blobs for another problem, truncated blobs and out-of-range choices are refused with the plan left
    untouched.  This is what `DataParallel` broadcasts from rank 0 so that every replica runs the same kernels."""
    import ctypes as C
    import struct
    from attention_based_tbn_amd._lib import lib
    L = lib()
    a, b, other = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.tbn_backbone_plan_create(3, 4, 96, 96, C.byref(a)) == 0
    assert L.tbn_backbone_plan_create(3, 4, 96, 96, C.byref(b)) == 0
    assert L.tbn_backbone_plan_create(3, 5, 96, 96, C.byref(other)) == 0
    n = L.tbn_backbone_plan_export_bytes(a)
    assert n == 4 * (8 + 26 * 44) and n == L.tbn_backbone_plan_export_bytes(b)        # 44 GEMMs per backbone
    buf = C.create_string_buffer(n)
    assert L.tbn_backbone_plan_export(a, buf, n) == 0
    assert L.tbn_backbone_plan_export(a, buf, n - 4) < 0 and b"too small" in L.tbn_last_error()
    fp0 = L.tbn_backbone_plan_fingerprint(a)
    assert fp0 != 0 and fp0 == L.tbn_backbone_plan_fingerprint(b) and fp0 != L.tbn_backbone_plan_fingerprint(other)
    ints = list(struct.unpack("%di" % (n // 4), buf.raw))
    assert ints[:8] == [0x54424E50, 1, 3, 4, 96, 96, 44, 26]
    # "tune" the blob by hand: the forward (training mode) and data-gradient choices of inception_4a_3x3 (a 3x3 / stride-1
    # layer, first member of a sibling pair): LDS-halo <2,1>, paired forward launch, split-K data gradient
    names, info = [], (C.c_int * 16)()
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    target = None
    for g in range(44):
        q = ints[8 + 26 * g: 8 + 26 * (g + 1)]
        assert len(q) == 26
    # find the GEMM whose training-mode forward matches launch_info of the layer, by changing one and reading it back
    for g in range(44):
        trial = list(ints)
        base = 8 + 26 * g
        trial[base + 8:base + 12] = [2, 1, 0, 1]            # training-mode forward: mt, nt, stages, variant = LDS-halo
        blob = struct.pack("%di" % len(trial), *trial)
        rc = L.tbn_backbone_plan_import(b, blob, len(blob))
        if rc != 0:                                          # the stem refuses a non-generic variant: plan untouched
            assert b"invalid launch choice" in L.tbn_last_error() and L.tbn_backbone_plan_fingerprint(b) == fp0
            continue
        assert L.tbn_backbone_launch_info(b, b"inception_4a_3x3", 1, info) == 0
        if list(info)[:4] == [1, 2, 1, 0]:
            target = g
        assert L.tbn_backbone_plan_import(b, buf, n) == 0 and L.tbn_backbone_plan_fingerprint(b) == fp0
    assert target is not None
    tuned = list(ints)
    base = 8 + 26 * target
    tuned[base + 8:base + 16] = [2, 1, 0, 1, 1, 0, 1, 2]     # forward (training): halo <2,1>, paired (variant 0, <1,2>)
    tuned[base + 16:base + 24] = [1, 2, 1, 3, 0, 1, 1, 1]    # data gradient: split-K tile <1,2>
    tuned[base + 24:base + 26] = [3, 2]                      # weight-gradient tile
    blob = struct.pack("%di" % len(tuned), *tuned)
    assert L.tbn_backbone_plan_import(b, blob, len(blob)) == 0
    fp1 = L.tbn_backbone_plan_fingerprint(b)
    assert fp1 != fp0
    assert L.tbn_backbone_launch_info(b, b"inception_4a_3x3", 1, info) == 0
    assert list(info) == [1, 2, 1, 0, 1, 0, 1, 2, 3, 1, 2, 1, 0, 1, 1, 1]
    assert L.tbn_backbone_launch_info(b, b"inception_4a_3x3", 0, info) == 0 and list(info)[0] == 0   # eval choices untouched
    # ... and on to a third plan through export: a -> equal to b
    out = C.create_string_buffer(n)
    assert L.tbn_backbone_plan_export(b, out, n) == 0 and out.raw == blob
    assert L.tbn_backbone_plan_import(a, out, n) == 0 and L.tbn_backbone_plan_fingerprint(a) == fp1
    # refusals leave the plan as it was
    assert L.tbn_backbone_plan_import(other, out, n) < 0 and b"this plan for" in L.tbn_last_error()
    assert L.tbn_backbone_plan_import(a, out, 16) < 0 and b"truncated" in L.tbn_last_error()
    bad = list(tuned)
    bad[0] = 7
    bb = struct.pack("%di" % len(bad), *bad)
    assert L.tbn_backbone_plan_import(a, bb, len(bb)) < 0 and b"not a plan blob" in L.tbn_last_error()
    # tile / variant / wgrad tile out of range; wgrad tiles the planner would swap for another (mt 4, nt 4 | 5, one of the two 0)
    for off, val in ((8, 3), (9, 5), (11, 4), (16, 0), (24, 9), (24, 4), (25, 4), (25, 5), (24, 0), (25, 0), (24, -1), (24, 6),
                     (24, 5)):
        bad = list(tuned)
        if (off, val) == (24, 5):                                       # 5 x 3 (5 x 2, mt 5 beside the tuned nt 2, is a tile)
            bad[base + 25] = 3
        bad[base + off] = val
        bb = struct.pack("%di" % len(bad), *bad)
        assert L.tbn_backbone_plan_import(a, bb, len(bb)) < 0 and b"invalid launch choice" in L.tbn_last_error(), (off, val)
        assert L.tbn_backbone_plan_fingerprint(a) == fp1
    for h in (a, b, other):
        L.tbn_backbone_plan_destroy(h)


def test_plan_cache_files_carry_one_modes_choices(tmp_path, monkeypatch):
    """TBN_PLAN_CACHE (opt-in): a process writes the choices it tuned for one (problem, mode); a later plan of the same
    problem adopts exactly that mode's fields and keeps the other mode's; no variable, a missing file, another library
    version or another problem: nothing is loaded.  Host only."""
    import ctypes as C
    import struct
    from attention_based_tbn_amd._lib import lib
    from attention_based_tbn_amd.core.models.bn_inception import _Plan
    a = _Plan(3, 4, 96, 96)
    assert a.load_cached(3, True) is False                      # variable not set
    monkeypatch.setenv("TBN_PLAN_CACHE", str(tmp_path / "plans"))
    assert a.load_cached(3, True) is False                      # no file yet
    ints = list(struct.unpack("%di" % (len(a.export_choices()) // 4), a.export_choices()))
    g = next(i for i in range(44) if ints[8 + 26 * i + 8 + 3] == 0 and i > 2)   # any non-stem GEMM
    base = 8 + 26 * g
    ints[base + 8:base + 12] = [2, 2, 2, 0]                     # training forward: <2,2>, 2 LDS stages
    ints[base:base + 4] = [1, 3, 1, 0]                          # eval forward: <1,3>, 1 stage
    a.import_choices(struct.pack("%di" % len(ints), *ints))
    fp_a = a.fingerprint()
    a.store_cached(3, True)
    files = os.listdir(tmp_path / "plans")
    assert len(files) == 1 and files[0] == "tbnplan_v%d_c3_f4_96x96_train.bin" % lib().tbn_version()
    b = _Plan(3, 4, 96, 96)
    fp_fresh = b.fingerprint()
    assert b.load_cached(3, False) is False                     # no eval file
    assert b.load_cached(3, True) is True
    got = list(struct.unpack("%di" % len(ints), b.export_choices()))
    assert got[base + 8:base + 12] == [2, 2, 2, 0]              # the training-mode choice came over ...
    assert got[base:base + 4] != [1, 3, 1, 0]                   # ... the eval-mode one did not (a training file)
    assert b.fingerprint() not in (fp_fresh, fp_a)
    a.store_cached(3, False)
    assert b.load_cached(3, False) is True and b.fingerprint() == fp_a
    assert _Plan(3, 5, 96, 96).load_cached(3, True) is False    # another problem: another file name


def test_isa_wait_scan_flags_a_wait_right_behind_its_load(tmp_path, capsys):
    """scripts/isa_wait_scan.py on a synthetic listing: a loop that waits vmcnt(0) two MFMAs behind a load is reported as
    tight, the same loop with the load issued a whole trip earlier (vmcnt(1)) is not"""
    import runpy, sys
    def listing(wait):
        body = ["_Z4demov:", ".LBB0_1:", "\tbuffer_load_dwordx4 v[0:3], v9, s[0:3], 0 offen"]
        body += ["\tv_mfma_f32_32x32x2_f32 v[16:31], v4, v5, v[16:31]"] * 2
        body += ["\t" + wait, "\tds_write_b128 v8, v[0:3]"]
        body += ["\tv_mfma_f32_32x32x2_f32 v[16:31], v4, v5, v[16:31]"] * 14
        body += ["\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm"]
        return "\n".join(body) + "\n"
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "isa_wait_scan.py")
    out = []
    for name, wait in (("tight.s", "s_waitcnt vmcnt(0)"), ("far.s", "s_waitcnt vmcnt(1)")):
        f = tmp_path / name
        f.write_text(listing(wait))
        old = sys.argv
        sys.argv = [script, str(f), "demo"]
        try:
            runpy.run_path(script, run_name="__main__")
        finally:
            sys.argv = old
        out.append(capsys.readouterr().out)
    assert "tightest wait   2 MFMAs" in out[0] and "1 of 1 waits closer than 12" in out[0], out[0]
    assert "tightest wait  18 MFMAs" in out[1] and "0 of 1 waits closer than 12" in out[1], out[1]


def test_bench_roofline_is_a_median_over_post_loop_samples():
    """bench.py host logic (no GPU): `roofline` comes from the instrumented steps run AFTER the timed loop -- dominant kernel
    by summed time, achieved / conv-stage figures as medians with min / max beside them, head Linear GEMMs kept apart"""
    import bench

    def sample(scale):
        return [{"kernel": "conv_wgrad_kernel<2, 2, 0>", "launches": 36, "ms": 3.6 * scale, "flops": 36 * 13.0e9, "alg_bytes": 36 * 50e6},
                {"kernel": "conv_halo_kernel<1, 1, 1>", "launches": 20, "ms": 1.5 * scale, "flops": 20 * 8.0e9, "alg_bytes": 20 * 30e6},
                {"kernel": "linear: conv_sk4_kernel<1, 1, 0>", "launches": 6, "ms": 0.1, "flops": 6e9, "alg_bytes": 1e6}]
    r = bench.roofline_object([sample(1.00), sample(1.10), sample(0.95)], 1, 0.68)
    assert r["kernel"] == "conv_wgrad_kernel<2, 2, 0>" and r["samples"] == 3 and r["launches"] == 36
    tf = [36 * 13.0e9 / (3.6e-3 * s) / 1e12 for s in (1.00, 1.10, 0.95)]
    dom = r["dominant"]               # round 6: the dominant kernel's own figure sits under `dominant` ...
    assert dom["kernel"] == r["kernel"] and abs(dom["achieved"] - sorted(tf)[1]) < 0.01 and dom["launches"] == 36
    assert abs(dom["frac_min"] - min(tf) / bench.PEAK_FP32_MFMA_TFLOPS) < 1e-3 and abs(dom["frac_max"] - max(tf) / bench.PEAK_FP32_MFMA_TFLOPS) < 1e-3
    conv = [(36 * 13.0e9 + 20 * 8.0e9) / (5.1e-3 * s) / 1e12 for s in (1.00, 1.10, 0.95)]
    # ... and the line LEADS with the conv stage: of the timed schedule when the timeline steps ran, else one stream at a time
    assert r["frac_is"].startswith("all_conv_gemm") and abs(r["achieved"] - sorted(conv)[1]) < 0.01 and r["conv_stage_timed_schedule"] is None
    sched = {"achieved": 111.0, "frac": round(111.0 / bench.PEAK_FP32_MFMA_TFLOPS, 4), "steps": 4}
    r3 = bench.roofline_object([sample(1.00)], 1, 0.68, sched)
    assert r3["frac_is"] == "conv_stage_timed_schedule" and r3["achieved"] == 111.0 and r3["frac"] == sched["frac"]
    assert r3["conv_stage_timed_schedule"] is sched and abs(r3["dominant"]["achieved"] - tf[0]) < 0.01
    assert abs(r["all_conv_gemm"]["achieved"] - sorted(conv)[1]) < 0.01 and r["all_conv_gemm"]["frac_min"] < r["all_conv_gemm"]["frac"] < r["all_conv_gemm"]["frac_max"]
    assert r["head_linear_gemm"]["launches"] == 6 and r["end_to_end_frac"] == 0.68 and r["kernel_families"]["conv_halo_kernel"] == 20
    assert bench.roofline_object([], 1, 0.5) is None
    # the diagnostic in-loop mode (--profile-every): ONE aggregate over several steps, launches reported per step
    agg = [dict(e, launches=e["launches"] * 4, ms=e["ms"] * 4, flops=e["flops"] * 4, alg_bytes=e["alg_bytes"] * 4) for e in sample(1.0)]
    r2 = bench.roofline_object([agg], 4, 0.5)
    assert r2["launches"] == 36 and abs(r2["all_conv_gemm"]["ms_per_profiled_step"] - 5.1) < 0.01
    cpu = bench.host_cpu()
    assert cpu["hardware_threads"] >= 1 and (cpu["physical_cores"] is None or cpu["physical_cores"] <= cpu["hardware_threads"])


def test_bench_pins_the_committed_launch_plans(tmp_path, monkeypatch):
    """bench.py host logic (no GPU): the committed plans are written into a fresh plan-cache directory that TBN_PLAN_CACHE
    points at, under the names core/models/bn_inception.py looks for with THIS library version, config 4's three backbones
    among them; a TBN_PLAN_CACHE of the caller's own wins"""
    import shutil
    import bench
    from attention_based_tbn_amd._lib import lib
    monkeypatch.delenv("TBN_PLAN_CACHE", raising=False)
    with open(bench.PINNED_PLANS) as f:
        plans = json.load(f)["plans"]
    d, names = bench.pin_plans()
    try:
        assert os.environ["TBN_PLAN_CACHE"] == d and names == set(plans) == set(os.listdir(d))
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                assert f.read() == bytes.fromhex(plans[n]), n
    finally:
        shutil.rmtree(d)
    shapes = set()
    for n in names:
        m = re.fullmatch(r"tbnplan_v(\d+)_(c\d+_f\d+_\d+x\d+_(?:train|eval))\.bin", n)
        assert m and int(m.group(1)) == lib().tbn_version(), n
        shapes.add(m.group(2))
    assert {"c3_f96_224x224_train", "c10_f96_224x224_train", "c1_f96_256x256_train"} <= shapes, shapes
    monkeypatch.setenv("TBN_PLAN_CACHE", str(tmp_path))
    assert bench.pin_plans() is None and os.environ["TBN_PLAN_CACHE"] == str(tmp_path)


def test_bench_dump_outputs_are_float32_and_sampled_at_fixed_positions(tmp_path, monkeypatch):
    """bench.py --dump-outputs host logic (no GPU): one float32 .npy per returned array; parameters, gradients and BN
    statistics beyond DUMP_SAMPLE elements are a sample taken at the same positions in every run, within 64 MB"""
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.BatchNorm1d(30), torch.nn.Linear(30, 5))
    model[2].weight.requires_grad_(False)
    out = model(torch.randn(8, 40))
    loss = out.square().mean()
    loss.backward()
    out = {"verb": out[:, :3], "noun": out[:, 3:]}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss.detach(), out, model, True, True)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["buffers.npy", "grads.npy", "loss.npy", "out_noun.npy", "out_verb.npy", "params.npy"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float32 for a in got.values())
    for k, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / (k + ".npy"))), k
    assert got["out_verb"].shape == (8, 3) and got["loss"][0] == np.float32(loss.item())
    assert got["buffers"].shape == (60,)                        # running mean + var: below the sample size, whole
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert got["params"].shape == got["grads"].shape == (1000,) and sum(p.numel() for p in trainable) > 1000
    flat = torch.cat([p.detach().reshape(-1) for p in trainable]).numpy()
    gflat = torch.cat([p.grad.reshape(-1) for p in trainable]).numpy()
    idx = torch.randint(flat.size, (1000,), generator=torch.Generator().manual_seed(0)).sort().values.numpy()
    assert np.array_equal(got["params"], flat[idx]) and np.array_equal(got["grads"], gflat[idx])   # same positions in both
    bench.dump_outputs(str(tmp_path / "eval"), None, out, model, False, False)
    assert sorted(os.listdir(tmp_path / "eval")) == ["out_noun.npy", "out_verb.npy"]


def test_pmc_traffic_prices_requests_with_the_calibration(tmp_path):
    """scripts/pmc_traffic.py --raw on synthetic rocprofv3 counter CSVs: bytes per request come from the calibration
    launches of known byte counts (128 here, as on the MI355X), the priming / warm-up steps are cut at the SKIP-th
    optimiser dispatch, a calibration entry that matched a no-read kernel falls back"""
    import csv as _csv
    import subprocess
    hdr = ["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"]

    def write(path, rows):
        with open(path, "w", newline="") as f:
            w = _csv.writer(f)
            w.writerow(hdr)
            w.writerows(rows)

    def rd(d, k, req, r32=0, bub=0):
        return [[d, k, "TCC_EA0_RDREQ_sum", req], [d, k, "TCC_EA0_RDREQ_32B_sum", r32], [d, k, "TCC_BUBBLE_sum", bub]]
    cal = rd(1, "void at::native::vectorized_elementwise_kernel<4, FillFunctor>", 22) + \
        rd(2, "void conv_wgrad_kernel<2, 2, 2>(WgradP)", 8_000_000) + rd(3, "bn_apply_kernel(float const*)", 6_000_000)
    write(tmp_path / "cal.csv", cal)
    expect = {"wide_copy": {"kernel_contains": "elementwise", "read_bytes_per_launch": 1 << 30, "launches": 1},
              "wgrad_pointwise_64x64": {"kernel_contains": "conv_wgrad_kernel", "read_bytes_per_launch": 8_000_000 * 128, "launches": 1},
              "bn_apply": {"kernel_contains": "bn_apply_kernel", "read_bytes_per_launch": 6_000_000 * 128, "launches": 1}}
    (tmp_path / "expect.json").write_text(json.dumps(expect))
    reads, writes = [], []
    d = 0
    for step in range(3):                      # step 0 is cut off (SKIP = 1)
        for k, req, wkib in (("void conv_wgrad_kernel<2, 2, 0>(WgradP)", 670_000, 12_000.0), ("bn_apply_multi_kernel(BnFwdBatch)", 250_000, 31_000.0),
                             ("opt_sgd_kernel(OptTab, float)", 1000, 10.0)):
            d += 1
            reads += rd(d, k, req * (10 if step == 0 else 1))
            writes.append([d, k, "WRITE_SIZE", wkib])
    write(tmp_path / "rd.csv", reads)
    write(tmp_path / "wr.csv", writes)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pmc_traffic.py"), "--raw", str(tmp_path / "rd.csv"),
                        str(tmp_path / "wr.csv"), str(tmp_path / "out.json"), "1", "unit test", str(tmp_path / "cal.csv"),
                        str(tmp_path / "expect.json")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    doc = json.loads((tmp_path / "out.json").read_text())
    assert doc["calibration"]["wgrad_pointwise_64x64"]["bytes_per_request_of_the_64B_class"] == 128.0
    k = doc["kernels"]["conv_wgrad_kernel<2, 2, 0>"]
    assert k["launches"] == 2 and k["hbm_read_bytes_per_launch"] == 670_000 * 128 and k["hbm_write_bytes_per_launch"] == 12_000 * 1024
    b = doc["kernels"]["bn_apply_multi_kernel"]
    assert b["bytes_per_request_used"] == 128.0 and b["hbm_read_bytes_per_launch"] == 250_000 * 128      # wide entry invalid -> bn_apply's
    assert len(doc["source_sha16"]) == 16
