"""GPU: the real TBN model under the data-parallel wrapper with 2 ranks (both on cuda:0, gloo backend --
RCCL needs one GPU per rank, which a 1-GPU box cannot give): every rank's averaged gradient must equal the
mean of the two ranks' local gradients, and replicas must start identical after the wrap-time broadcast."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from attention_based_tbn_amd.config import load_config, get_modality
from attention_based_tbn_amd.core.models import build_model, DataParallel
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=2)
rank = dist.get_rank()
dev = torch.device("cuda:0")
cfg = load_config(["data.flow.enable=False", "data.audio.audio_length=1.279", "model.fusion_dropout=0",
                   "model.attention.attn_dropout=0.0"])
modality = get_modality(cfg)
torch.manual_seed(10 + rank)                              # replicas differ until the broadcast
model, crit, _ = build_model(cfg, modality, dev)
assert isinstance(model, DataParallel) and model.world_size == 2
sd = model.module.state_dict()
ref = [torch.empty_like(sd["classifier.verb.weight"]) for _ in range(2)]
dist.all_gather(ref, sd["classifier.verb.weight"])
assert torch.equal(ref[0], ref[1])                       # broadcast made the replicas identical
g = torch.Generator().manual_seed(100 + rank)            # each rank its own shard of clips
B, n = 2, 3
inp = {"RGB": (torch.rand(B, n, 3, 64, 64, generator=g) - 0.45).to(dev),
       "Audio": (torch.randn(B, n, 1, 128, 256, generator=g) * 3 - 6).to(dev)}
tgt = {"class": {"verb": torch.randint(0, 125, (B,), generator=g).to(dev), "noun": torch.randint(0, 352, (B,), generator=g).to(dev)}}
model.train()
def run(m):
    for p in m.parameters(): p.grad = None
    st = {k: v.clone() for k, v in model.module.state_dict().items()}
    out = m(inp); loss, _ = m.get_loss(crit, tgt, out, 12); loss["total"].backward()
    torch.cuda.synchronize()
    model.module.load_state_dict(st)                      # undo the BN running-stat update
    return {k: p.grad.clone() for k, p in model.module.named_parameters() if p.grad is not None}
with model.no_sync():
    local = run(model.module)                             # gradient hooks off: this rank's own gradients
synced = run(model)                                       # hooks: backbone all-reduces inside backward, small tensors at its end
for k, gl in local.items():
    parts = [torch.empty_like(gl) for _ in range(2)]
    dist.all_gather(parts, gl)
    want = (parts[0] + parts[1]) / 2
    err = float((synced[k] - want).abs().max() / (want.abs().max() + 1e-20))
    assert err < 1e-5, (k, err)
assert len(local) >= 12 and model._fired == set() and model._pending == []
# every replica runs the kernels rank 0 tuned (tbn_backbone_plan_export / _import through DataParallel's PlanSync): the
# plans' fingerprints are equal across the ranks, although each rank would have tuned from its own noisy timings
fps = {m: getattr(model.module, "Base_" + m).plan_fingerprints() for m in modality}
both = [None, None]
dist.all_gather_object(both, fps)
assert both[0] == both[1] and all(len(v) == 1 for v in fps.values()), both
assert all(getattr(model.module, "Base_" + m).plan_sync is not None for m in modality)

# ---- audio dropout (reference model.py:215-222: a per-replica host draw): the ranks exchange the draw after forward on
# a side stream; all kept / one dropped / both dropped must give the mean of the local gradients (zeros where dropped),
# and `None` for the audio branch when nobody kept it
import numpy as np
cfg2 = load_config(["data.flow.enable=False", "data.audio.audio_length=1.279", "model.fusion_dropout=0",
                    "model.attention.enable=False", "data.audio.dropout=0.5"])
torch.manual_seed(3)
model2, crit2, _ = build_model(cfg2, get_modality(cfg2), dev)
model2.train()
assert model2.module.maybe_unused_parameter_prefixes()
def seed_for(drop):                                      # a NumPy seed whose first uniform() is > 0.5 (drop) or not
    s = 0
    while (np.random.RandomState(s).uniform() > 0.5) != drop: s += 1
    return s
def run2(m, drop):
    for p in m.parameters(): p.grad = None
    st = {k: v.clone() for k, v in model2.module.state_dict().items()}
    np.random.seed(seed_for(drop))
    out = m(inp); loss, _ = m.get_loss(crit2, tgt, out, 12); loss["total"].backward()
    torch.cuda.synchronize()
    model2.module.load_state_dict(st)
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in model2.module.named_parameters() if p.requires_grad}
named2 = dict(model2.module.named_parameters())
for drops in ((False, False), (False, True), (True, True), (True, False)):
    with model2.no_sync():
        local2 = run2(model2.module, drops[rank])
    synced2 = run2(model2, drops[rank])
    assert model2._presence is None and model2._pending == []
    for k, gs in synced2.items():
        gl = local2[k] if local2[k] is not None else torch.zeros_like(named2[k])
        parts = [torch.empty_like(gl) for _ in range(2)]
        dist.all_gather(parts, gl)
        if k.startswith("Base_Audio.") and all(drops):
            assert gs is None, (drops, k)                 # nobody kept the branch: the optimiser must see None
            continue
        want = (parts[0] + parts[1]) / 2
        assert gs is not None, (drops, k)
        err = float((gs - want).abs().max() / (want.abs().max() + 1e-20))
        assert err < 1e-5, (drops, k, err)
print("DP_GPU_OK", rank, len(local))
'''


def test_dataparallel_real_model_two_ranks_on_one_gpu(tmp_path):
    script = tmp_path / "dp_gpu_worker.py"
    script.write_text(_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"DP_GPU_OK {r}" in o, "\n".join(f"---- rank {i}: {x[-2500:]}" for i, x in enumerate(outs))


@pytest.mark.parametrize("launcher", ["torch.distributed.run", "plain python"])
def test_bench_n2_control_flow_rehearsal(launcher):
    """`bench.py --gpus 2` exactly as the driver launches it for N > 1 (torch.distributed.run, one rank per process) AND as
    the driver launches its 1-GPU run (plain `python bench.py --gpus 2`, no RANK / WORLD_SIZE in the environment: bench.py
    then starts the ranks itself as a child process and relays the JSON line and the exit code -- round-5 verdict item 2a),
    with the two ranks sharing the one card over gloo (TBN_BENCH_BACKEND=gloo: RCCL needs a GPU per rank): the barrier /
    max-over-ranks timing / DataParallel path (gradient buckets included) must run and stdout must be exactly one JSON line
    from rank 0.  --full: the line then also carries the roofline, bucket count and plan check asserted here."""
    import json
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(TBN_BENCH_BACKEND="gloo", OMP_NUM_THREADS="2")
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch-per-gpu", "2", "--full"]
    if launcher == "plain python":
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port)] + tail
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["config"]["global_batch"] == 4 and d["value"] > 0
    assert d["scaling"] == "weak" and "cpu_baseline" not in d and d["roofline"]["frac"] > 0
    assert d["multi_gpu"]["dist_world_size"] == 2 and d["multi_gpu"]["plans_equal_across_ranks"] is True
    assert d["multi_gpu"]["gradient_buckets_per_step"] == 6, d["multi_gpu"]      # two per backbone, from inside its backward
    if launcher == "plain python":
        assert "launching 2 ranks" in r.stderr
    # a failing child must fail the parent: an argument the ranks reject
    if launcher == "plain python":
        bad = subprocess.run([sys.executable] + tail + ["--config", "3", "--audio-2p1s", "--stft-inputs"], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and not [l for l in bad.stdout.splitlines() if l.strip().startswith("{")]


_RCCL_WORKER = r'''
import os, sys, math, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from attention_based_tbn_amd.config import load_config, get_modality
from attention_based_tbn_amd.core.models import DataParallel
from attention_based_tbn_amd.core.models.model import TBNModel
from attention_based_tbn_amd.core.utils import FusedSGD
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]), device_id=dev)
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
cfg = load_config(["model.attention.enable=False", "data.audio.audio_length=1.279", "data.sampling=async",
                   "model.fusion_dropout=0"])
modality = get_modality(cfg)
torch.manual_seed(5)
model = TBNModel(cfg, modality, dev).to(dev)
crit = {"crossentropy": torch.nn.CrossEntropyLoss()}
plain = DataParallel(model)                                # the default wrap of a lone rank: a pass-through
assert not plain.active and plain._hooks == []
dp = DataParallel(model, force_sync=True)                  # hooks + collectives although the group has one rank
assert dp.active and dp.world_size == 1 and len(dp._hooks) > 0
# the plan hand-over of a real multi-rank job (rank 0 tunes, tbn_backbone_plan_export -> broadcast -> _import) on RCCL's
# tensor path: a one-rank group broadcasts to itself, through the same device-tensor round trip
from attention_based_tbn_amd.core.models.dataparallel import PlanSync
for mod in model.modules():
    if hasattr(mod, "plan_sync"):
        assert mod.plan_sync is None                      # not installed for a lone rank by default
        mod.plan_sync = PlanSync(None)
dp.time_sync = True
calls = []
_ar = dist.all_reduce
def counting_all_reduce(t, *a, **k):
    calls.append(t.numel())
    return _ar(t, *a, **k)
dist.all_reduce = counting_all_reduce
g = torch.Generator().manual_seed(11)
B, n = 2, 3
inp = {"RGB": (torch.rand(B, n, 3, 64, 64, generator=g) - 0.45).to(dev),
       "Flow": (torch.rand(B, n, 10, 64, 64, generator=g) - 0.5).to(dev),
       "Audio": (torch.randn(B, n, 1, 128, 256, generator=g) * 3 - 6).to(dev)}
tgt = {"class": {"verb": torch.randint(0, 125, (B,), generator=g).to(dev), "noun": torch.randint(0, 352, (B,), generator=g).to(dev)}}
model.train()
params = [p for p in model.parameters() if p.requires_grad]
opt = FusedSGD(params, lr=0.01, momentum=0.9, weight_decay=0)
def run(m):
    for p in model.parameters(): p.grad = None
    st = {k: v.clone() for k, v in model.state_dict().items()}
    out = m(inp); loss, _ = m.get_loss(crit, tgt, out, 0); loss["total"].backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return st, grads, float(loss["total"])
for step in range(2):
    with dp.no_sync():
        st, local, l0 = run(model)                         # hooks off: the un-wrapped model's own gradients
    model.load_state_dict(st)                              # undo the BN running-statistics update
    n0 = len(calls)
    _, synced, l1 = run(dp)                                # hook -> all_reduce(async_op=True) -> queue_callback -> work.wait()
    # the three flat backbone gradients (~41 MB each) and the fusion Linear's weight (3072 x 512) from their hooks, as
    # soon as autograd has accumulated them, + ONE packed collective for every small tensor at the end of backward
    step_calls = calls[n0:]
    # round 6: a backbone's flat gradient travels in THREE collectives -- the weights of inception_5a..5b and of 4a..4e from
    # inside its backward as the engine reports them final (tbn_backbone_grads.bucket_cb), the remaining prefix (stem,
    # 3a..3c: ~10 %) at the end of backward behind every bucket: fusion weight + 3 x 2 buckets + 3 prefixes + packed = 11
    assert len(step_calls) == 11, step_calls
    assert model.fusion.fusion_layer[0].weight.numel() in step_calls, step_calls
    assert step_calls[-1] == min(step_calls), step_calls       # the packed small tensors go last
    log = list(dp.bucket_log)
    assert len(log) == 6, log
    for m in modality:
        nfl = getattr(model, "Base_" + m).flat_weight.numel()
        mine = [e for e in log if e[0] == nfl]          # the three stems differ (3 / 10 / 1 input channels): so do the sizes
        assert len(mine) == 2, (m, log)
        (n1, lo1, hi1), (n2, lo2, hi2) = mine
        assert hi1 == nfl and hi2 == lo1 and 0 < lo2 < lo1, (m, mine)          # top-down suffixes of the flat tensor
        assert 0.40 < (hi1 - lo1) / nfl < 0.47 and 0.43 < (hi2 - lo2) / nfl < 0.50 and lo2 / nfl < 0.12, (m, mine)
        # the prefix (stem, 3a..3c; differs per modality) goes at the END of backward, behind every bucket of every backbone and
        # in front of the packed buffer: issued from the gradient hook it would hold up the later backbones' buckets
        assert lo2 in step_calls[-4:-1], (m, lo2, step_calls)
    b1, b2 = log[0][2] - log[0][1], log[1][2] - log[1][1]            # the same two bucket sizes for every backbone (same blocks)
    assert step_calls[:7] == [model.fusion.fusion_layer[0].weight.numel(), b1, b2, b1, b2, b1, b2], step_calls
    dp.bucket_log.clear()
    assert l0 == l1, (l0, l1)
    assert set(local) == set(synced) and len(local) == 18, sorted(local)   # 3 x (flat weight, flat bias, first-BN affine) + heads
    for k in local:
        assert torch.equal(local[k], synced[k]), (step, k, float((local[k] - synced[k]).abs().max()))
    assert dp._pending == [] and dp._fired == set() and not dp._callback_queued and dp._forwards_pending == 0
    opt.step(clip_grad=20)                                 # the second step runs on updated weights
torch.cuda.synchronize()
fps = {m: getattr(model, "Base_" + m).plan_fingerprints() for m in modality}
assert all(len(v) == 1 and all(len(f) == 16 for f in v.values()) for v in fps.values()), fps
ms = dp.exposed_sync_ms()
assert ms is not None and math.isfinite(ms) and ms >= 0.0, ms
dist.destroy_process_group()
print("RCCL_W1_OK exposed_allreduce_ms=%.3f" % ms)
'''


def test_gradient_sync_on_real_rccl_world_size_1(tmp_path):
    """ProcessGroupNCCL (= RCCL) under the gradient-sync path, on the one GPU a development box has: `force_sync`
    registers the hooks at world size 1, the child is started by torch.distributed.run (fresh process, rendezvous on
    127.0.0.1) and runs two training steps of the real three-modality model through hook -> all_reduce(async_op=True)
    -> queue_callback -> work.wait() (a STREAM wait on RCCL; gloo, which every other rehearsal uses, blocks the host).
    Gradients must equal the un-wrapped model's bit for bit (AVG over one rank, packing and unpacking are exact) and the
    exposed all-reduce time must be a finite number.  Replaces reference core/models/model_builder.py:73-75."""
    script = tmp_path / "rccl_w1_worker.py"
    script.write_text(_RCCL_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(port), str(script), ROOT]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_W1_OK" in r.stdout, (r.stdout[-1500:] + "\n----\n" + r.stderr[-3000:])
