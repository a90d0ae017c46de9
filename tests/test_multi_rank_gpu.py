"""GPU: the epoch-loop layer as two ranks of one job -- sharded `ClipLoader` batches against the world-1 private pass,
`DeviceMetric`'s merge, the loss scale of `TrainStep` under `DataParallel`, and `run_trainer` / `run_tester` end to end.
As in tests/test_dp_gpu.py both ranks are fresh child processes on cuda:0 over gloo (RCCL needs a GPU per rank); the
group's timeout is a minute, the parent kills both children as soon as one fails, and nothing is retried."""
import json
import os
import socket
import subprocess
import sys
import threading

import pytest

from tests import clip_loader_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HEAD = r'''
import datetime, json, os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
ARGS = json.load(open(sys.argv[2]))
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=2, timeout=datetime.timedelta(seconds=60))
rank, dev = dist.get_rank(), torch.device("cuda", 0)
def everyone(x):
    got = [None, None]
    dist.all_gather_object(got, x)
    return got
'''


def _run_ranks(tmp_path, body, args, token, timeout=240):
    """two children run `_HEAD + body`; the first one to fail takes the other down -> their outputs"""
    script, argfile = tmp_path / "worker.py", tmp_path / "args.json"
    script.write_text(_HEAD + body)
    argfile.write_text(json.dumps(args))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs, logs = [], []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", TBN_PLAN_CACHE=str(tmp_path / "plans"))
        logs.append(open(tmp_path / "rank{}.log".format(r), "w+"))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT, str(argfile)], env=env, stdout=logs[r],
                                      stderr=subprocess.STDOUT, text=True))

    def watch(i):
        try:
            if procs[i].wait(timeout=timeout) == 0:
                return
        except subprocess.TimeoutExpired:
            pass
        for p in procs:
            if p.poll() is None:
                p.kill()

    watchers = [threading.Thread(target=watch, args=(i,)) for i in range(2)]
    for t in watchers:
        t.start()
    for t in watchers:
        t.join()
    outs = []
    for p, f in zip(procs, logs):
        p.wait()
        f.seek(0)
        outs.append(f.read())
        f.close()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "{} {}".format(token, r) in o, \
            "\n".join("---- rank {} (exit {}): {}".format(i, q.returncode, x[-6000:]) for i, (q, x) in enumerate(zip(procs, outs)))
    print("\n".join(line for line in outs[0].splitlines() if line.startswith(("metric ", "gradient rule "))))
    return outs


_TWIN = r'''
from attention_based_tbn_amd.config import load_config
from attention_based_tbn_amd.core.dataset import dataset as D
from attention_based_tbn_amd.core.utils import ClipLoader
from tests import clip_loader_util as U
MODALITY = ["RGB", "Flow", "Audio"]
decoded = []
real = D.decode_jpegs
D.decode_jpegs = lambda blobs, **kw: (decoded.append(len(blobs)), real(blobs, **kw))[1]
FILES = 2 + 2 * 2 * 2            # per clip: num_segments RGB frames + num_segments * win_length * (x, y) flow frames

def cut(x, lo, hi, n):
    if isinstance(x, torch.Tensor):
        assert x.shape[0] == n
        return x[lo:hi]
    if isinstance(x, dict):
        return type(x)((k, cut(v, lo, hi, n)) for k, v in x.items())
    assert isinstance(x, list) and len(x) == n
    return x[lo:hi]

def same(a, b, path):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.device == b.device, path
        assert a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert type(a) is type(b) and list(a.keys()) == list(b.keys()), path
        for k in a:
            same(a[k], b[k], path + "." + str(k))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (path, i))
    else:
        assert a == b, path

cases = 0
for mode, extra in (("train", ["data.sampling=async", "model.attention.use_prior=True", "model.attention.prior_type=loud"]),
                    ("val", ["data.sampling=sync", "model.attention.enable=False"])):
    cfg = load_config(ARGS["overrides"] + extra)
    ds = U.make_dataset(cfg, MODALITY, mode, device=dev)
    for B in (2, 3):
        torch.manual_seed(40 + B)
        del decoded[:]
        twin = list(ClipLoader(ds, B, shuffle=(mode == "train"), prefetch=0, rng="private"))     # the world-1 pass, on this rank
        assert sum(decoded) == 3 * FILES
        sizes = [len(t[0]["vid_id"]) for t in twin]
        assert sizes == ([2, 1] if B == 2 else [3])
        kept = [i for i, n in enumerate(sizes) if not (mode == "train" and n < 2)]     # the train batch of one clip is dropped
        for prefetch in (0, 2):
            torch.manual_seed(40 + B if rank == 0 else 7000 + rank)      # rank 0's generator alone decides the pass
            np.random.seed(rank)
            state = np.random.get_state()[1].copy()
            loader = ClipLoader(ds, B, shuffle=(mode == "train"), prefetch=prefetch, shard=(rank, 2))
            assert len(loader) == len(kept)
            del decoded[:]
            seen, clips = [], 0
            for batch in loader:
                n_r, n, W = loader.share
                no = kept[loader.batch_no]
                lo, hi = rank * n // 2, (rank + 1) * n // 2
                assert (n_r, n, W) == (hi - lo, sizes[no], 2) and n_r > 0
                assert len(batch) == len(twin[no]) == (2 if mode == "train" else 3)
                same(batch, tuple(cut(part, lo, hi, n) for part in twin[no]), "%s B=%d prefetch=%d batch %d" % (mode, B, prefetch, no))
                seen.append(no)
                clips += n_r
            loader.close()
            # exactly the global batches this rank has a share of, in order; an empty share is not yielded
            assert seen == [no for no in kept if (rank + 1) * sizes[no] // 2 > rank * sizes[no] // 2], seen
            # a foreign clip's files are never decoded
            assert sum(decoded) == clips * FILES, (decoded, clips)
            assert np.array_equal(np.random.get_state()[1], state)
            both = everyone((seen, clips))
            assert both[0][1] + both[1][1] == sum(sizes[no] for no in kept)
            cases += 1
assert cases == 8
print("TWIN_OK", rank)
'''


def test_sharded_batches_concatenate_to_the_world_1_pass(tmp_path):
    """three clips, B in {2, 3}, W = 2: the unequal split 1 + 2, the empty share in val mode, the dropped batch in train
    mode; train with shuffle and val, prefetch 0 and 2"""
    _run_ranks(tmp_path, _TWIN, {"overrides": U.write_dataset(tmp_path / "data")}, "TWIN_OK")


_METRIC = r'''
from attention_based_tbn_amd.config import load_config
from attention_based_tbn_amd.core.utils import DeviceMetric
cfg = load_config(["model.attention.enable=False"])
g = torch.Generator().manual_seed(21)
N = 5
scores = {"verb": torch.randn(N, 125, generator=g), "noun": torch.randn(N, 352, generator=g)}
target = {"verb": torch.randint(0, 125, (N,), generator=g), "noun": torch.randint(0, 352, (N,), generator=g)}
for i in (0, 2, 3):                       # some hits, so that the accuracies are not all zero
    scores["verb"][i, target["verb"][i]] += 9.0
for i in (0, 3, 4):
    scores["noun"][i, target["noun"][i]] += 9.0
keys = ["verb", "noun", "all_class", "total"]
# global batch 0 = clips 0..3 (shares 2 + 2), global batch 1 = clip 4 (shares 0 + 1): rank 0 holds 2 clips, rank 1 holds 3
batches = [(0, 4), (4, 5)]
local = torch.rand(2, 2, 4, generator=g) * 3 + 0.1        # [rank][batch][key]: each rank's own float32 loss terms

def feed(metric, lo, hi, losses, **kw):
    out = {k: scores[k][lo:hi].to(dev) for k in ("verb", "noun")}
    tgt = {"class": {k: target[k][lo:hi].to(dev) for k in ("verb", "noun")}}
    metric.set_metrics(out, tgt, hi - lo, {k: losses[j].to(dev) for j, k in enumerate(keys)}, **kw)

single = DeviceMetric(cfg, 2, dev)                        # one process fed the whole batches
for b, (lo, hi) in enumerate(batches):
    feed(single, lo, hi, local[0, b])
_, want_acc, want_conf = single.get_metrics()

merged = DeviceMetric(cfg, 2, dev, process_group=dist.group.WORLD)
for b, (lo, hi) in enumerate(batches):
    n = hi - lo
    a, z = lo + rank * n // 2, lo + (rank + 1) * n // 2
    if z > a:
        feed(merged, a, z, local[rank, b], share=(z - a, n, 2), row=b)
assert len(merged._pending) == (1 if rank == 0 else 2)
assert merged.running("total") == sum(float(local[rank, b, 3]) for b in range(2) if not (rank == 0 and b == 1))   # local
loss, acc, conf = merged.get_metrics()
assert acc == want_acc and any(v > 0 for v in acc["verb"]) and any(v > 0 for v in acc["all_class"]), (acc, want_acc)
for k in ("verb", "noun"):
    assert torch.equal(conf[k], want_conf[k]) and float(conf[k].sum()) == N
# sum_r (n_r / n) loss_r per batch, summed over the batches and divided by their number: two products and two additions
# of float32 values per key; 4 ulp of the float32 value bounds any evaluation order of them, half a unit of the fifth
# decimal is get_metrics' own rounding
for j, k in enumerate(keys):
    want = (0.5 * float(local[0, 0, j]) + 0.5 * float(local[1, 0, j]) + 1.0 * float(local[1, 1, j])) / 2
    bound = 0.5e-5 + 4 * float(np.spacing(np.float32(want)))
    print("metric", k, loss[k], want, abs(loss[k] - want), bound)
    assert abs(loss[k] - want) <= bound, (k, loss[k], want)
both = everyone((loss, acc, {k: v.cpu().tolist() for k, v in conf.items()}))
assert both[0] == both[1]
# a share without a group, and a group without a share, are refused
try:
    feed(single, 0, 2, local[0, 0], share=(2, 4, 2)); raise SystemExit("no error")
except ValueError:
    pass
try:
    feed(merged, 0, 2, local[0, 0]); raise SystemExit("no error")
except ValueError:
    pass
print("METRIC_OK", rank)
'''


def test_device_metric_merges_the_ranks_shares(tmp_path):
    _run_ranks(tmp_path, _METRIC, {}, "METRIC_OK")


_GRAD = r'''
from attention_based_tbn_amd.config import load_config, get_modality
from attention_based_tbn_amd.core.models import build_model, DataParallel
from attention_based_tbn_amd.core.models.contrast_loss import ContrastLoss
from attention_based_tbn_amd.core.tools.train import local_plans
from attention_based_tbn_amd.core.utils import TrainStep
cfg = load_config(["data.flow.enable=False", "data.audio.audio_length=1.279", "model.fusion_dropout=0",
                   "model.attention.attn_dropout=0.0", "model.attention.use_prior=True", "model.attention.use_entropy=True",
                   "model.attention.use_contrast=True", "model.attention.entropy_thresh=0.0"])
modality = get_modality(cfg)
torch.manual_seed(10 + rank)
model, crit, _ = build_model(cfg, modality, dev)
assert isinstance(model, DataParallel) and model.world_size == 2
bare, att, EPOCH, W = model.module, cfg.model.attention, 12, 2
n_seg = 3

def make(B, seed):
    g = torch.Generator().manual_seed(seed)
    inp = {"RGB": (torch.rand(B, n_seg, 3, 64, 64, generator=g) - 0.45).to(dev),
           "Audio": (torch.randn(B, n_seg, 1, 128, 256, generator=g) * 3 - 6).to(dev)}
    tgt = {"class": {"verb": torch.randint(0, 125, (B,), generator=g).to(dev),
                     "noun": torch.randint(0, 352, (B,), generator=g).to(dev)}}
    return inp, tgt, g

model.train()
opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.0)
step = TrainStep(model, opt, crit)

def restore(st):
    bare.load_state_dict(st)                              # undo the BN running-statistics update

def local_grads(inp, tgt, part, factor=None):
    """this rank's own gradient of one part of the loss ("total"; "prior": multiplier * prior term; "effective": see
    below) through the bare module, gradient hooks off; `factor`: of factor * that part (a figure that is printed, not asserted)"""
    for p in bare.parameters(): p.grad = None
    st = {k: v.clone() for k, v in bare.state_dict().items()}
    torch.manual_seed(77)                                 # whatever a training forward draws, every run draws alike
    with model.no_sync():
        out = bare(inp); loss, _ = bare.get_loss(crit, tgt, out, EPOCH)
        term = loss["total"] if part == "total" else att.wt_decay * loss["prior"]
        if part == "effective":
            # the global loss, sum_r [(n_r / n) means_r + sums_r], is sum_r (n_r / n) [total_r + (n / n_r - 1) sums_r]:
            # the bracket is this rank's part of it, differentiated in ONE backward pass
            term = loss["total"] + (n / n_r - 1) * term
        (term if factor is None else term * factor).backward()
    torch.cuda.synchronize()
    restore(st)
    return {k: p.grad.clone() for k, p in bare.named_parameters() if p.grad is not None}

def stepped(inp, tgt, share):
    st = {k: v.clone() for k, v in bare.state_dict().items()}
    torch.manual_seed(77)
    loss, _ = step(0, inp, tgt, EPOCH, share=share)       # zero_grad, forward, scaled backward + exchange, step at lr 0
    torch.cuda.synchronize()
    restore(st)
    return {k: p.grad.clone() for k, p in bare.named_parameters() if p.grad is not None}, loss

def gathered(grads, k):
    parts = [torch.empty_like(grads[k]) for _ in range(W)]
    dist.all_gather(parts, grads[k])
    return parts

misses = []
with local_plans(model):                                  # the ranks' shapes differ: each tunes for itself (as `train` does)
    # ---- a global batch of 3 split 1 + 2
    n_r, n = (1, 3) if rank == 0 else (2, 3)
    inp, tgt, g = make(n_r, 100 + rank)
    st0 = {k: v.clone() for k, v in bare.state_dict().items()}
    with torch.no_grad():
        rows, T = bare(inp)["weights"].squeeze(1).shape
    restore(st0)
    assert rows == n_r * n_seg
    tgt["weights"] = torch.softmax(torch.randn(n_r, n_seg, T, 1, generator=g), 2).to(dev)
    for reduction in ARGS["reductions"]:
        # "batchmean": every term is a mean over clips.  "sum": the prior term is a sum over clips, cross entropy and
        # entropy stay means (ContrastLoss "sum" is an unreduced vector that cannot be back-propagated: contrast is off)
        att.loss_reduction = reduction
        att.use_contrast = reduction != "sum"
        crit["prior"] = torch.nn.KLDivLoss(reduction=reduction).to(dev)
        if att.use_contrast:
            crit["contrast"] = ContrastLoss(threshold=att.contrast_thresh, reduction=reduction)
        else:
            crit.pop("contrast", None)
        total = local_grads(inp, tgt, "total")
        prior = local_grads(inp, tgt, "prior") if reduction == "sum" else None
        effective = local_grads(inp, tgt, "effective") if reduction == "sum" else None
        synced, loss = stepped(inp, tgt, (n_r, n, W))
        again = local_grads(inp, tgt, "total")
        scaled = local_grads(inp, tgt, "total", n_r * W / n)
        def rel(a, b):
            return float((a - b).abs().max() / (b.abs().max() + 1e-20))
        # what the reference g_r itself is good for: a second run of it, and the factor applied before backward
        # against the factor applied to the finished gradient
        floor = {k: (rel(again[k], total[k]), rel(scaled[k], total[k] * (n_r * W / n))) for k in total}
        assert step.last_scale == (n_r * W / n, W if reduction == "sum" else None), step.last_scale
        assert step.last_scale_on == "gradient" and model.grad_weight is None      # k == 1: the wrapper weighed, and forgot
        assert set(loss) >= {"verb", "noun", "all_class", "prior", "entropy", "total"} and len(total) >= 12
        assert set(synced) == set(total)
        worst = 0.0
        for k in total:
            if reduction == "sum":
                # the global loss is the mean terms over all n clips + the prior summed over all n clips.  Its gradient,
                # sum_r (n_r / n) h_r with h_r the gradient of the rank's bracket above from ONE backward pass of the bare
                # module, is what is asserted.  The same quantity put together from two separately back-propagated
                # gradients, sum_r (n_r / n) g_r + sum_r (1 - n_r / n) p_r, is printed beside it: on a tensor that is a small
                # sum of cancelling contributions the two references themselves are 1e-4 apart (measured: pe.2.bias)
                parts = gathered(effective, k)
                want = (1 / 3) * parts[0] + (2 / 3) * parts[1]
                pk = prior[k] if k in prior else torch.zeros_like(total[k])
                parts, sums = gathered(total, k), gathered({k: pk}, k)
                other = (1 / 3) * parts[0] + (2 / 3) * parts[1] + (2 / 3) * sums[0] + (1 / 3) * sums[1]
                print("gradient rule sum       %-40s the reference in one backward pass against in two: %.3e"
                      % (k, float((other - want).abs().max() / (want.abs().max() + 1e-20))))
            else:
                parts = gathered(total, k)
                want = (1 / 3) * parts[0] + (2 / 3) * parts[1]           # sum_r (n_r / n) g_r
            err = float((synced[k] - want).abs().max() / (want.abs().max() + 1e-20))
            worst = max(worst, err)
            print("gradient rule %-9s %-40s err %.3e | g_r run to run %.3e | factor before / after backward %.3e"
                  % (reduction, k, err, floor[k][0], floor[k][1]))
            if not err < 1e-5:
                misses.append((reduction, k, err))
        print("gradient rule", reduction, "worst relative max-norm error", worst)
        if reduction == "sum":
            assert any(float(p.abs().max()) > 0 for p in prior.values())      # the sum term does reach the weights

    def even_split():
        # ---- an equal split 2 + 2: the factor is exactly one and is skipped, loss["total"] itself is back-propagated
        att.loss_reduction, att.use_contrast = "batchmean", True
        crit["prior"] = torch.nn.KLDivLoss(reduction="batchmean").to(dev)
        crit["contrast"] = ContrastLoss(threshold=att.contrast_thresh, reduction="batchmean")
        inp, tgt, g = make(2, 200 + rank)
        tgt["weights"] = torch.softmax(torch.randn(2, n_seg, T, 1, generator=g), 2).to(dev)
        taken = []
        real = step._shared_total
        def spy(loss, share, epoch):
            out = real(loss, share, epoch)
            taken.append(out is loss["total"])
            return out
        step._shared_total = spy
        even, _ = stepped(inp, tgt, (2, 4, W))
        assert taken == [True] and step.last_scale == (None, None) and model.grad_weight is None
        plain, _ = stepped(inp, tgt, None)
        assert taken == [True, True] and step.last_scale is None
        for k in even:
            assert torch.equal(even[k], plain[k]), k           # bit-identical to the step without a share
    if ARGS["even"]:
        even_split()
assert model._fired == set() and model._pending == []
assert not misses, misses                                 # every figure above is printed first; the bound is 1e-5
print("GRAD_OK", rank)
'''


def test_exchanged_gradient_is_the_global_batchs(tmp_path):
    """one `TrainStep` iteration on a global batch of 3 split 1 + 2, attention losses on (prior, contrast and entropy
    under the default "batchmean": every term a mean over clips): after the exchange every parameter gradient is
    sum_r (n_r / n) g_r, g_r from the bare module under `no_sync()` from the same weights, to tests/test_dp_gpu.py's
    relative max-norm bound of 1e-5; with 2 + 2 the factor is skipped and the step is bit-identical to one without a share.
    The worker prints, per tensor, the error, a second run of g_r against the first, and -- on one rank, no exchange --
    the gradient of `factor * loss` against `factor *` the gradient of the loss: why the factor is not put on the loss
    when it can go on the finished gradients (`TrainStep.__call__`)."""
    _run_ranks(tmp_path, _GRAD, {"reductions": ["batchmean"], "even": True}, "GRAD_OK")


def test_exchanged_gradient_with_a_sum_reduced_prior(tmp_path):
    """the same split with `loss_reduction="sum"` (prior and entropy; ContrastLoss "sum" cannot be back-propagated): the
    prior term is a sum over clips, so the global loss is sum_r (n_r / n) [total_r + (n / n_r - 1) m prior_r] and the
    exchanged gradient must be sum_r (n_r / n) h_r, h_r the gradient of the rank's bracket from one backward pass of the
    bare module under `no_sync()`; same bound.  The same quantity assembled from two separately back-propagated
    gradients (total and prior part) is printed, not asserted: for `pe.2.bias` the two references are 1.5e-4 apart
    (MI355X), for every other tensor at most 3.4e-6."""
    _run_ranks(tmp_path, _GRAD, {"reductions": ["sum"], "even": False}, "GRAD_OK")


_LOOPS = r'''
import glob, hashlib, logging
from attention_based_tbn_amd.config import load_config, get_modality
from attention_based_tbn_amd.core import tools
T = sys.modules["attention_based_tbn_amd.core.tools.train"]       # the package's `train` / `test` attributes are the functions
E = sys.modules["attention_based_tbn_amd.core.tools.test"]
cfg = load_config(ARGS["overrides"])
modality = get_modality(cfg)
root = ARGS["root"]
LOG = logging.getLogger("multi_rank_loops")
records = []
handler = logging.Handler()
handler.emit = records.append
LOG.addHandler(handler)
LOG.setLevel(logging.INFO)

models, validated, written, saves = [], [], [], []
real_build, real_validate, real_scores, real_save = T.build_model, T.validate, E.save_scores, T.save_checkpoint
T.build_model = lambda *a, **k: (lambda r: (models.append(r[0]), r)[1])(real_build(*a, **k))
T.validate = lambda *a, **k: (lambda r: (validated.append(r), r)[1])(real_validate(*a, **k))
T.save_checkpoint = lambda *a, **k: (saves.append(k["filename"]), real_save(*a, **k))[1]
E.save_scores = lambda *a, **k: (written.append(a[1]), real_scores(*a, **k))[1]

class Writer(object):
    rows = []
    def add_scalar(self, tag, value, epoch):
        self.rows.append(tag)

def digest(model):
    h = {}
    for k, v in list(model.module.named_parameters()) + list(model.module.named_buffers()):
        h[k] = hashlib.sha1(v.detach().cpu().numpy().tobytes()).hexdigest()
    return h

torch.manual_seed(1 + rank)                  # the ranks' generators differ: rank 0's decides the passes and the weights
np.random.seed(1 + rank)
tools.run_trainer(cfg, LOG, modality, Writer())
text = [r.getMessage() for r in records]
if rank == 0:
    assert any(t.startswith("Epoch: [1/1]") for t in text) and any("Batch Progress: [1/1]" in t for t in text), text[-20:]
    assert "train/total_loss" in Writer.rows and "val/accuracy/verb_top_1" in Writer.rows
    assert len(saves) == 1 and saves[0].endswith(".pth.tmp")
else:
    assert text == [] and Writer.rows == [] and saves == []         # only rank 0 logs, plots and writes
ckpts = glob.glob(os.path.join(root, cfg.model.checkpoint_dir, "loop", "*"))
assert len(ckpts) == 1 and ckpts[0].endswith(".pth"), ckpts         # one checkpoint, no temporary file left
data = torch.load(ckpts[0], map_location="cpu", weights_only=False)
assert data["epoch"] == 0 and len(data["train_loss"]) == 1 and len(data["validation_loss"]) == 1
model = models[0]
both = everyone(digest(model))
assert both[0] == both[1] and len(both[0]) > 20                     # parameters AND BatchNorm buffers, bit for bit
sd = model.module.state_dict()
assert all(torch.equal(sd[k].cpu(), v) for k, v in data["model"].items() if k.endswith("running_mean"))
assert len(validated) == 1
val = everyone((validated[0][0], validated[0][1], {k: v.cpu().tolist() for k, v in validated[0][2].items()}))
assert val[0] == val[1]
assert sum(sum(r) for r in val[0][2]["verb"]) == 3                  # every clip of the three was scored once
assert validated[0][0] == data["validation_loss"][0]

# ---- resume: every rank loads the checkpoint, one more epoch, without validation
cfg.train.pre_trained, cfg.val.enable = ckpts[0], False
tools.run_trainer(cfg, LOG, modality, prefetch=0)
cfg.train.pre_trained, cfg.val.enable = "", True
data = torch.load(ckpts[0], map_location="cpu", weights_only=False)
assert data["epoch"] == 1 and len(data["train_loss"]) == 2 and len(data["validation_loss"]) == 1
both = everyone(digest(models[1]))
assert both[0] == both[1]

# ---- run_tester with save_results: rank 0 writes every uid once, in annotation order
cfg.test.pre_trained, cfg.test.save_results = ckpts[0], True
cfg.test.annotation_file, cfg.test.results_file = ["ann.csv"], ["seen.json"]
del records[:]
tools.run_tester(cfg, LOG, modality)
dist.barrier()
out_file = os.path.join(root, "inferences", "seen.json")
assert written == ([out_file] if rank == 0 else [])
assert (records != []) == (rank == 0)
assert not [r for r in records if r.levelno >= logging.ERROR], [r.getMessage() for r in records if r.levelno >= logging.ERROR]
doc = json.load(open(out_file))
assert list(doc["results"].keys()) == ["11", "12", "13"]
assert all(len(v["verb"]) == 125 and len(v["noun"]) == 352 for v in doc["results"].values())
import threading
assert not [t for t in threading.enumerate() if t.name == "ClipLoader-producer" and t.is_alive()]
print("LOOPS_OK", rank)
'''


def test_loops_end_to_end_on_two_ranks(tmp_path):
    """one epoch of `run_trainer` (a train batch of 3 split 1 + 2; validation batches of 2 and 1, the latter an empty share
    on rank 0), a resume, and `run_tester` with save_results (test batches 1 + 1 and 0 + 1)"""
    import pandas as pd
    root = tmp_path / "data"
    overrides = U.write_big_dataset(root) + [
        "data.flow.enable=False", "model.attention.enable=False", "model.fusion_dropout=0", "val.vid_list=",
        "test.vid_list=", "test.annotation_file=ann.csv", "val.num_segments=2", "test.num_segments=2",
        "train.batch_size=3", "val.batch_size=2", "test.batch_size=2", "train.epochs=1", "out_dir=" + str(root),
        "exp_name=loop"]
    os.makedirs(root / "annotations", exist_ok=True)
    pd.to_pickle({}, str(root / "annotations" / "action_id_to_name.pkl"))
    _run_ranks(tmp_path, _LOOPS, {"overrides": overrides, "root": str(root)}, "LOOPS_OK", timeout=420)
