"""`DataParallel.weigh_next_backward` and the two places `TrainStep(share=)` can put its factor, on two gloo ranks on the
CPU: a global batch of 3 rows split 1 + 2, one tensor large enough for the gradient-hook path and small ones for the packed
buffer.  The exchanged gradient must be the full batch's whichever way the factor travels."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import datetime, os, sys, copy, torch, torch.distributed as dist, torch.nn as nn
sys.path.insert(0, sys.argv[1])
from attention_based_tbn_amd.config import load_config
from attention_based_tbn_amd.core.models.dataparallel import DataParallel
from attention_based_tbn_amd.core.utils.train_step import TrainStep
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=2, timeout=datetime.timedelta(seconds=60))
rank = dist.get_rank()
K, OVERLAP = int(os.environ["WX_K"]), os.environ["WX_OVERLAP"] == "1"

class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.cfg = load_config(["model.attention.enable=False"])
        self.a = nn.Linear(600, 600)                      # 360000 elements: reduced from its gradient hook
        self.b = nn.Linear(600, 3)                        # small: the packed buffer
    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))
    def get_loss(self, criterion, target, out, epoch=0):
        loss = ((out - target) ** 2).mean()
        return {"all_class": loss, "total": loss}, out.shape[0]

torch.manual_seed(0)
ref = Net().double()
model = DataParallel(copy.deepcopy(ref), overlap=OVERLAP)
assert model.active and model.world_size == 2
g = torch.Generator().manual_seed(5)
X, Y = torch.randn(3, 600, generator=g).double(), torch.randn(3, 3, generator=g).double()
rows = slice(0, 1) if rank == 0 else slice(1, 3)
share = (1, 3, 2) if rank == 0 else (2, 3, 2)
opt = torch.optim.SGD(model.parameters(), lr=0.0)
step = TrainStep(model, opt, None, accumulator_step=K)
it = K - 1 if K > 1 else 0                                # an iteration that zeroes first and exchanges (see TrainStep)
assert step.zeroes(it) and (K == 1 or not step.steps(it))
if K > 1:
    step.clip_grad = 1e9                                  # clipping on: every iteration synchronises, nothing is clipped
loss, _ = step(it, X[rows], Y[rows], 0, share=share)
assert step.last_scale == (share[0] * 2 / 3, None) and step.last_scale_on == ("gradient" if K == 1 else "loss")
assert model.grad_weight is None and model._pending == []
want_loss, _ = ref.get_loss(None, Y[rows], ref(X[rows]))
assert torch.allclose(loss["total"].detach() * K, want_loss["total"].detach(), rtol=1e-12)     # the rank's own, un-scaled
full, _ = ref.get_loss(None, Y, ref(X))
(full["total"] / K).backward()
for (n, p), (_, q) in zip(model.module.named_parameters(), ref.named_parameters()):
    assert torch.allclose(p.grad, q.grad, rtol=1e-10, atol=1e-14), (n, float((p.grad - q.grad).abs().max()))
# the weight is used once: the next backward without one is the plain average
model.zero_grad(set_to_none=True)
model.get_loss(None, Y[rows], model(X[rows]))[0]["total"].backward()
with model.no_sync():
    mine = copy.deepcopy(ref)
    mine.get_loss(None, Y[rows], mine(X[rows]))[0]["total"].backward()
for (n, p), (_, q) in zip(model.module.named_parameters(), mine.named_parameters()):
    both = [torch.empty_like(q.grad) for _ in range(2)]
    dist.all_gather(both, q.grad)
    assert torch.allclose(p.grad, (both[0] + both[1]) / 2, rtol=1e-10, atol=1e-14), n
print("WX_OK", rank)
dist.destroy_process_group()
'''


@pytest.mark.parametrize("k,overlap", [(1, True), (1, False), (2, True)])
def test_factor_on_the_gradients_or_on_the_loss_gives_the_full_batch_gradient(tmp_path, k, overlap):
    script = tmp_path / "wx_worker.py"
    script.write_text(_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", WX_K=str(k), WX_OVERLAP=str(int(overlap)))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"WX_OK {r}" in o, "\n----\n".join(x[-2500:] for x in outs)
