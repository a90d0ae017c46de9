"""One train step of ResNet-50 on the operator-level HIP path vs the same network built from torch.nn on torch-ROCm (MIOpen).

Arms alternate in ONE process: forward + backward + SGD step of `Resnet(50, "RGB", 3)` with `FusedSGD`, and of a plain
nn.Conv2d / nn.BatchNorm2d twin with torch.optim.SGD, on the same frames (default 96 x 3 x 224 x 224).  Reported: the median
of the rounds after warm-up per arm, then -- from `tbn_profile_enable(2)` over one more HIP step -- the share of every
profiled kernel (conv GEMMs and the residual-join kernels) and the achieved GB/s of the three join kernels against their
algorithmic bytes.  Every arm runs under a time limit of its own (SIGALRM): a step that does not come back ends the script.

    python scripts/resnet_step.py [--frames 96] [--size 224] [--rounds 3] [--warmup 1] [--arm-timeout 240] [--out file.md]
"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COUNTS = (3, 4, 6, 3)


class TorchBottleneck(nn.Module):
    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width)
        self.conv2, self.bn2 = nn.Conv2d(width, width, 3, stride, 1, bias=False), nn.BatchNorm2d(width)
        self.conv3, self.bn3 = nn.Conv2d(width, 4 * width, 1, bias=False), nn.BatchNorm2d(4 * width)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or cin != 4 * width:
            self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * width, 1, stride, bias=False), nn.BatchNorm2d(4 * width))

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class TorchResnet50(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 64
        for i, (width, n) in enumerate(zip((64, 128, 256, 512), COUNTS)):
            blocks = []
            for b in range(n):
                blocks.append(TorchBottleneck(cin, width, 2 if (i > 0 and b == 0) else 1))
                cin = 4 * width
            layers.append(nn.Sequential(*blocks))
        self.model = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
                                   nn.MaxPool2d(3, 2, 1), *layers, nn.AdaptiveAvgPool2d((1, 1)))

    def forward(self, x):
        return self.model(x).flatten(1)


class TimeLimit:
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def expired(*_):
            raise TimeoutError("%s did not finish within %d s" % (self.what, self.seconds))
        signal.signal(signal.SIGALRM, expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--arm-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from attention_based_tbn_amd._lib import lib
    from attention_based_tbn_amd.core.models import Resnet
    from attention_based_tbn_amd.core.utils import FusedSGD
    dev = torch.device("cuda")
    torch.manual_seed(0)
    hip = Resnet(50, "RGB", 3).to(dev).train()
    ref = TorchResnet50().to(dev).train()
    ref.load_state_dict(hip.state_dict())
    x = torch.randn(a.frames, 3, a.size, a.size, device=dev)
    R = torch.randn(a.frames, 2048, device=dev) / a.frames
    opt_hip = FusedSGD(hip.parameters(), 0.01, momentum=0.9, weight_decay=0)
    opt_ref = torch.optim.SGD(ref.parameters(), 0.01, momentum=0.9, weight_decay=0)

    def step_hip():
        opt_hip.zero_grad()
        (hip(x) * R).sum().backward()
        opt_hip.step()

    def step_ref():
        opt_ref.zero_grad()
        (ref(x) * R).sum().backward()
        opt_ref.step()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = {"hip": step_hip, "torch": step_ref}
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.rounds):
        for name, fn in arms.items():
            with TimeLimit(a.arm_timeout, "arm %s, round %d" % (name, r)):
                t0 = time.time()
                ms = timed(fn)
            print("round %d %-5s %8.2f ms (host %.1f s)" % (r, name, ms, time.time() - t0), flush=True)
            if r >= a.warmup:
                times[name].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}

    # per-kernel shares of one more HIP step
    L = lib()
    L.tbn_profile_reset()
    L.tbn_profile_enable(2)
    with TimeLimit(a.arm_timeout, "profiled hip step"):
        step_hip()
        torch.cuda.synchronize()
    n = L.tbn_profile_num_entries()
    rows = []
    for i in range(n):
        name = C.create_string_buffer(256)
        launches, ms, fl, by = C.c_long(), C.c_double(), C.c_double(), C.c_double()
        L.tbn_profile_entry(i, name, 256, C.byref(launches), C.byref(ms), C.byref(fl))
        L.tbn_profile_entry_bytes(i, C.byref(by))
        rows.append((name.value.decode().split(" | ")[0], launches.value, ms.value, fl.value, by.value))
    L.tbn_profile_enable(0)
    total = sum(r[2] for r in rows) or 1.0
    rows.sort(key=lambda r: -r[2])
    lines = ["# ResNet-50 train step on the operator path (%d x 3 x %d x %d, fp32)" % (a.frames, a.size, a.size), "",
             "| arm | median step ms | rounds |", "|---|---|---|"]
    for k in arms:
        lines.append("| %s | %.2f | %s |" % (k, med[k], " ".join("%.2f" % t for t in times[k])))
    lines += ["", "hip / torch = %.3f" % (med["hip"] / med["torch"]),
              "", "Profiled kernels of one HIP step (sum of kernel times %.2f ms):" % total, "",
              "| kernel | launches | ms | share | TFLOP/s | alg. GB/s |", "|---|---|---|---|---|---|"]
    for name, launches, ms, fl, by in rows[:24]:
        lines.append("| `%s` | %d | %.3f | %.1f %% | %s | %s |" % (
            name[:70], launches, ms, 100 * ms / total, "%.1f" % (fl / ms / 1e9) if fl and ms else "-",
            "%.0f" % (by / ms / 1e6) if by and ms else "-"))
    join = {}
    for name, launches, ms, fl, by in rows:
        for fam in ("bn_res_apply_kernel", "bn_res_bwd_reduce_kernel", "bn_res_bwd_apply_kernel"):
            if name.startswith(fam):
                j = join.setdefault(fam, [0, 0.0, 0.0])
                j[0] += launches
                j[1] += ms
                j[2] += by
    lines += ["", "| join kernel | launches | ms | algorithmic GB | GB/s |", "|---|---|---|---|---|"]
    for fam, (launches, ms, by) in join.items():
        lines.append("| `%s` | %d | %.3f | %.2f | %.0f |" % (fam, launches, ms, by / 1e9, by / ms / 1e6 if ms else 0))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"hip_ms": med["hip"], "torch_ms": med["torch"], "frames": a.frames, "size": a.size}))


if __name__ == "__main__":
    main()
