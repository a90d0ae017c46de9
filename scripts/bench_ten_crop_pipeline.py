"""Ten-crop test pipeline: one tbn_frames_to_tensor_crops launch per modality (arm A) against the ten launches of the
unchanged tbn_frames_to_tensor it replaces (arm B: five windows x plain / mirrored), alternated in one process.

Workload: one 25-segment test clip -- 25 RGB frames and 25 ten-frame Flow stacks, 256x456 -> Rescale(256) (identity at
this size, as for EPIC frames) -> ten 224x224 crops = 250 RGB rows and 250 Flow rows.  Both arms read the same uint8
frames and write the same number of fp32 rows into one buffer.  RGB: the same rows, in the reference's order only in
arm A (arm B leaves them window- and mirror-major; checked below).  Flow: arm B cannot interleave plain and mirrored
images inside a stack as FixedCrop + Stack do, so its rows match in count and bytes, not in content.
Timed with device events around `reps` back-to-back calls (Python + ctypes launch cost included in both arms).
HBM-bound: algorithmic bytes = fp32 output written once + one uint8 read per output element.
Usage: python scripts/bench_ten_crop_pipeline.py [alternations=5] [reps=50]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attention_based_tbn_amd._lib import call, ptr, stream_ptr  # noqa: E402
from attention_based_tbn_amd.config import load_config  # noqa: E402
from attention_based_tbn_amd.core.dataset import FixedCrop  # noqa: E402

ALTERNATIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
H, W, CROP, SEG = 256, 456, 224, 25
assert torch.cuda.is_available(), "needs the MI355X"
cfg = load_config([])
rng = np.random.RandomState(0)
windows = FixedCrop(CROP, [0, 1, 2, 3, 4]).windows(H, W)
xs, ys = (C.c_int * 5)(*[x for x, _ in windows]), (C.c_int * 5)(*[y for _, y in windows])


def modality(name):
    c, stack = (3, 1) if name == "RGB" else (1, 10)
    node = cfg.data.rgb if name == "RGB" else cfg.data.flow
    frames = torch.from_numpy(rng.randint(0, 256, (SEG * stack, H, W, c)).astype(np.uint8)).cuda()
    mean, std = torch.tensor(list(node.mean)).cuda(), torch.tensor(list(node.std)).cuda()
    n = frames.shape[0]
    out_a = torch.empty((SEG * 10, c * stack, CROP, CROP), device="cuda")
    out_b = torch.empty_like(out_a)

    def arm_a():
        call("tbn_frames_to_tensor_crops", ptr(frames), n, H, W, c, 0, 0, W, H, W, H, xs, ys, 5, CROP, CROP, 2, stack,
             ptr(mean), ptr(std), mean.numel(), 1, ptr(out_a), stream_ptr())

    def arm_b():
        k = 0
        for x, y in windows:
            for flip in (0, 1):
                call("tbn_frames_to_tensor", ptr(frames), n, H, W, c, 0, 0, W, H, W, H, x, y, CROP, CROP, flip, stack,
                     ptr(mean), ptr(std), mean.numel(), 1, ptr(out_b[k * SEG:]), stream_ptr())
                k += 1
    return name, arm_a, arm_b, out_a, out_b


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3          # us per call


mods = [modality("RGB"), modality("Flow")]
for name, a, b, out_a, out_b in mods:               # warm both arms, check what can be checked
    for _ in range(3):
        a()
        b()
    torch.cuda.synchronize()
    if name == "RGB":       # arm A row (w * SEG + i) * 2 + f  ==  arm B row (w * 2 + f) * SEG + i
        same = torch.equal(out_a.view(5, SEG, 2, -1), out_b.view(5, 2, SEG, -1).transpose(1, 2))
        print(f"RGB: the two arms hold the same rows: {same}")
        assert same
res = {(name, arm): [] for name, *_ in mods for arm in "AB"}
for _ in range(ALTERNATIONS):
    for name, a, b, out_a, _ in mods:
        res[name, "A"].append(timed(a))
        res[name, "B"].append(timed(b))
print(f"{ALTERNATIONS} alternations x {REPS} calls; us per call (one modality, 250 rows of {CROP}x{CROP})")
total = {"A": 0.0, "B": 0.0}
for name, _, _, out_a, _ in mods:
    alg = out_a.numel() * 5
    for arm, what in (("A", "1 launch  tbn_frames_to_tensor_crops"), ("B", "10 launches tbn_frames_to_tensor   ")):
        v = res[name, arm]
        med = statistics.median(v)
        total[arm] += med
        print(f"{name:4s} arm {arm} ({what}): median {med:8.1f} us  range {min(v):8.1f} .. {max(v):8.1f}  "
              f"-> {alg / med / 1e6:5.2f} TB/s algorithmic")
print(f"both modalities, sum of medians: arm A {total['A']:.1f} us, arm B {total['B']:.1f} us, "
      f"A / B = {total['A'] / total['B']:.3f}")
