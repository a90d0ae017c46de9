"""A/B of the attention-weight path of the learnt fusion variants (model.attention.type = unimodal | proto) in a
config-3 shaped train step (RGB + Audio, B = 64 clips x 3 segments, 1.279 s audio): the weights as they were computed
before ops.attn_weights -- F.gumbel_softmax, plus torch.matmul for the prototypes, rebuilt here -- against the one-launch
HIP operator.  Both arms run in ONE process and alternate (same box, same clocks); per arm the median over the
alternations of the mean step time, and the 'turn' from the library's kernel timeline: the GPU time between the end of
the last backbone forward kernel (spatial_mean_fwd) and the start of the first backward kernel (spatial_mean_bwd).
With --type mha both arms are the same code (the TBN's own call shape stays on tbn_mha_q1): a null control that shows
the run-to-run range of the method.

    python scripts/attn_general_ab.py --type unimodal proto mha --alternations 7 --steps 10
"""
import argparse
import csv
import gc
import json
import os
import statistics
import sys
import tempfile
import time
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from attention_based_tbn_amd import ops  # noqa: E402
from attention_based_tbn_amd._lib import lib  # noqa: E402


def old_unimodal_attend(self, vis, seq):
    logits = self._logits(vis)
    if self.training and self.use_gumbel:
        w = F.gumbel_softmax(logits, tau=self.temperature, hard=self.one_hot)
    else:
        w = F.softmax(logits, dim=1)
    return ops.weighted_sum(seq, w), w


def old_proto_attend(self, vis, seq):
    h = ops.linear(vis, self.seq[0].weight, self.seq[0].bias, relu=True)
    logits = ops.linear(h, self.seq[2].weight, self.seq[2].bias)
    if self.training and self.use_gumbel:
        m = F.gumbel_softmax(logits, tau=self.temperature, hard=True)
    else:
        m = F.softmax(logits, dim=1)
    w = torch.matmul(m, self.prototype_wts)
    return ops.weighted_sum(seq, w), w


OLD = {"unimodal": old_unimodal_attend, "proto": old_proto_attend}


def turn_us(path):
    """(turn in us, library launches inside it) of the last step in a timeline CSV"""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    fwd = [i for i, r in enumerate(rows) if "spatial_mean_fwd" in r["Kernel_Name"]]
    bwd = [i for i, r in enumerate(rows) if "spatial_mean_bwd" in r["Kernel_Name"]]
    end_fwd = max(int(rows[i]["End_Timestamp"]) for i in fwd)
    first = min(i for i in bwd if int(rows[i]["Start_Timestamp"]) >= end_fwd)
    inside = sum(1 for r in rows if int(r["Start_Timestamp"]) >= end_fwd
                 and int(r["Start_Timestamp"]) < int(rows[first]["Start_Timestamp"]))
    return (int(rows[first]["Start_Timestamp"]) - end_fwd) / 1e3, inside


def run(att_type, alternations, steps, batch, device):
    from attention_based_tbn_amd.config import load_config, get_modality
    from attention_based_tbn_amd.core.models import build_model
    from attention_based_tbn_amd.core.utils import FusedSGD
    ov = list(bench.CONFIGS[3]["ov"]) + ["model.attention.type=" + att_type, "data.audio.dropout=0"]
    cfg = load_config(ov)
    modality = get_modality(cfg)
    torch.manual_seed(0)
    model, criterion, _ = build_model(cfg, modality, device)
    model.train(True)
    core = getattr(model, "module", model)
    layer = core.attention_layer
    opt = FusedSGD([p for p in model.parameters() if p.requires_grad], lr=cfg.train.optim.lr,
                   momentum=cfg.train.optim.momentum, weight_decay=cfg.train.optim.weight_decay)
    inp, tgt = bench.synthetic_batch(batch, cfg.train.num_segments, device, seed=0, modality=modality)

    def step():
        opt.zero_grad(set_to_none=True)
        out = model(inp)
        loss, _ = model.get_loss(criterion, tgt, out, 0)
        loss["total"].backward()
        opt.step(clip_grad=cfg.train.clip_grad, grads_consumed=True)

    def arm(name):
        if name == "old" and att_type in OLD:
            layer.attend = types.MethodType(OLD[att_type], layer)
        else:
            layer.__dict__.pop("attend", None)

    L = lib()
    tmp = tempfile.mkdtemp(prefix="attn_ab_")
    for name in ("old", "new"):         # priming: plans, allocator, both code paths
        arm(name)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    ms = {"old": [], "new": []}
    turn = {"old": [], "new": []}
    launches = {}
    for alt in range(alternations):
        for name in (("old", "new") if alt % 2 == 0 else ("new", "old")):
            arm(name)
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
            L.tbn_timeline_enable(1)
            step()
            L.tbn_timeline_enable(0)
            path = os.path.join(tmp, "tl.csv")
            L.tbn_timeline_dump(path.encode())
            t, n = turn_us(path)
            turn[name].append(t)
            launches[name] = n
    arm("new")
    gc.unfreeze()
    res = {"type": att_type, "batch": batch, "alternations": alternations, "steps_per_sample": steps}
    for name in ("old", "new"):
        res[name] = {"step_ms_median": round(statistics.median(ms[name]), 3),
                     "step_ms_range": [round(min(ms[name]), 3), round(max(ms[name]), 3)],
                     "turn_us_median": round(statistics.median(turn[name]), 1),
                     "turn_us_range": [round(min(turn[name]), 1), round(max(turn[name]), 1)],
                     "library_launches_in_turn": launches[name]}
    res["step_ms_delta_new_minus_old"] = round(res["new"]["step_ms_median"] - res["old"]["step_ms_median"], 3)
    res["turn_us_delta_new_minus_old"] = round(res["new"]["turn_us_median"] - res["old"]["turn_us_median"], 1)
    del model, opt
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--type", nargs="+", default=["unimodal", "proto", "mha"], choices=["unimodal", "proto", "mha"])
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=bench.CONFIGS[3]["batch"])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert args.alternations >= 5, "the median of at least five alternations"
    bench.pin_plans()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lines = []
    for t in args.type:
        lines.append(json.dumps(run(t, args.alternations, args.steps, args.batch, device)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
