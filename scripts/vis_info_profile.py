#!/usr/bin/env python
"""Measures the visualiser's table on an MI355X and writes profiles/vis_summary.md:

  * `core.tools.vis.get_info` per clip at batch_size 1 and 8 against the reference's loop body (core/tools/vis.py:64-86:
    batch size 1, five `.item()` reads per clip) written out literally, in the same process on the same model and the
    same synthetic 256x456 dataset (tests/clip_loader_util.write_big_dataset, more annotation rows over its video);
    every arm reads through a `ClipLoader(prefetch=2)`; the arms alternate;
  * `tbn_clip_summary` at B = 64, heads of 125 + 352 classes, k = 5, 3 segments of T = 8: device events around
    back-to-back launches, per launch;
  * the largest observed error / bound ratios of the operator's probabilities and entropies over the cases of
    tests/vis_summary_ref.py (the bounds are derived there; each ratio has to stay at or below 1).

Usage:  python scripts/vis_info_profile.py [--clips 48] [--rounds 3] [--out profiles/vis_summary.md]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_loop(model, dataset, epic_classes, device):
    """the reference's get_info loop body, literally, over this package's batches of one clip"""
    import torch
    from attention_based_tbn_amd.core.utils import ClipLoader
    data_dict = {"vid_id": [], "gt_verb": [], "gt_noun": [], "pred_verb": [], "pred_noun": [], "entropy": []}
    loader = ClipLoader(dataset, 1, shuffle=False, prefetch=2)
    model.eval()
    try:
        with torch.no_grad():
            for data, target, _ in loader:
                out = model(data)
                data_dict["vid_id"].append(data["vid_id"][0])
                gt_verb = epic_classes.verbs[target["class"]["verb"].item()]
                gt_noun = epic_classes.nouns[target["class"]["noun"].item()]
                data_dict["gt_verb"].append(gt_verb)
                data_dict["gt_noun"].append(gt_noun)
                _, pred_verb = out["verb"].max(dim=1)
                _, pred_noun = out["noun"].max(dim=1)
                pred_verb = epic_classes.verbs[pred_verb.item()]
                pred_noun = epic_classes.nouns[pred_noun.item()]
                data_dict["pred_verb"].append(pred_verb)
                data_dict["pred_noun"].append(pred_noun)
                if "weights" in out.keys():
                    b = 1
                    n = out["weights"].shape[0]
                    weights = out["weights"].view(b * n, -1)
                    entropy = (-1 * (weights * torch.log(weights + 1e-6)).sum(1)).mean()
                    data_dict["entropy"].append(entropy.item())
                else:
                    data_dict["entropy"].append("N/A")
    finally:
        loader.close()
    return data_dict


def table_times(clips, rounds):
    import numpy as np
    import torch
    from tests import clip_loader_util as U
    from tests import vis_util as V
    from attention_based_tbn_amd.config import get_modality, load_config
    from attention_based_tbn_amd.core.dataset import EpicClasses
    from attention_based_tbn_amd.core.models import build_model
    from attention_based_tbn_amd.core.tools import create_dataset, get_info
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as root:
        overrides = U.write_big_dataset(root)
        rows = [(100 + i,) + (0,) + U.ROWS[i % 3][2:4] + (i % 125, i % 352) for i in range(clips)]
        V.write_annotations(root, "ann_many.csv", ("P02_01",), rows)
        cfg = load_config(overrides + ["data.flow.enable=False", "model.attention.type=mha", "model.fusion_dropout=0",
                                       "test.vid_list=", "test.annotation_file=[ann_many.csv]", "test.num_segments=2"])
        epic_classes = EpicClasses(V.write_class_files(root, ["verb%03d" % i for i in range(125)],
                                                       ["noun%03d" % i for i in range(352)]))
        torch.manual_seed(0)
        np.random.seed(0)
        model, _, _ = build_model(cfg, get_modality(cfg), dev)
        dataset = create_dataset(cfg)
        arms = {"reference loop (batch 1, .item() per clip)": lambda: reference_loop(model, dataset, epic_classes, dev),
                "get_info(batch_size=1)": lambda: get_info(model, dataset, epic_classes, dev, batch_size=1, widget=False),
                "get_info(batch_size=8)": lambda: get_info(model, dataset, epic_classes, dev, batch_size=8, widget=False)}
        times = {name: [] for name in arms}
        tables = {}
        for name, fn in arms.items():       # warm-up: every batch shape once
            tables[name] = fn()
        for _ in range(rounds):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / clips)
        ref = tables["reference loop (batch 1, .item() per clip)"]
        same = {}
        for name in list(arms)[1:]:
            df = tables[name]
            same[name] = all(df[c].tolist() == ref[c] for c in ("vid_id", "gt_verb", "gt_noun", "pred_verb", "pred_noun"))
    return times, same


def kernel_time(launches=1000):
    import torch
    from attention_based_tbn_amd import ops
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(3)
    scores = {"verb": (torch.randn(64, 125, generator=gen) * 4).to(dev), "noun": (torch.randn(64, 352, generator=gen) * 4).to(dev)}
    weights = torch.softmax(torch.randn(64 * 3, 8, generator=gen), 1).to(dev)
    idx = torch.empty((64, 2, 5), dtype=torch.int32, device=dev)
    prob = torch.empty((64, 2, 5), dtype=torch.float32, device=dev)
    ent = torch.empty((64,), dtype=torch.float32, device=dev)
    for _ in range(20):
        ops.clip_summary(scores, 5, weights, 3, out=(idx, prob, ent))
    torch.cuda.synchronize()
    per_launch = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            ops.clip_summary(scores, 5, weights, 3, out=(idx, prob, ent))
        e1.record()
        torch.cuda.synchronize()
        per_launch.append(e0.elapsed_time(e1) * 1e3 / launches)
    return per_launch


def ratios():
    from tests import vis_summary_ref as R
    worst_p, worst_e = 0.0, 0.0
    for n, case in enumerate(R.cases()):
        p, e = R.check_case(case, R.run_case(case, 100 + n, "cuda"))
        worst_p, worst_e = max(worst_p, p), max(worst_e, e)
    return worst_p, worst_e, len(R.cases())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vis_summary.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vis_info_profile: no GPU; nothing is measured without one")
    worst_p, worst_e, n_cases = ratios()
    kernel = kernel_time()
    times, same = table_times(args.clips, args.rounds)
    lines = ["# Visualiser table and clip summary, measured on an MI355X", "",
             "Written by `scripts/vis_info_profile.py --clips %d --rounds %d` (%s)." % (
                 args.clips, args.rounds, torch.cuda.get_device_name(0)), "",
             "## `get_info` per clip", "",
             "RGB + Audio, `model.attention.type=mha`, 2 segments, 256x456 frames, %d clips; every arm reads through a "
             "`ClipLoader(prefetch=2)`; one warm-up pass per arm, then %d timed passes per arm, arms alternated; host clock "
             "around a pass that ends in a device synchronise." % (args.clips, args.rounds), "",
             "| arm | ms per clip: median | min | max | same names as the reference loop |", "|---|---|---|---|---|"]
    for name, t in times.items():
        lines.append("| %s | %.3f | %.3f | %.3f | %s |" % (name, float(np.median(t)), min(t), max(t), same.get(name, "-")))
    lines += ["", "## `tbn_clip_summary` alone", "",
              "B = 64, heads of 125 + 352 classes, k = 5, 3 segments of T = 8 per clip; device events around 1000 back-to-back "
              "launches through `ops.clip_summary(out=)`, five windows: the figure includes the wrapper's enqueue rate.", "",
              "| us per launch: median | min | max |", "|---|---|---|",
              "| %.2f | %.2f | %.2f |" % (float(np.median(kernel)), min(kernel), max(kernel)), "",
              "## Error against the fp64 restatement, as a share of the derived bound", "",
              "Over the %d cases of `tests/vis_summary_ref.py` (bounds derived there from fp32 rounding):" % n_cases, "",
              "| quantity | bound | largest observed error / bound |", "|---|---|---|",
              "| softmax probability, relative | (2 (max - min) + 32) 2^-24 per row | %.3f |" % worst_p,
              "| attention entropy, absolute | 2^-20 (1 + S) per clip | %.3f |" % worst_e, ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
