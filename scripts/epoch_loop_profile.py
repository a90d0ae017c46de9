"""Measurements behind profiles/epoch_loop.md (needs the MI355X; no fallback).

The train loop of `core.tools.train` over the synthetic dataset of scripts/clip_loader_profile.py (BASELINE config 4: RGB +
Flow + Audio, async sampling, attention off, B = 32 clips x 3 segments, 256x456 JPEG files -> 224 crops), four arms in one
process, alternated repetition by repetition after warm-up:

  (a) the loop over `ClipLoader(prefetch=0, rng="private")`: loader, then step -- what a loop costs without prefetch;
  (b) the same loop over `ClipLoader(prefetch=2)`;
  (c) the step alone (`TrainStep` + `DeviceMetric`) on one resident batch;
  (d) `Video_Dataset.batch` alone.

(a) and (b) are timed per epoch of --batches batches (a host clock round the epoch, ending in a device synchronise) and
reported per batch, so (b) carries its pipeline fill: the first batch of an epoch is not overlapped with anything.  Each
(threads, entropy) setting runs in a child process of its own under a time limit; the first failure ends the run.  The
synchronisation count per batch of `Metric` against `DeviceMetric` is taken by counting the calls of `.item()`, `.tolist()`,
`.cpu()`, `.numpy()` and `float()` on device tensors inside `set_metrics`.

    python scripts/epoch_loop_profile.py [--batches 12] [--reps 7] [--out profiles/epoch_loop.md]
"""
import argparse
import json
import logging
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MODALITY = ["RGB", "Flow", "Audio"]
SETTINGS = [(8, "host"), (16, "host"), (8, "device"), (16, "device")]
CHILD_LIMIT = 300          # seconds per (threads, entropy) child


def stats(t):
    import numpy as np
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def count_syncs(cfg, out, target, batch_size, loss):
    """calls that make the host wait for the device, inside one `set_metrics` of each class"""
    import torch
    from attention_based_tbn_amd.core.utils import DeviceMetric, Metric
    names = ("item", "tolist", "cpu", "numpy", "__float__")
    real = {n: getattr(torch.Tensor, n) for n in names}
    counts = {}

    def counting(name, box):
        def call(self, *a, **kw):
            if self.is_cuda:
                box[0] += 1
            return real[name](self, *a, **kw)
        return call
    for cls in (Metric, DeviceMetric):
        metric = cls(cfg, 4, torch.device("cuda"))
        metric.set_metrics(out, target, batch_size, loss)        # first use apart
        box = [0]
        for n in names:
            setattr(torch.Tensor, n, counting(n, box))
        try:
            metric.set_metrics(out, target, batch_size, loss)
        finally:
            for n in names:
                setattr(torch.Tensor, n, real[n])
        counts[cls.__name__] = box[0]
    return counts


def child(args):
    import numpy as np
    import torch
    from clip_loader_profile import write_dataset
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import Video_Dataset, get_transforms
    from attention_based_tbn_amd.core.models import build_model
    from attention_based_tbn_amd.core.tools import train
    from attention_based_tbn_amd.core.utils import ClipLoader, DeviceMetric, TrainStep, build_optimizer
    if not torch.cuda.is_available():
        raise SystemExit("epoch_loop_profile: needs the MI355X")
    dev = torch.device("cuda")
    log = logging.getLogger("epoch_loop_profile")
    log.setLevel(logging.WARNING)
    B, nb = 32, args.batches
    with tempfile.TemporaryDirectory() as root:
        vids, _ = write_dataset(root, B * nb, np.random.RandomState(3))
        cfg = load_config(["data_dir=" + root, "data.rgb.dir_prefix=rgb", "data.flow.dir_prefix=flow",
                           "data.audio.dir_prefix=audio", "data.audio.read_audio_pickle=True", "data.sampling=async",
                           "model.attention.enable=False", "data.audio.audio_length=1.279", "train.num_segments=3",
                           "train.batch_size=%d" % B])
        tfs = get_transforms(cfg, MODALITY, "train")
        ds = Video_Dataset(cfg, vids, "ann.csv", MODALITY, transform=tfs, mode="train", threads=args.threads,
                           entropy=args.entropy)
        torch.manual_seed(0)
        np.random.seed(0)
        model, criterion, _ = build_model(cfg, MODALITY, dev)
        optimizer, scheduler, _ = build_optimizer(cfg, model)
        sync_loader = ClipLoader(ds, B, shuffle=True, prefetch=0, rng="private")
        pre_loader = ClipLoader(ds, B, shuffle=True, prefetch=2)
        rng = np.random.RandomState(1)
        order = list(range(B))
        data, target = ds.batch(order, rng=rng)
        step = TrainStep.from_config(cfg, model, optimizer, criterion)
        model.train()

        def epoch(loader):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train(cfg, model, loader, optimizer, scheduler, criterion, 0, log, dev)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / nb

        def step_alone():
            metric = DeviceMetric(cfg, nb, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(nb):
                loss, bs = step(it, data, target, 0)
                metric.set_metrics(step.last_out, target, bs, loss)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / nb

        def batch_alone():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(nb):
                ds.batch(order, rng=rng)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / nb

        arms = dict(a=lambda: epoch(sync_loader), b=lambda: epoch(pre_loader), c=step_alone, d=batch_alone)
        for _ in range(2):                       # warm-up: plans, tile choices, caches, the loader's stream and thread
            for fn in arms.values():
                fn()
        times = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                times[k].append(fn())
        res = dict(threads=args.threads, entropy=args.entropy, batches=nb, reps=args.reps, clips=B,
                   device=torch.cuda.get_device_name(0), **{k: stats(v) for k, v in times.items()})
        loss, bs = step(0, data, target, 0)
        res["syncs_per_batch"] = count_syncs(cfg, step.last_out, target, bs, loss)
        pre_loader.close()
    print("RESULT " + json.dumps(res), flush=True)


def row(r):
    a, b, c, d = r["a"], r["b"], r["c"], r["d"]
    spread = a["max"] - a["min"]
    gain = a["median"] - b["median"]
    floor = max(c["median"], d["median"])

    def cell(s):
        return "%.1f (%.1f–%.1f)" % (s["median"], s["min"], s["max"])
    verdict = "yes" if gain > spread else "NO"
    return ("| %d | %s | %s | %s | %s | %s | %.2f | %+.1f | %.1f | %.1f | %s |" % (
        r["threads"], r["entropy"], cell(a), cell(b), cell(c), cell(d), a["median"] / b["median"], b["median"] - floor,
        gain, spread, verdict)), gain > spread


def report(results, args):
    lines = ["# Epoch loop: prefetching loader and sync-free metric", "",
             "Written by `scripts/epoch_loop_profile.py` on %s: the train loop of `core.tools.train` on the synthetic" % results[0]["device"],
             "config-4 dataset (B = 32 clips x 3 segments, 256x456 JPEG files), %d batches per epoch, %d repetitions per arm," % (args.batches, args.reps),
             "arms alternated in one process after two warm-up rounds.  Milliseconds per batch, median (min–max).", "",
             "- (a) loop over `ClipLoader(prefetch=0, rng=\"private\")`: loader, then step",
             "- (b) the same loop over `ClipLoader(prefetch=2)`; its epochs include the pipeline fill (the first batch of an",
             "  epoch overlaps nothing), so over n batches the floor is max(c, d) + min(c, d) / n, not max(c, d)",
             "- (c) step + `DeviceMetric` alone on a resident batch; (d) `Video_Dataset.batch` alone", "",
             "The claim checked: (b) is faster than (a) by more than (a)'s own min–max spread.", "",
             "| threads | entropy | (a) no prefetch | (b) prefetch=2 | (c) step | (d) batch() | a/b | b − max(c,d) | a − b | spread of a | a − b > spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    held = []
    for r in results:
        text, ok = row(r)
        lines.append(text)
        held.append(ok)
    lines += ["", "Result: the claim %s." % ("holds in every setting" if all(held) else
                                           "holds in %d of %d settings; where the last column says NO, prefetching did not "
                                           "beat the synchronous loop by more than its spread" % (sum(held), len(held))), "",
              "The step here runs with the launch plans the engine chooses on first use, not the pinned plans of `bench.py`, so",
              "(c) is not the benchmark's number; the comparison is between arms of this run.", "",
              "## Host synchronisations per batch inside `set_metrics`", "",
              "Calls of `.item()`, `.tolist()`, `.cpu()`, `.numpy()`, `float()` on device tensors (config 4: two heads, top-1/5):", ""]
    s = results[0]["syncs_per_batch"]
    lines += ["| class | calls per batch |", "|---|---|", "| `Metric` | %d |" % s["Metric"],
              "| `DeviceMetric` | %d |" % s["DeviceMetric"], "", "## Raw results", "", "```"]
    lines += [json.dumps(r) for r in results] + ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_loop.md"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--entropy", default="host")
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    for threads, entropy in SETTINGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--threads", str(threads), "--entropy", entropy,
               "--batches", str(args.batches), "--reps", str(args.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit("epoch_loop_profile: threads=%d entropy=%s passed its %d s limit; nothing more is started"
                             % (threads, entropy, CHILD_LIMIT))
        found = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not found:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("epoch_loop_profile: threads=%d entropy=%s ended with status %d; nothing more is started"
                             % (threads, entropy, p.returncode))
        results.append(json.loads(found[-1][len("RESULT "):]))
        print(found[-1], flush=True)
    text = report(results, args)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
