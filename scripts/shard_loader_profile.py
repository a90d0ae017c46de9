"""The `shard=` argument of `ClipLoader` at world size 1, measured (needs the MI355X; no fallback): the train loop of
`core.tools.train` over the dataset and model of scripts/epoch_loop_profile.py (config 4, B = 32, 8 decode threads, host
entropy decoding) through `ClipLoader(prefetch=2)` and through `ClipLoader(prefetch=2, shard=(0, 1))`, alternated epoch
by epoch in ONE process after two warm-up rounds.  The yardstick is arm (b) of profiles/epoch_loop.md, 40 - 41 ms per
batch: the sharded arm has to stay within that run-to-run spread.  One card, one rank: nothing here says anything about
the speed of several GPUs.

    python scripts/shard_loader_profile.py [--batches 12] [--reps 7] [--out profiles/epoch_loop.md]

The result replaces the section "## `shard=(0, 1)` against `shard=None`" at the end of --out (scripts/epoch_loop_profile.py
rewrites that file without it: run this script after it).
"""
import argparse
import json
import logging
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MODALITY = ["RGB", "Flow", "Audio"]
HEADING = "## `shard=(0, 1)` against `shard=None`"
BASELINE = (39.6, 43.2)         # arm (b) of the parent commit's profile at 8 threads, host entropy: min and max, ms per batch


def measure(args):
    import numpy as np
    import torch
    from clip_loader_profile import write_dataset
    from epoch_loop_profile import stats
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import Video_Dataset, get_transforms
    from attention_based_tbn_amd.core.models import build_model
    from attention_based_tbn_amd.core.tools import train
    from attention_based_tbn_amd.core.utils import ClipLoader, build_optimizer
    if not torch.cuda.is_available():
        raise SystemExit("shard_loader_profile: needs the MI355X")
    dev = torch.device("cuda")
    log = logging.getLogger("shard_loader_profile")
    log.setLevel(logging.WARNING)
    B, nb = 32, args.batches
    with tempfile.TemporaryDirectory() as root:
        vids, _ = write_dataset(root, B * nb, np.random.RandomState(3))
        cfg = load_config(["data_dir=" + root, "data.rgb.dir_prefix=rgb", "data.flow.dir_prefix=flow",
                           "data.audio.dir_prefix=audio", "data.audio.read_audio_pickle=True", "data.sampling=async",
                           "model.attention.enable=False", "data.audio.audio_length=1.279", "train.num_segments=3",
                           "train.batch_size=%d" % B])
        tfs = get_transforms(cfg, MODALITY, "train")
        ds = Video_Dataset(cfg, vids, "ann.csv", MODALITY, transform=tfs, mode="train", threads=8, entropy="host")
        torch.manual_seed(0)
        np.random.seed(0)
        model, criterion, _ = build_model(cfg, MODALITY, dev)
        optimizer, scheduler, _ = build_optimizer(cfg, model)
        loaders = dict(none=ClipLoader(ds, B, shuffle=True, prefetch=2),
                       shard01=ClipLoader(ds, B, shuffle=True, prefetch=2, shard=(0, 1)))

        def epoch(loader):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train(cfg, model, loader, optimizer, scheduler, criterion, 0, log, dev)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / nb

        # ONE side stream for both arms: a loader makes its own on first use, and which hardware queue a new stream lands
        # on can decide whether its work overlaps the step at all (a first run with a stream per loader had the loader
        # made second at the no-prefetch rate, 64.8 ms against 46.9 ms per batch) -- that is not what is compared here
        loaders["shard01"]._stream = loaders["none"]._loader_stream()[0]
        for _ in range(2):
            for loader in loaders.values():
                epoch(loader)
        times = {k: [] for k in loaders}
        for rep in range(args.reps):
            order = list(loaders) if rep % 2 == 0 else list(loaders)[::-1]       # A B, B A, ...: no arm is always second
            for k in order:
                times[k].append(epoch(loaders[k]))
        for loader in loaders.values():
            loader.close()
        return dict(batches=nb, reps=args.reps, clips=B, device=torch.cuda.get_device_name(0),
                    **{k: stats(v) for k, v in times.items()})


def section(r):
    def cell(s):
        return "%.1f (%.1f–%.1f)" % (s["median"], s["min"], s["max"])
    diff = r["shard01"]["median"] - r["none"]["median"]
    spread = r["none"]["max"] - r["none"]["min"]
    recorded = BASELINE[0] <= r["none"]["median"] <= BASELINE[1]
    return "\n".join([
        HEADING, "",
        "Written by `scripts/shard_loader_profile.py` on %s: the loop of arm (b) above (8 threads, host entropy," % r["device"],
        "`prefetch=2`, %d batches per epoch, %d repetitions per arm) through a loader made with `shard=None` and one made" % (r["batches"], r["reps"]),
        "with `shard=(0, 1)`, alternated in one process after two warm-up rounds.  Milliseconds per batch, median (min–max).",
        "One card and one rank: no multi-GPU speed is measured or claimed; RCCL with one GPU per rank has not been run.", "",
        "| `shard=None` | `shard=(0, 1)` | difference of the medians | spread of `shard=None` | slower by more than that spread |",
        "|---|---|---|---|---|",
        "| %s | %s | %+.2f | %.1f | %s |" % (cell(r["none"]), cell(r["shard01"]), diff, spread, "YES" if diff > spread else "no"), "",
        "Arm (b) as recorded above for the parent commit ran %.1f–%.1f ms; the unsharded arm of THIS run is %s that range," % (
            BASELINE[0], BASELINE[1], "inside" if recorded else "outside"),
        "so the comparison that counts is the one between the two arms of this run, on one machine in one process.", "",
        "```", json.dumps(r), "```", ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_loop.md"))
    args = ap.parse_args()
    res = measure(args)
    print("RESULT " + json.dumps(res), flush=True)
    text = open(args.out).read() if os.path.exists(args.out) else ""
    if HEADING in text:
        text = text[:text.index(HEADING)]
    with open(args.out, "w") as f:
        f.write(text.rstrip("\n") + "\n\n" + section(res))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
