"""Measurements behind profiles/clip_loader.md (needs the MI355X; no fallback).

(i)  tbn_frames_to_tensor_batch against the per-clip loop of tbn_frames_to_tensor (+ torch.stack) on the same decoded
     frames and the same recorded geometries: B clips x n segments, 256x456 -> 224, RGB and Flow (win_length 5).
(ii) Video_Dataset.batch against the same batch assembled clip by clip from the existing parts (get_offsets, FrameReader,
     DevicePipeline.__call__, AudioSegments, torch.stack) for RGB + Flow + Audio, on a dataset synthesised in a temporary
     directory from the frame-sized files of tests/golden/jpeg_cases.npz, at threads = 8 and 16.

Both sides of a comparison run in one process, alternated repetition by repetition after warm-up; every timing is a host
clock round work that ends in a device synchronise; median and range are printed, and one JSON line at the end.

    python scripts/clip_loader_profile.py [--clips 32] [--segments 3] [--reps 15] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from attention_based_tbn_amd.config import load_config  # noqa: E402
from attention_based_tbn_amd.core.dataset import (AudioSegments, FrameReader, Video_Dataset, frame_span, get_offsets,  # noqa: E402
                                                  get_transforms)
from attention_based_tbn_amd.core.dataset.transform import _frames_to_tensor  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(a, b, warmup, reps):
    """-> (times of a, times of b) in ms, a and b alternated"""
    for _ in range(warmup):
        a()
        b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a)[0])
        tb.append(timed(b)[0])
    return ta, tb


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def launch_part(args, res):
    cfg = load_config([])
    tfs = get_transforms(cfg, ["RGB", "Flow"], "train")
    rng = np.random.RandomState(0)
    for m, c, per_clip in (("RGB", 3, args.segments), ("Flow", 1, args.segments * 10)):
        pipe = tfs[m]
        frames = torch.from_numpy(rng.randint(0, 256, (args.clips * per_clip, 256, 456, c)).astype(np.uint8)).cuda()
        np.random.seed(1)
        geos = pipe._record_batch([(256, 456)] * args.clips)
        mean, std = pipe._stats()
        clips = [list(range(args.clips))]

        def batched():
            return pipe._run_batch([frames], clips, geos)

        def per_clip_loop():
            return torch.stack([_frames_to_tensor(frames[b * per_clip:(b + 1) * per_clip], geos[b], c, pipe.stack, mean, std,
                                                  True, pipe.device) for b in range(args.clips)])
        assert torch.equal(batched(), per_clip_loop())
        tb, tl = alternate(batched, per_clip_loop, 5, args.reps * 2)
        res["launch_" + m] = dict(batched_ms=stats(tb), per_clip_ms=stats(tl), ratio=float(np.median(tl) / np.median(tb)),
                                  frames=int(frames.shape[0]), resized=sum(g.resized is not None for g in geos))
        print(m, json.dumps(res["launch_" + m]), flush=True)


def write_dataset(root, clips, rng):
    from tests import jpeg_ref as R
    vids = ["P%02d_01" % v for v in range(4)]
    os.makedirs(os.path.join(root, "audio"))
    for vid in vids:
        os.makedirs(os.path.join(root, "rgb", vid))
        os.makedirs(os.path.join(root, "flow", vid))
        for i in range(200):
            with open(os.path.join(root, "rgb", vid, "img_%010d.jpg" % i), "wb") as f:
                f.write(R.blob("big_256x456_420"))
            if i < 110:
                for axis in "xy":
                    with open(os.path.join(root, "flow", vid, "%s_%010d.jpg" % (axis, i)), "wb") as f:
                        f.write(R.blob("big_256x456_gray"))
        np.save(os.path.join(root, "audio", vid + ".npy"), (rng.rand(24000 * 8) * 2 - 1).astype(np.float32) * 0.3)
    rows = []
    with open(os.path.join(root, "ann.csv"), "w") as f:
        f.write("uid,video_id,start_timestamp,stop_timestamp,start_frame,stop_frame,verb_class,noun_class,action_class\n")
        for k in range(clips):
            a = int(rng.randint(1, 60))
            b = a + int(rng.randint(60, 130))
            rows.append((vids[k % 4], a, b))
            f.write('%d,%s,00:00:01.00,00:00:02.00,%d,%d,%d,%d,"1,2"\n' % (k, vids[k % 4], a, b, k % 125, k % 352))
    return vids, rows


def loader_part(args, res):
    rng = np.random.RandomState(3)
    modality = ["RGB", "Flow", "Audio"]
    with tempfile.TemporaryDirectory() as root:
        vids, rows = write_dataset(root, args.clips, rng)
        cfg = load_config(["data_dir=" + root, "data.rgb.dir_prefix=rgb", "data.flow.dir_prefix=flow",
                           "data.audio.dir_prefix=audio", "data.audio.read_audio_pickle=True", "data.sampling=async",
                           "model.attention.enable=False", "data.audio.audio_length=1.279",
                           "train.num_segments=%d" % args.segments])
        tfs = get_transforms(cfg, modality, "train")
        audio = AudioSegments.from_config(cfg)
        waves = {v: torch.from_numpy(np.load(os.path.join(root, "audio", v + ".npy"))).cuda() for v in vids}
        for threads in (8, 16):
            ds = Video_Dataset(cfg, vids, "ann.csv", modality, transform=tfs, mode="train", threads=threads)
            reader = FrameReader(root, "rgb", "flow", "jpg", threads=threads)
            order = list(range(args.clips))

            def batched():
                np.random.seed(5)
                return ds.batch(order)[0]

            def per_clip():
                np.random.seed(5)
                out = {m: [] for m in modality}
                for vid, a, b in rows:
                    first, num = frame_span(a, b)
                    for m in modality:
                        idx = get_offsets(first[m], num[m], m, "train", args.segments, 5 if m == "Flow" else 1)
                        if m == "RGB":
                            out[m].append(tfs[m](reader.read_rgb(vid, idx)))
                        elif m == "Flow":
                            fr = (idx.repeat(5) + np.tile(np.arange(5), args.segments)).astype(np.int64)
                            out[m].append(tfs[m](reader.read_flow(vid, fr)))
                        else:
                            out[m].append(audio([waves[vid]], idx[None])["Audio"][0])
                return {m: torch.stack(v) for m, v in out.items()}
            got, want = batched(), per_clip()
            assert all(torch.equal(got[m], want[m]) for m in modality)
            tb, tl = alternate(batched, per_clip, 3, args.reps)
            key = "loader_threads%d" % threads
            res[key] = dict(batched_ms=stats(tb), per_clip_ms=stats(tl), ratio=float(np.median(tl) / np.median(tb)),
                            batched_clips_per_s=args.clips / np.median(tb) * 1e3,
                            per_clip_clips_per_s=args.clips / np.median(tl) * 1e3)
            print(key, json.dumps(res[key]), flush=True)
            # where the batched call spends its time: the host half alone (files, parse, draws)
            tp = []
            for _ in range(args.reps):
                np.random.seed(5)
                t0 = time.perf_counter()
                ds.plan(order)
                tp.append((time.perf_counter() - t0) * 1e3)
            res[key]["plan_ms"] = stats(tp)
            print(key, "plan", json.dumps(res[key]["plan_ms"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_loader_profile: needs the MI355X")
    res = dict(clips=args.clips, segments=args.segments, reps=args.reps, device=torch.cuda.get_device_name(0))
    launch_part(args, res)
    loader_part(args, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
