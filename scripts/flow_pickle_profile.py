"""Measurements behind profiles/flow_pickle.md (needs the MI355X; no fallback).

A synthetic Flow-only dataset of frame_XXXXXXXXXX.npz pickles, each (256, 456, 10) uint8 written with
np.savez_compressed from the fixture's `big_256x456_gray` frame shifted ten ways (JPEG-like content), read with
data.flow.read_flow_pickle at B = clips x segments pickles per batch:

  (h) Video_Dataset.batch with flow_load="host"   -- np.load per pickle inside plan(), one H2D copy of the inflated batch
  (d) the same batch with flow_load="device"      -- npz_member per pickle, one H2D copy of the compressed bytes, one
                                                     tbn_inflate_batch call, one permute pass

Both arms run in one process, alternated repetition by repetition after warm-up; every timing is a host clock round work
that ends in a device synchronise; median and range are printed, and one JSON line at the end.  Also: the host half alone
(plan) of each arm, the two kernels' own times from the library timeline, and the bytes per batch.

    python scripts/flow_pickle_profile.py [--clips 32] [--segments 3] [--reps 9] [--out FILE]
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from attention_based_tbn_amd import _lib  # noqa: E402
from attention_based_tbn_amd.config import load_config  # noqa: E402
from attention_based_tbn_amd.core.dataset import Video_Dataset, get_transforms, npz_member  # noqa: E402

FILES = 110        # pickles per video
KINDS = 8          # distinct pickle contents


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def write_dataset(root, clips, rng):
    from tests import jpeg_ref as R
    frame = R.golden("big_256x456_gray", "gray")[:, :, 0]
    blobs = []
    for k in range(KINDS):
        # shifts large enough that the ten bytes of a pixel are unrelated, as the ten flow frames of a stack are: deflate
        # ratio about 3.6 (small shifts give 9 and more, and a stream that is nearly all matches)
        stack = np.stack([np.roll(frame, (17 * c + k, 29 * c + 2 * k), (0, 1)) for c in range(10)], 2)
        buf = io.BytesIO()
        np.savez_compressed(buf, flow=np.ascontiguousarray(stack))
        blobs.append(buf.getvalue())
    vids = ["P%02d_01" % v for v in range(4)]
    for v, vid in enumerate(vids):
        os.makedirs(os.path.join(root, "flow", vid))
        for i in range(FILES):
            with open(os.path.join(root, "flow", vid, "frame_%010d.npz" % i), "wb") as f:
                f.write(blobs[(i + 3 * v) % KINDS])
    with open(os.path.join(root, "ann.csv"), "w") as f:
        f.write("uid,video_id,start_timestamp,stop_timestamp,start_frame,stop_frame,verb_class,noun_class,action_class\n")
        for k in range(clips):
            a = int(rng.randint(1, 60))
            b = a + int(rng.randint(60, 130))
            f.write('%d,%s,00:00:01.00,00:00:02.00,%d,%d,%d,%d,"1,2"\n' % (k, vids[k % 4], a, b, k % 125, k % 352))
    return vids, blobs


def kernel_times(fn, reps):
    """the library's own kernels during `reps` calls of fn -> {kernel: median us}"""
    _lib.call("tbn_timeline_enable", 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    _lib.call("tbn_timeline_enable", 0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tl.csv")
        _lib.call("tbn_timeline_dump", path.encode())
        rows = [r.rsplit(",", 3) for r in open(path).read().splitlines()[1:]]
    times = {}
    for name, _, a, b in rows:
        times.setdefault(name.strip('"'), []).append((int(b) - int(a)) * 1e-3)
    return {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), launches=len(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_pickle_profile: needs the MI355X")
    res = dict(clips=args.clips, segments=args.segments, reps=args.reps, device=torch.cuda.get_device_name(0))
    rng = np.random.RandomState(3)
    with tempfile.TemporaryDirectory() as root:
        vids, blobs = write_dataset(root, args.clips, rng)
        records = [npz_member(b) for b in blobs]
        res["pickle"] = dict(shape=list(records[0].shape), inflated_bytes=int(np.mean([r.size for r in records])),
                             deflated_bytes=int(np.mean([r.data_length for r in records])),
                             ratio=float(np.mean([r.size / r.data_length for r in records])))
        n = args.clips * args.segments
        res["batch"] = dict(pickles=n, inflated_MB=n * res["pickle"]["inflated_bytes"] * 1e-6,
                            deflated_MB=n * res["pickle"]["deflated_bytes"] * 1e-6)
        print(json.dumps(res), flush=True)
        cfg = load_config(["data_dir=" + root, "data.flow.dir_prefix=flow", "data.flow.read_flow_pickle=True",
                           "data.sampling=async", "model.attention.enable=False", "train.num_segments=%d" % args.segments])
        tfs = get_transforms(cfg, ["Flow"], "train")
        ds = {mode: Video_Dataset(cfg, vids, "ann.csv", ["Flow"], transform=tfs, mode="train", flow_load=mode)
              for mode in ("host", "device")}
        order = list(range(args.clips))

        def arm(mode):
            def run():
                np.random.seed(5)
                return ds[mode].batch(order)[0]["Flow"]
            return run
        host, device = arm("host"), arm("device")
        assert torch.equal(host(), device()) and ds["device"].flow_fallbacks == 0
        for _ in range(2):
            host()
            device()
        th, td = [], []
        for _ in range(args.reps):
            th.append(timed(host)[0])
            td.append(timed(device)[0])
        res["batch_ms"] = dict(host=stats(th), device=stats(td), ratio=float(np.median(th) / np.median(td)),
                               device_wins_by_more_than_the_host_spread=bool(
                                   np.median(th) - np.median(td) > np.max(th) - np.min(th)))
        print("batch", json.dumps(res["batch_ms"]), flush=True)
        for mode in ("host", "device"):                 # the host half alone: files, np.load or npz_member, draws
            tp = []
            for _ in range(args.reps):
                np.random.seed(5)
                t0 = time.perf_counter()
                ds[mode].plan(order)
                tp.append((time.perf_counter() - t0) * 1e3)
            res["plan_ms_" + mode] = stats(tp)
            print("plan", mode, json.dumps(res["plan_ms_" + mode]), flush=True)
        res["kernels"] = kernel_times(device, 5)
        print("kernels", json.dumps(res["kernels"]), flush=True)
        assert ds["device"].flow_fallbacks == 0
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
