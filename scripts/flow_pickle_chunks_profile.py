"""Measurements behind profiles/flow_pickle_chunks.md (needs the MI355X; no fallback), by the method of
scripts/flow_pickle_profile.py.

The synthetic Flow-only dataset of that script -- frame_XXXXXXXXXX.npz pickles of (256, 456, 10) uint8 made from the
fixture's `big_256x456_gray` frame shifted ten ways -- written ONCE by `save_npz_arrays(chunk_index=True)`: device-written
streams (chunks of 32 KB compressed independently) that carry their chunk index.  B = clips x segments pickles per batch:

  (h) Video_Dataset.batch with flow_load="host"          -- np.load per pickle (np.load does not see the index)
  (d) load_npz_arrays(chunked=False)                     -- one wavefront per MEMBER: what the library did with these files
                                                            before it had a chunk reader
  (c) load_npz_arrays(chunked="auto")                    -- one wavefront per CHUNK (tbn_inflate_chunks)
  (D) / (C) Video_Dataset.batch with flow_load="device"  -- the batch round (d) and (c)

All arms run in one process, alternated repetition by repetition after warm-up; every timing is a host clock round work
that ends in a device synchronise.  Kernel times come from the library timeline.  `--variant-lib PATH` adds the chunk
kernel's time under another build of the library (the A/B build with per-symbol global stores: scripts/README.md), taken
in a child process that loads it.

    python scripts/flow_pickle_chunks_profile.py [--clips 32] [--segments 3] [--reps 9] [--out FILE] [--md FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
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
from attention_based_tbn_amd.core.dataset import dataset as dataset_module  # noqa: E402
from attention_based_tbn_amd.core.dataset import npz_file as F  # noqa: E402

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


def make_blobs():
    from tests import jpeg_ref as R
    frame = R.golden("big_256x456_gray", "gray")[:, :, 0]
    # the stacks of scripts/flow_pickle_profile.py: shifts large enough that the ten bytes of a pixel are unrelated
    stacks = np.stack([np.stack([np.roll(frame, (17 * c + k, 29 * c + 2 * k), (0, 1)) for c in range(10)], 2)
                       for k in range(KINDS)])
    arrays = torch.from_numpy(np.ascontiguousarray(stacks)).cuda()
    blobs = F.save_npz_arrays(arrays, chunk_index=True)
    plain = F.save_npz_arrays(arrays)
    for a, b in zip(blobs, plain):        # the index changes nothing in front of the central directory
        r = npz_member(a)
        assert a[:r.data_offset + r.data_length] == b[:r.data_offset + r.data_length] and F.npz_chunk_index(a) is not None
    return blobs


def write_dataset(root, clips, rng, blobs):
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
    return vids


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


def kernels_only(args):
    """the child of --variant-lib: the chunk reader's kernels over one batch, under whatever library TBN_LIB names"""
    blobs = make_blobs()
    batch = [blobs[i % KINDS] for i in range(args.clips * args.segments)]
    records = [npz_member(b) for b in batch]
    want, _ = F.load_npz_arrays(batch, records=records, chunked=False)
    got, statuses = F.load_npz_arrays(batch, records=records)
    assert torch.equal(got, want) and not any(statuses)
    for _ in range(2):
        F.load_npz_arrays(batch, records=records)
    print(json.dumps(kernel_times(lambda: F.load_npz_arrays(batch, records=records), 5)))


def ms(s, digits=1):
    return "%.*f (%.*f - %.*f)" % (digits, s["median"], digits, s["min"], digits, s["max"])


def us_ms(k, digits=2):
    return "%.*f (%.*f - %.*f)" % (digits, k["median_us"] * 1e-3, digits, k["min_us"] * 1e-3, digits, k["max_us"] * 1e-3)


def markdown(res):
    b, k = res["batch_ms"], res["kernels"]
    call = res["call_ms"]
    lines = [
        "# Flow pickles with a chunk index: one wavefront per chunk against one per member",
        "",
        "Written by `python scripts/flow_pickle_chunks_profile.py --md ...` from one run on one MI355X (the device reports",
        "itself as \"%s\").  The dataset of `profiles/flow_pickle.md` -- four videos of %d `frame_XXXXXXXXXX.npz` pickles, each"
        % (res["device"], FILES),
        "(256, 456, 10) `uint8`, eight distinct contents -- written once by `save_npz_arrays(chunk_index=True)`: device-written",
        "streams with their chunk index in the central directory.  B = %d clips x %d segments = %d pickles per batch."
        % (res["clips"], res["segments"], res["batch"]["pickles"]),
        "All arms in one process, alternated repetition by repetition after two warm-up rounds, %d repetitions; host clock"
        % res["reps"],
        "round work that ends in a device synchronise; milliseconds, median (minimum - maximum).  Files come from the page",
        "cache.  `torch.equal` results of all arms, `fallback_count()` unchanged and `chunked_count()` risen by the batch are",
        "asserted before anything is timed.",
        "",
        "| per pickle | |",
        "|---|---|",
        "| inflated (128-byte `.npy` header + array) | %d B, %d chunks of 32 768 B |" % (res["pickle"]["inflated_bytes"], res["pickle"]["chunks"]),
        "| deflated by `tbn_deflate_batch_indexed` | %d B (ratio %.2f) |" % (res["pickle"]["deflated_bytes"], res["pickle"]["ratio"]),
        "| the index | %d B of extra field in the central directory |" % res["pickle"]["index_bytes"],
        "",
        "| arm | what is timed | ms |",
        "|---|---|---|",
        "| (h) `Video_Dataset.batch`, `flow_load=\"host\"` | `np.load` + transpose per pickle, upload, one transform launch | %s |" % ms(b["host"]),
        "| (D) `Video_Dataset.batch`, `flow_load=\"device\"`, `chunked=False` | the batch round (d) | %s |" % ms(b["device_whole"]),
        "| (C) `Video_Dataset.batch`, `flow_load=\"device\"` | the batch round (c): what the dataset does | %s |" % ms(b["device_chunked"]),
        "| (d) `load_npz_arrays(chunked=False)` | one upload, `tbn_inflate_batch`, one permute pass, the status copy | %s |" % ms(call["whole"]),
        "| (c) `load_npz_arrays(chunked=\"auto\")` | `npz_chunk_index` per file, one upload, `tbn_inflate_chunks`, permute, status copy | %s |" % ms(call["chunked"]),
        "| `npz_chunk_index` over the batch | host only: the central directory walk | %s |" % ms(res["index_ms"], 2),
        "| `inflate_kernel` alone | library timeline, %d workgroups of one wavefront | %s |" % (res["batch"]["pickles"], us_ms(k["inflate_kernel"])),
        "| `inflate_chunk_kernel` alone | library timeline, %d workgroups of one wavefront, %d B of LDS | %s |"
        % (res["batch"]["chunks"], res["lds_bytes"], us_ms(k["inflate_chunk_kernel"])),
        "| `inflate_fold_kernel` alone | one wavefront per member | %s |" % us_ms(k["inflate_fold_kernel"], 3),
        "| `inflate_crc_kernel` alone | both paths | %s |" % us_ms(k["inflate_crc_kernel"]),
    ]
    if res.get("variant_kernels"):
        lines.append("| `inflate_chunk_kernel`, A/B build with per-symbol global stores | the same batch, a child process with that library | %s |"
                     % us_ms(res["variant_kernels"]["inflate_chunk_kernel"]))
    gain = call["whole"]["median"] - call["chunked"]["median"]
    spread = call["whole"]["max"] - call["whole"]["min"]
    lines += [
        "",
        "The claim that was to be checked: (c) is faster than (d) by more than (d)'s own min-max spread.  %s: %.1f ms against"
        % ("It is" if res["chunked_wins"] else "It is NOT", gain),
        "a spread of %.1f ms, a factor of %.2f on the call and %.1f on the inflate launch." % (
            spread, call["whole"]["median"] / call["chunked"]["median"],
            k["inflate_kernel"]["median_us"] / k["inflate_chunk_kernel"]["median_us"]),
    ]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_pickle_chunks_profile: needs the MI355X")
    if args.kernels_only:
        return kernels_only(args)
    res = dict(clips=args.clips, segments=args.segments, reps=args.reps, device=torch.cuda.get_device_name(0), lds_bytes=39104)
    rng = np.random.RandomState(3)
    with tempfile.TemporaryDirectory() as root:
        blobs = make_blobs()
        vids = write_dataset(root, args.clips, rng, blobs)
        records = [npz_member(b) for b in blobs]
        index = [F.npz_chunk_index(b) for b in blobs]
        n = args.clips * args.segments
        res["pickle"] = dict(shape=list(records[0].shape), inflated_bytes=int(np.mean([r.size for r in records])),
                             deflated_bytes=int(np.mean([r.data_length for r in records])),
                             ratio=float(np.mean([r.size / r.data_length for r in records])), chunks=len(index[0]),
                             index_bytes=4 + 12 + 4 * len(index[0]))
        res["batch"] = dict(pickles=n, chunks=n * len(index[0]), inflated_MB=n * res["pickle"]["inflated_bytes"] * 1e-6,
                            deflated_MB=n * res["pickle"]["deflated_bytes"] * 1e-6)
        print(json.dumps(res), flush=True)
        cfg = load_config(["data_dir=" + root, "data.flow.dir_prefix=flow", "data.flow.read_flow_pickle=True",
                           "data.sampling=async", "model.attention.enable=False", "train.num_segments=%d" % args.segments])
        tfs = get_transforms(cfg, ["Flow"], "train")
        ds = {mode: Video_Dataset(cfg, vids, "ann.csv", ["Flow"], transform=tfs, mode="train", flow_load=mode)
              for mode in ("host", "device")}
        order = list(range(args.clips))
        auto = F.load_npz_arrays

        def whole_only(*a, **kw):
            return auto(*a, chunked=False, **kw)

        def arm(mode, loader=auto):
            def run():
                np.random.seed(5)
                dataset_module.load_npz_arrays = loader         # the one call the dataset makes per batch
                try:
                    return ds[mode].batch(order)[0]["Flow"]
                finally:
                    dataset_module.load_npz_arrays = auto
            return run
        host, dev_whole, dev_chunked = arm("host"), arm("device", whole_only), arm("device")
        batch = [blobs[i % KINDS] for i in range(n)]
        brecords = [records[i % KINDS] for i in range(n)]

        def call_whole():
            return F.load_npz_arrays(batch, records=brecords, planes=True, chunked=False)[0]

        def call_chunked():
            return F.load_npz_arrays(batch, records=brecords, planes=True)[0]
        before = (F.fallback_count(), F.chunked_count())
        want = host()
        assert torch.equal(want, dev_whole()) and F.chunked_count() == before[1]
        assert torch.equal(want, dev_chunked()) and F.chunked_count() == before[1] + n
        assert torch.equal(call_whole(), call_chunked())
        assert F.fallback_count() == before[0] and ds["device"].flow_fallbacks == 0
        arms = dict(host=host, device_whole=dev_whole, device_chunked=dev_chunked, whole=call_whole, chunked=call_chunked)
        for _ in range(2):
            for fn in arms.values():
                fn()
        t = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                t[k].append(timed(fn)[0])
        res["batch_ms"] = {k: stats(t[k]) for k in ("host", "device_whole", "device_chunked")}
        res["call_ms"] = {k: stats(t[k]) for k in ("whole", "chunked")}
        res["chunked_wins"] = bool(np.median(t["whole"]) - np.median(t["chunked"]) > np.max(t["whole"]) - np.min(t["whole"]))
        print("batch", json.dumps(res["batch_ms"]), flush=True)
        print("call", json.dumps(res["call_ms"]), res["chunked_wins"], flush=True)
        ti = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for b in batch:
                F.npz_chunk_index(b)
            ti.append((time.perf_counter() - t0) * 1e3)
        res["index_ms"] = stats(ti)
        res["kernels"] = kernel_times(lambda: (call_whole(), call_chunked()), 5)
        print("kernels", json.dumps(res["kernels"]), flush=True)
        assert F.fallback_count() == before[0]
    if args.variant_lib:
        env = dict(os.environ, TBN_LIB=args.variant_lib)
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--clips", str(args.clips),
                                "--segments", str(args.segments)], env=env, capture_output=True, text=True, timeout=300)
        if child.returncode != 0:
            raise SystemExit("the --variant-lib child failed:\n" + child.stdout + child.stderr)
        res["variant_kernels"] = json.loads(child.stdout.strip().splitlines()[-1])
        print("variant", json.dumps(res["variant_kernels"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
