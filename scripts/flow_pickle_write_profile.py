"""Writing flow pickles: `save_npz_arrays(deflate="device")` (csrc/deflate.hip) against np.savez_compressed on 16 host
threads, on 96 stacks of 256 x 456 x 10 (the batch of profiles/flow_pickle.md).  Needs the MI355X.

    python scripts/flow_pickle_write_profile.py [--stacks 96] [--reps 5] [--out FILE.json]

Prints one JSON object: wall time per batch of both paths (host clock around calls that end with the bytes on the host,
alternating, after a warm-up of both), the library's kernel timeline of the three launches (a run of its own),
the compressed sizes against zlib level 1 and level 6, and that every device-written file reads back equal.
The stacks are synthetic (smooth motion blobs on 128 plus noise, a JPEG round trip through PIL): seeded."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from attention_based_tbn_amd import _lib  # noqa: E402
from attention_based_tbn_amd.core.dataset.npz_file import npy_header, save_npz_arrays  # noqa: E402
from make_deflate_golden import flow_stack  # noqa: E402

H, W, C = 256, 456, 10
HOST_THREADS = 16
KINDS = 12          # distinct stacks; the batch cycles through them with a per-stack shift so that no two are equal


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


def host_savez(arrays):
    """the reference's way, 16 at a time: np.savez_compressed into memory"""
    def one(a):
        buf = io.BytesIO()
        np.savez_compressed(buf, flow=a)
        return buf.getvalue()
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        return list(ex.map(one, arrays))


def raw_deflate_size(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return len(c.compress(data) + c.flush())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=96)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_pickle_write_profile: needs the MI355X")
    rng = np.random.default_rng(11)
    kinds = [flow_stack(rng, H, W, C) for _ in range(KINDS)]
    host_arrays = [np.ascontiguousarray(np.roll(kinds[i % KINDS], i // KINDS, axis=1)) for i in range(args.stacks)]
    stacks = torch.from_numpy(np.stack(host_arrays)).cuda()
    n = args.stacks
    raw_bytes = n * (len(npy_header((H, W, C))) + H * W * C)
    res = dict(stacks=n, shape=[H, W, C], raw_MB=raw_bytes * 1e-6, host_threads=HOST_THREADS, reps=args.reps,
               device=torch.cuda.get_device_name(0), chunk=int(_lib.lib().tbn_deflate_chunk()))

    def device_path():
        return save_npz_arrays(stacks, deflate="device")

    def host_path():                       # the reference has the arrays on the host already: no copy is charged to it
        return host_savez(host_arrays)

    blobs = device_path()                  # warm-up of both, and the read-back check
    host_blobs = host_path()
    for b, a in zip(blobs, host_arrays):
        with np.load(io.BytesIO(b)) as z:
            assert np.array_equal(z["flow"], a)
    res["read_back_equal"] = True
    t = dict(device=[], host=[])
    for _ in range(args.reps):             # alternating: other people's work shares the host
        for name, fn in (("device", device_path), ("host", host_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    for name in t:
        res[name + "_ms"] = dict(median=statistics.median(t[name]), min=min(t[name]), max=max(t[name]))
        res[name + "_MB_per_s"] = raw_bytes * 1e-6 / (statistics.median(t[name]) * 1e-3)
    res["device_over_host_time"] = res["device_ms"]["median"] / res["host_ms"]["median"]
    res["kernels"] = kernel_times(device_path, 3)
    members = [npy_header((H, W, C)) + a.tobytes() for a in host_arrays[:KINDS]]
    ours = sum(len(b) for b in blobs[:KINDS])
    container = 30 + 8 + 46 + 8 + 22      # local header, central directory and end record around the stream (name: flow.npy)
    z1 = sum(raw_deflate_size(m, 1) for m in members)
    z6 = sum(raw_deflate_size(m, 6) for m in members)
    ours -= KINDS * container
    res["sizes"] = dict(raw=sum(map(len, members)), device=ours, zlib1=z1, zlib6=z6, device_over_raw=ours / sum(map(len, members)),
                        zlib6_over_raw=z6 / sum(map(len, members)), device_over_zlib1=ours / z1, device_over_zlib6=ours / z6,
                        savez_compressed_file=len(host_blobs[0]), device_file=len(blobs[0]))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
