"""Measures the JPEG decode path for profiles/jpeg_decode.md: one training step's worth of frames of config 4
(96 colour + 960 gray frames of 456x256, the two frame-sized files of tests/golden/jpeg_cases.npz repeated).

    python scripts/jpeg_decode_profile.py [--out FILE.json]

  host    tbn_jpeg_entropy_decode per frame on one thread, and the whole batch on 16 threads
  pillow  libjpeg-turbo's full decode of the same bytes on the same host (the baseline being replaced), if Pillow imports
  kernels per-launch device time of the two kernels from the library's own timeline (events on the dispatch packets),
          with the bytes each moves by its algorithm
  e2e     decode_jpegs (parse + entropy decode + copy + kernels), host clock round a device synchronise
"""
import ctypes as C
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from attention_based_tbn_amd import _lib  # noqa: E402
from attention_based_tbn_amd.core.dataset import decode_jpegs  # noqa: E402

N_COLOR, N_GRAY, THREADS, REPS = 96, 960, 16, 7


def host_stage(blob, n):
    L = _lib.lib()
    geo = _lib.JpegGeometry()
    assert L.tbn_jpeg_parse(blob, len(blob), C.byref(geo)) == 0
    coef = np.empty((n, int(geo.coef_count)), np.int16)
    quant = np.empty((n, geo.components, 64), np.uint16)

    def work(i):
        rc = L.tbn_jpeg_entropy_decode(blob, len(blob), C.byref(geo), coef[i].ctypes.data, quant[i].ctypes.data)
        assert rc == 0

    one = []
    for _ in range(REPS):
        t = time.perf_counter()
        for i in range(min(n, 96)):
            work(i)
        one.append((time.perf_counter() - t) / min(n, 96))
    many = []
    with ThreadPoolExecutor(THREADS) as ex:      # one task per thread (images first, first + THREADS, ...), as decode_jpegs
        for _ in range(REPS):
            t = time.perf_counter()
            list(ex.map(lambda first: [work(i) for i in range(first, n, THREADS)], range(THREADS)))
            many.append(time.perf_counter() - t)
    return geo, coef, quant, {"us_per_frame_1_thread": statistics.median(one) * 1e6,
                              "ms_batch_16_threads": statistics.median(many) * 1e3,
                              "us_per_frame_16_threads": statistics.median(many) / n * 1e6}


def pillow_stage(blob, n, gray):
    try:
        from PIL import Image
    except ImportError:
        return None

    def work(_):
        im = Image.open(io.BytesIO(blob))
        if gray:
            im.draft("L", im.size)
        return np.asarray(im).shape

    one = []
    for _ in range(REPS):
        t = time.perf_counter()
        for i in range(min(n, 96)):
            work(i)
        one.append((time.perf_counter() - t) / min(n, 96))
    many = []
    with ThreadPoolExecutor(THREADS) as ex:      # one task per thread (images first, first + THREADS, ...), as decode_jpegs
        for _ in range(REPS):
            t = time.perf_counter()
            list(ex.map(lambda first: [work(i) for i in range(first, n, THREADS)], range(THREADS)))
            many.append(time.perf_counter() - t)
    return {"us_per_frame_1_thread": statistics.median(one) * 1e6, "ms_batch_16_threads": statistics.median(many) * 1e3,
            "us_per_frame_16_threads": statistics.median(many) / n * 1e6}


def kernel_stage(geo, coef, quant, channels):
    L = _lib.lib()
    n = coef.shape[0]
    dev = torch.device("cuda")
    coef_d = torch.from_numpy(coef).to(dev)
    quant_d = torch.from_numpy(quant.view(np.int16)).to(dev)
    frames = torch.empty((n, geo.height, geo.width, channels), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(L.tbn_jpeg_workspace_bytes(C.byref(geo), n)), dtype=torch.uint8, device=dev)
    args = (_lib.ptr(coef_d), _lib.ptr(quant_d), n, C.byref(geo), channels, _lib.ptr(frames), _lib.ptr(ws), _lib.stream_ptr())
    for _ in range(3):
        _lib.call("tbn_jpeg_reconstruct", *args)
    torch.cuda.synchronize()
    _lib.call("tbn_timeline_enable", 1)
    for _ in range(20):
        _lib.call("tbn_jpeg_reconstruct", *args)
    torch.cuda.synchronize()
    _lib.call("tbn_timeline_enable", 0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tl.csv")
        _lib.call("tbn_timeline_dump", path.encode())
        rows = [r.rsplit(",", 3) for r in open(path).read().splitlines()[1:]]
    times = {}
    for name, _, a, b in rows:
        times.setdefault("idct" if "idct" in name else "color", []).append((int(b) - int(a)) * 1e-9)
    planes = 1 if channels == 1 else geo.components
    samples = sum(64 * geo.blocks_w[c] * geo.blocks_h[c] for c in range(planes))
    bytes_a = n * (3 * samples + 128 * planes)                            # int16 in, uint8 out, the quantiser rows
    true = geo.width * geo.height
    chroma = 0 if planes == 1 else 2 * (-(-geo.width // geo.hsamp[0])) * (-(-geo.height // geo.vsamp[0]))
    bytes_b = n * (true + chroma + true * channels)                       # planes read once, frames written
    out = {}
    for k, nbytes in (("idct", bytes_a), ("color", bytes_b)):
        t = statistics.median(times[k])
        out[k] = {"us_per_launch": t * 1e6, "us_per_frame": t / n * 1e6, "bytes": nbytes, "GB_per_s": nbytes / t * 1e-9,
                  "launches_timed": len(times[k])}
    return out


def e2e_stage(blob, n, gray):
    blobs = [blob] * n
    for _ in range(2):
        decode_jpegs(blobs, gray=gray, threads=THREADS)
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        decode_jpegs(blobs, gray=gray, threads=THREADS)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return {"ms_batch": statistics.median(ts) * 1e3, "us_per_frame": statistics.median(ts) / n * 1e6}


def dense_frames():
    """456x256 files of the size real video frames have (about 42 KB colour 4:2:0, 14 KB gray), if Pillow imports: the
    fixture's two frame-sized files are mostly flat tiles and entropy-decode faster than a camera frame"""
    try:
        from PIL import Image
    except ImportError:
        return None
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:256, 0:456].astype(np.float64)
    img = np.stack([128 + 90 * np.sin(0.05 * (c + 1) * x + c) * np.cos(0.07 * y - c) + rng.normal(0, 9.0, (256, 456))
                    for c in range(3)], -1)
    img = np.clip(img, 0, 255).astype(np.uint8)
    out = []
    for arr, kw in ((img, dict(quality=90, subsampling=2)), (img[:, :, 0], dict(quality=60))):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "JPEG", **kw)
        out.append(buf.getvalue())
    return out


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    with np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")) as z:
        color, gray = z["big_256x456_420.jpg"].tobytes(), z["big_256x456_gray.jpg"].tobytes()
    dense = dense_frames()
    res = {"frames": {"color": N_COLOR, "gray": N_GRAY, "size": "456x256"}, "threads": THREADS,
           "file_bytes": {"color": len(color), "gray": len(gray)}, "device": torch.cuda.get_device_name(0)}
    for kind, blob, n, is_gray in (("color", color, N_COLOR, False), ("gray", gray, N_GRAY, True)):
        geo, coef, quant, host = host_stage(blob, n)
        res[kind] = {"host_entropy": host, "pillow_full_decode": pillow_stage(blob, n, is_gray),
                     "kernels": kernel_stage(geo, coef, quant, 1 if is_gray else 3), "decode_jpegs": e2e_stage(blob, n, is_gray)}
    if dense is not None:
        res["dense_file_bytes"] = {"color": len(dense[0]), "gray": len(dense[1])}
        for kind, blob, n, is_gray in (("dense_color", dense[0], N_COLOR, False), ("dense_gray", dense[1], N_GRAY, True)):
            geo, coef, quant, host = host_stage(blob, n)
            res[kind] = {"host_entropy": host, "pillow_full_decode": pillow_stage(blob, n, is_gray),
                         "kernels": kernel_stage(geo, coef, quant, 1 if is_gray else 3),
                         "decode_jpegs": e2e_stage(blob, n, is_gray)}
    text = json.dumps(res, indent=1)
    print(text)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
