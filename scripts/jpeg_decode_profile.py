"""Measures the JPEG decode path for profiles/jpeg_decode.md: one training step's worth of frames of config 4
(96 colour + 960 gray frames of 456x256, the two frame-sized files of tests/golden/jpeg_cases.npz repeated).

    python scripts/jpeg_decode_profile.py [--out FILE.json]
    python scripts/jpeg_decode_profile.py --device-entropy [--out FILE.json]     # the opt-in device Huffman decoder only

  host    tbn_jpeg_entropy_decode per frame on one thread, and the whole batch on 16 threads
  pillow  libjpeg-turbo's full decode of the same bytes on the same host (the baseline being replaced), if Pillow imports
  kernels per-launch device time of the two kernels from the library's own timeline (events on the dispatch packets),
          with the bytes each moves by its algorithm
  e2e     decode_jpegs (parse + entropy decode + copy + kernels), host clock round a device synchronise

--device-entropy (camera-sized files, eight different ones per kind so that the rounds vary):
  pack    tbn_jpeg_scan_pack of the whole batch on 1, 4 and 16 threads, against tbn_jpeg_entropy_decode the same way
  kernel  jpeg_entropy_kernel per launch from the library's timeline at S = 512, 1024, 2048; the whole call (the
          hipMemsetAsync of the coefficients included) between two device events; lanes and rounds from `info`
  e2e     decode_jpegs(entropy="host") and (entropy="device") alternated, 1, 4 and 16 threads, medians; the bytes each
          copies to the device; the frames of the two compared
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


def camera_files(kinds=8):
    """`kinds` different camera-sized files per kind: dense_frames' recipe with other seeds (the first is its file)"""
    from PIL import Image
    y, x = np.mgrid[0:256, 0:456].astype(np.float64)
    color, gray = [], []
    for k in range(kinds):
        rng = np.random.default_rng(7 + k)
        img = np.stack([128 + 90 * np.sin(0.05 * (c + 1 + 0.3 * k) * x + c) * np.cos(0.07 * y - c - k) + rng.normal(0, 9.0, (256, 456))
                        for c in range(3)], -1)
        img = np.clip(img, 0, 255).astype(np.uint8)
        for arr, kw, out in ((img, dict(quality=90, subsampling=2), color), (img[:, :, 0], dict(quality=60), gray)):
            buf = io.BytesIO()
            Image.fromarray(arr).save(buf, "JPEG", **kw)
            out.append(buf.getvalue())
    return color, gray


def pack_stage(blobs):
    """the pack stage and the host stage on the same blobs, whole batch on 1, 4 and 16 threads -> ms"""
    L = _lib.lib()
    n = len(blobs)
    geo = _lib.JpegGeometry()
    assert L.tbn_jpeg_parse(blobs[0], len(blobs[0]), C.byref(geo)) == 0
    caps = [int(L.tbn_jpeg_scan_pack_bytes(len(b), 1)) for b in blobs]
    offs = np.concatenate([[0], np.cumsum(caps)])
    rec = np.empty(int(offs[-1]) + 16, np.uint8)
    base = rec.ctypes.data + (-rec.ctypes.data % 16)
    coef = np.empty((n, int(geo.coef_count)), np.int16)
    quant = np.empty((n, geo.components, 64), np.uint16)
    used_total = [0]

    def pack(first, threads):
        count, used, tot = C.c_int(0), C.c_size_t(0), 0
        for i in range(first, n, threads):
            assert L.tbn_jpeg_scan_pack(blobs[i], len(blobs[i]), C.byref(geo), base + int(offs[i]), caps[i], 1024,
                                        quant[i].ctypes.data, C.byref(count), C.byref(used)) == 0 and used.value
            tot += used.value
        return tot

    def host(first, threads):
        for i in range(first, n, threads):
            assert L.tbn_jpeg_entropy_decode(blobs[i], len(blobs[i]), C.byref(geo), coef[i].ctypes.data, quant[i].ctypes.data) == 0
        return 0

    out = {}
    for threads in (1, 4, 16):
        with ThreadPoolExecutor(threads) as ex:
            for name, fn in (("pack", pack), ("host_entropy", host)):
                ts = []
                for _ in range(REPS + 1):
                    t = time.perf_counter()
                    tot = sum(ex.map(lambda first: fn(first, threads), range(threads)))
                    ts.append(time.perf_counter() - t)
                    if name == "pack":
                        used_total[0] = tot
                out["%s_ms_%d_threads" % (name, threads)] = statistics.median(ts[1:]) * 1e3
    out["record_bytes_per_frame"] = used_total[0] / n
    out["file_bytes_per_frame"] = sum(len(b) for b in blobs) / n
    return geo, rec, base, offs, out


def entropy_kernel_stage(geo, rec, base, offs, n):
    L = _lib.lib()
    dev = torch.device("cuda")
    lead = base - rec.ctypes.data
    total = int(offs[-1])
    packed = torch.from_numpy(rec[lead:lead + total]).to(dev)
    offsets = torch.from_numpy(offs[:-1].astype(np.uint32).view(np.int32)).to(dev)
    coef = torch.empty(n * int(geo.coef_count), dtype=torch.int16, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty((n, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.tbn_jpeg_entropy_workspace_bytes(C.byref(geo), n)), dtype=torch.uint8, device=dev)
    out = {}
    for S in (512, 1024, 2048):
        args = (_lib.ptr(packed), total, _lib.ptr(offsets), n, C.byref(geo), S, _lib.ptr(coef), _lib.ptr(status),
                _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
        for _ in range(3):
            _lib.call("tbn_jpeg_entropy_decode_dev", *args)
        torch.cuda.synchronize()
        assert not status.any().item()
        calls = []
        for _ in range(20):                     # the whole call, its memset included: device events
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.call("tbn_jpeg_entropy_decode_dev", *args)
            b.record()
            b.synchronize()
            calls.append(a.elapsed_time(b) * 1e3)
        _lib.call("tbn_timeline_enable", 1)
        for _ in range(20):
            _lib.call("tbn_jpeg_entropy_decode_dev", *args)
        torch.cuda.synchronize()
        _lib.call("tbn_timeline_enable", 0)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "tl.csv")
            _lib.call("tbn_timeline_dump", path.encode())
            rows = [r.rsplit(",", 3) for r in open(path).read().splitlines()[1:]]
        ts = [(int(b) - int(a)) * 1e-3 for name, _, a, b in rows if "entropy" in name]
        lanes, rounds = info[:, 0].cpu().numpy(), info[:, 1].cpu().numpy()
        words = ws.cpu().numpy().view(np.uint32).reshape(n, 4)
        out["S%d" % S] = {"kernel_us_per_launch": statistics.median(ts), "kernel_us_per_frame": statistics.median(ts) / n,
                          "launches_timed": len(ts), "call_with_memset_us": statistics.median(calls),
                          "S_used_min_max": [int(words[:, 0].min()), int(words[:, 0].max())],
                          "scan_in_lds_frames": int(words[:, 3].sum()),
                          "lanes_min_median_max": [int(lanes.min()), float(np.median(lanes)), int(lanes.max())],
                          "rounds_min_median_max": [int(rounds.min()), float(np.median(rounds)), int(rounds.max())]}
    return out


def entropy_e2e_stage(blobs, gray, geo):
    n = len(blobs)
    same = torch.equal(decode_jpegs(blobs, gray=gray, entropy="device"), decode_jpegs(blobs, gray=gray, entropy="host"))
    out = {"frames_identical": bool(same)}
    for threads in (1, 4, 16):
        ts = {"host": [], "device": []}
        for rep in range(REPS + 2):              # alternated; the first two rounds warm up
            for mode in ("host", "device"):
                torch.cuda.synchronize()
                t = time.perf_counter()
                decode_jpegs(blobs, gray=gray, threads=threads, entropy=mode)
                torch.cuda.synchronize()
                if rep >= 2:
                    ts[mode].append(time.perf_counter() - t)
        h, d = statistics.median(ts["host"]) * 1e3, statistics.median(ts["device"]) * 1e3
        out["%d_threads" % threads] = {"host_ms": h, "device_ms": d, "host_over_device": h / d,
                                       "host_ms_min_max": [min(ts["host"]) * 1e3, max(ts["host"]) * 1e3],
                                       "device_ms_min_max": [min(ts["device"]) * 1e3, max(ts["device"]) * 1e3]}
    L = _lib.lib()
    out["h2d_bytes_per_frame_host"] = int(geo.coef_count) * 2 + geo.components * 128
    out["h2d_bytes_per_frame_device"] = sum(int(L.tbn_jpeg_scan_pack_bytes(len(b), 1)) for b in blobs) / n + 4 + geo.components * 128
    return out


def device_entropy_main():
    assert torch.cuda.is_available(), "needs the MI355X"
    color, gray = camera_files()
    res = {"frames": {"color": N_COLOR, "gray": N_GRAY, "size": "456x256"}, "device": torch.cuda.get_device_name(0),
           "distinct_files_per_kind": len(color)}
    for kind, files, n, is_gray in (("color", color, N_COLOR, False), ("gray", gray, N_GRAY, True)):
        blobs = [files[i % len(files)] for i in range(n)]
        geo, rec, base, offs, pack = pack_stage(blobs)
        res[kind] = {"pack": pack, "kernel": entropy_kernel_stage(geo, rec, base, offs, n),
                     "decode_jpegs": entropy_e2e_stage(blobs, is_gray, geo)}
    text = json.dumps(res, indent=1)
    print(text)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")


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
    if "--device-entropy" in sys.argv:
        device_entropy_main()
    else:
        main()
