"""Measures the PNG decode path for profiles/png_decode.md: one training step's worth of frames of config 4 (96 colour
frames and 960 gray flow planes of 456x256), written by an ordinary encoder with adaptive filters from smooth synthetic
images (Pillow; eight different images per kind, repeated).

    python scripts/png_decode_profile.py [--out FILE.json]

  files     the file sizes, and the bytes each mode copies to the device
  e2e       decode_pngs(inflate="host") and (inflate="device") alternated, host clock round a device synchronise, medians
  unfilter  tbn_png_unfilter alone between two device events, against a device-to-device copy of the same scanline bytes
  decode    tbn_png_decode (inflate + Adler-32 + unfilter) between two device events; the inflate and Adler launches are
            that minus the unfilter launch
  baseline  the reference's way, one full decode per file on 16 host threads: cv2.imread's decoder if cv2 imports, else
            Pillow (said in the output)
"""
import ctypes as C
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from attention_based_tbn_amd import _lib  # noqa: E402
from attention_based_tbn_amd.core.dataset import frames as F  # noqa: E402

N_COLOR, N_GRAY, THREADS, REPS, H, W = 96, 960, 16, 7, 256, 456


def smooth(seed, channels):
    """seeded sinusoids + a little noise: what an encoder's adaptive filters have something to choose on"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = []
    for _ in range(channels):
        a, b, c, d = rng.uniform(0.01, 0.06, 4)
        p = 128 + 60 * np.sin(a * x + b * y + rng.uniform(0, 6)) + 40 * np.cos(c * x - d * y) + rng.normal(0, 3, (H, W))
        planes.append(np.clip(p, 0, 255).astype(np.uint8))
    return np.stack(planes, 2)


def write_files(n, channels):
    from PIL import Image
    blobs, pixels = [], []
    for k in range(8):
        px = smooth(100 * channels + k, channels)
        buf = io.BytesIO()
        Image.fromarray(px[:, :, 0] if channels == 1 else px).save(buf, format="PNG")
        blobs.append(buf.getvalue())
        pixels.append(px)
    return [blobs[i % 8] for i in range(n)], [pixels[i % 8] for i in range(n)]


def median_ms(fn, reps=REPS):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def events_ms(fn, reps=20):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def baseline(blobs):
    try:
        import cv2
        name = "cv2.imdecode " + cv2.__version__

        def work(first):
            for i in range(first, len(blobs), THREADS):
                cv2.imdecode(np.frombuffer(blobs[i], np.uint8), cv2.IMREAD_UNCHANGED)
    except ImportError:
        import PIL
        from PIL import Image
        name = "Pillow " + PIL.__version__

        def work(first):
            for i in range(first, len(blobs), THREADS):
                np.asarray(Image.open(io.BytesIO(blobs[i])))
    with ThreadPoolExecutor(THREADS) as ex:
        times = []
        for _ in range(REPS):
            t = time.perf_counter()
            list(ex.map(work, range(THREADS)))
            times.append((time.perf_counter() - t) * 1e3)
    return name, statistics.median(times)


def device_launches(blobs, gray):
    """the launches alone, on data already on the device"""
    L = _lib.lib()
    n, ch = len(blobs), 1 if gray else 3
    geos = [F.png_geometry(b) for b in blobs]
    geo = geos[0]
    staging, pal_at = F._png_host_stage(L, blobs, geos, list(range(n)), THREADS)
    dev = staging.cuda()
    frames = torch.empty((n, H, W, ch), dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    raw_bytes = n * int(geo.raw_bytes)

    def unfilter():
        _lib.call("tbn_png_unfilter", _lib.ptr(dev), _lib.ptr(dev) + pal_at, n, C.byref(geo), ch, _lib.ptr(frames), _lib.ptr(status),
                  _lib.stream_ptr())

    copy_dst = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda")
    unfilter()
    assert status.tolist() == [0] * n
    out = {"unfilter_ms": events_ms(unfilter), "d2d_copy_ms": events_ms(lambda: copy_dst.copy_(dev[:raw_bytes])),
           "scanline_bytes": raw_bytes, "frame_bytes": n * H * W * ch}
    # the device mode's input: gathered streams, palettes, table
    slots = [(int(L.tbn_png_gather_bytes(g.idat_bytes)) + 15) // 16 * 16 for g in geos]
    offsets = np.concatenate([[0], np.cumsum(slots)]).tolist()
    total = offsets[-1]
    packed = np.zeros(total + n * 1024 + n * 24, np.uint8)
    table = (_lib.PngImage * n).from_address(packed.ctypes.data + total + n * 1024)
    b, e, a = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    for i in range(n):
        assert L.tbn_png_gather(blobs[i], len(blobs[i]), C.byref(geos[i]), packed.ctypes.data + offsets[i],
                                packed.ctypes.data + total + i * 1024, C.byref(b), C.byref(e), C.byref(a)) == 0
        table[i].in_off, table[i].in_len, table[i].adler, table[i].palette_off = offsets[i] + b.value, e.value - b.value, a.value, total + i * 1024
    d_in = torch.from_numpy(packed).cuda()
    ws = torch.empty(int(L.tbn_png_workspace_bytes(C.byref(geo), n)), dtype=torch.uint8, device="cuda")
    info = torch.empty(n, dtype=torch.int32, device="cuda")

    def decode():
        _lib.call("tbn_png_decode", _lib.ptr(d_in), total + n * 1024, _lib.ptr(d_in) + total + n * 1024, n, C.byref(geo), ch,
                  _lib.ptr(frames), _lib.ptr(ws), _lib.ptr(status), _lib.ptr(info), _lib.stream_ptr())

    decode()
    assert status.tolist() == [0] * n
    out["decode_ms"] = events_ms(decode, 7)
    out["inflate_and_adler_ms"] = out["decode_ms"] - out["unfilter_ms"]
    out["device_mode_input_bytes"] = int(packed.size)
    return out


def main():
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    out = {"box": torch.cuda.get_device_name(0), "threads": THREADS, "reps": REPS}
    import PIL
    out["encoder"] = "Pillow " + PIL.__version__ + " (adaptive filters, default compression)"
    for kind, n, channels, gray in (("colour", N_COLOR, 3, False), ("gray", N_GRAY, 1, True)):
        blobs, pixels = write_files(n, channels)
        row = {"frames": n, "file_bytes_min_max": [min(map(len, blobs)), max(map(len, blobs))], "file_bytes_total": sum(map(len, blobs))}
        want = np.stack([p if gray else p[:, :, ::-1] for p in pixels[:8]])
        for mode in ("host", "device"):
            got = F.decode_pngs(blobs[:8], gray=gray, inflate=mode, threads=THREADS).cpu().numpy()
            assert np.array_equal(got, want), (kind, mode)
        host, dev = [], []
        for _ in range(REPS):           # alternated: other people's work shares the host
            host.append(median_ms(lambda: F.decode_pngs(blobs, gray=gray, inflate="host", threads=THREADS), 1))
            dev.append(median_ms(lambda: F.decode_pngs(blobs, gray=gray, inflate="device", threads=THREADS), 1))
        row["e2e_host_ms"], row["e2e_device_ms"] = statistics.median(host), statistics.median(dev)
        row["e2e_host_ms_min_max"], row["e2e_device_ms_min_max"] = [min(host), max(host)], [min(dev), max(dev)]
        row["fallbacks"] = F.png_fallback_count()
        row.update(device_launches(blobs, gray))
        row["baseline"], row["baseline_16_threads_ms"] = baseline(blobs)
        out[kind] = row
    text = json.dumps(out, indent=1)
    print(text)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
