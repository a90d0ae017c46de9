"""Writes tests/golden/jpeg_cases.npz: baseline JPEG byte strings and the pixels libjpeg-turbo decodes them to.

    python scripts/make_jpeg_golden.py
    python scripts/make_jpeg_golden.py --dump DIR     # writes the fixture's byte strings as DIR/NAME.jpg (no Pillow needed);
                                                      # input of scripts/jpeg_host_check.cpp

Needs Pillow (its bundled libjpeg-turbo is the reference: ISLOW IDCT, fancy upsampling, fixed-point colour -- what
cv2.imread gives the reference's dataset.py).  The tests that read the fixture do not need Pillow.

Per colour case NAME:  NAME.jpg (the bytes), NAME.bgr (H, W, 3: Pillow's RGB flipped, the order cv2.imread delivers),
NAME.luma (H, W: the luma-only decode, Image.draft("L", size) = cv2.imread(path, 0)).  Per gray case: NAME.jpg, NAME.gray.
`refuse_*` entries are files the decoder must refuse (bytes only).  Images are seeded synthetic: sinusoids plus noise,
scaled past [0, 255] before clipping, so that the AC terms and both clamping paths are live.
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")

SIZES = [(1, 1), (8, 8), (16, 16), (17, 31), (33, 47), (35, 50), (40, 56)]          # (H, W)
SAMPLINGS = {"444": 0, "422": 1, "420": 2}                                            # Pillow's `subsampling`
SETTINGS = {"q90": dict(quality=90),
            "q35r3opt": dict(quality=35, restart_marker_blocks=3, optimize=True),
            "q100r1": dict(quality=100, restart_marker_blocks=1)}
BATCH_QUALITIES = [20, 40, 55, 70, 80, 92, 98]
BIG = (256, 456)


def synth(h, w, channels, seed, noise):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(channels):
        fx, fy, ph = rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.9), rng.uniform(0, 6.28)
        v = 128 + 110 * np.sin(fx * x + ph) * np.cos(fy * y - ph) + 60 * np.sin(0.02 * (x + 1) * (y + 1) + c)
        v += rng.normal(0, noise, (h, w))
        planes.append(v)
    img = np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)
    return img if channels == 3 else img[:, :, 0]


def synth_big(channels, seed):
    h, w = BIG
    rng = np.random.default_rng(seed)
    tiles = rng.choice(np.array([0, 0, 255, 255, 30, 90, 128, 200, 240]), (h // 32, (w + 37) // 38, 3))
    img = np.repeat(np.repeat(tiles, 32, 0), 38, 1)[:, :w].astype(np.uint8)
    img[104:136] = synth(32, w, 3, seed + 1, 20.0)
    return img if channels == 3 else img[:, :, 0]


def encode(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def decode(blob, luma_only=False):
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    if luma_only:
        im.draft("L", im.size)
    return np.asarray(im)


def add_color(out, name, blob):
    out[name + ".jpg"] = np.frombuffer(blob, np.uint8)
    out[name + ".bgr"] = np.ascontiguousarray(decode(blob)[:, :, ::-1])
    out[name + ".luma"] = decode(blob, luma_only=True)


def add_gray(out, name, blob):
    out[name + ".jpg"] = np.frombuffer(blob, np.uint8)
    out[name + ".gray"] = decode(blob)


def dump(directory):
    os.makedirs(directory, exist_ok=True)
    with np.load(OUT) as z:
        for k in z.files:
            if k.endswith(".jpg"):
                with open(os.path.join(directory, k), "wb") as f:
                    f.write(z[k].tobytes())


def main():
    from PIL import Image
    out = {}
    seed = 1000
    for h, w in SIZES:
        for sname, sub in SAMPLINGS.items():
            for qname, kw in SETTINGS.items():
                seed += 1
                add_color(out, f"c_{h}x{w}_{sname}_{qname}", encode(synth(h, w, 3, seed, 12.0), subsampling=sub, **kw))
        seed += 1
        add_gray(out, f"g_{h}x{w}_q85r2", encode(synth(h, w, 1, seed, 12.0), quality=85, restart_marker_blocks=2))
    base = synth(40, 56, 3, 77, 25.0)
    for q in BATCH_QUALITIES:
        add_color(out, f"batch_40x56_420_q{q}", encode(base, subsampling=2, quality=q))
    # the two frame-sized files: flat tiles of random colours (0 and 255 among them) with one band of sinusoids and
    # noise, which keeps the stored pixels compressible
    add_color(out, "big_256x456_420", encode(synth_big(3, 4242), subsampling=2, quality=75))
    add_gray(out, "big_256x456_gray", encode(synth_big(1, 4243), quality=75, restart_marker_rows=4))
    # files the decoder refuses
    small = synth(16, 16, 3, 9, 25.0)
    out["refuse_progressive.jpg"] = np.frombuffer(encode(small, quality=80, progressive=True), np.uint8)
    buf = io.BytesIO()
    Image.fromarray(np.dstack([small, small[:, :, 0]]), "CMYK").save(buf, "JPEG", quality=80)
    out["refuse_cmyk.jpg"] = np.frombuffer(buf.getvalue(), np.uint8)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
    else:
        main()
