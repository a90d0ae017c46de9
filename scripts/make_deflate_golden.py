"""Fixtures of the deflate encoder and the flow-pickle tool (data only: raw byte strings, recorded zlib sizes, JPEG bytes).

    python scripts/make_deflate_golden.py                 -> tests/golden/deflate_cases.npz, tests/golden/flow_frames.npz
    python scripts/make_deflate_golden.py --dump DIR      -> DIR/NAME.raw per case, for scripts/deflate_check.cpp

deflate_cases.npz: `names` (the cases in order), `raw_<name>` uint8 per case, `zlib1` / `zlib6`: bytes of the raw deflate
stream zlib writes at level 1 / 6 for the same bytes.  Sizes are in units of the encoder's chunk
(tbn_deflate_chunk(), read from the built library).  Seeded: a second run writes the same files.
flow_frames.npz: `u` and `v`, 9 JPEG files each (object arrays of bytes do not load without pickle, so: one uint8 array
`u_<i>` / `v_<i>` per file), 40 x 56 grayscale baseline, all distinct.  PIL is needed here only."""
import argparse
import io
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _jpeg_round_trip(plane, quality=90):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(plane, "L").save(buf, "JPEG", quality=quality)
    return buf.getvalue(), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("L"))


def _flow_plane(rng, H, W):
    """smooth motion blobs on 128, plus a little noise"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.full((H, W), 128.0)
    for _ in range(3):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 6, H / 2)
        f += rng.uniform(-40, 40) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    f += rng.normal(0, 0.7, (H, W))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def flow_stack(rng, H, W, C):
    return np.ascontiguousarray(np.stack([_jpeg_round_trip(_flow_plane(rng, H, W))[1] for _ in range(C)], axis=2))


def cases(chunk):
    rng = np.random.default_rng(20241)
    out = []
    out.append(("empty", np.zeros(0, np.uint8)))
    out.append(("one_byte", np.array([0x41], np.uint8)))
    text = np.frombuffer((b"the quick brown fox jumps over the lazy dog; " * 4000), np.uint8)
    mixed = np.where(rng.random(3 * chunk) < 0.5, text[:3 * chunk], rng.integers(0, 256, 3 * chunk)).astype(np.uint8)
    out.append(("chunk_minus_1", mixed[:chunk - 1].copy()))
    out.append(("chunk", mixed[:chunk].copy()))
    out.append(("chunk_plus_1", mixed[:chunk + 1].copy()))
    out.append(("two_chunks_17", mixed[:2 * chunk + 17].copy()))
    out.append(("zeros_1mib", np.zeros(1 << 20, np.uint8)))
    period = rng.integers(0, 256, 10).astype(np.uint8)
    out.append(("period_10", np.tile(period, 3 * chunk // 10 + 1)[:3 * chunk].copy()))
    out.append(("uniform_random", rng.integers(0, 256, 2 * chunk).astype(np.uint8)))
    # i.i.d., about 2 bits of entropy: P = 1/2, 1/4, 1/8, 1/16 x 2 over five arbitrary byte values
    values = np.array([0x80, 0x7F, 0x81, 0x13, 0xE0], np.uint8)
    out.append(("skewed", values[rng.choice(5, 2 * chunk, p=[0.5, 0.25, 0.125, 0.0625, 0.0625])]))
    out.append(("flow_stack", flow_stack(rng, 64, 96, 10).reshape(-1)))
    return out


def raw_deflate_size(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return len(c.compress(data) + c.flush())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="write NAME.raw per case into this directory instead of the fixtures")
    args = ap.parse_args()
    from attention_based_tbn_amd import _lib
    chunk = int(_lib.lib().tbn_deflate_chunk())
    cs = cases(chunk)
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for name, raw in cs:
            raw.tofile(os.path.join(args.dump, name + ".raw"))
        print(f"{len(cs)} cases in {args.dump}")
        return
    golden = os.path.join(ROOT, "tests", "golden")
    arrays = {"names": np.array([n for n, _ in cs]), "chunk": np.array(chunk),
              "zlib1": np.array([raw_deflate_size(r.tobytes(), 1) for _, r in cs], np.int64),
              "zlib6": np.array([raw_deflate_size(r.tobytes(), 6) for _, r in cs], np.int64)}
    for name, raw in cs:
        arrays["raw_" + name] = raw
    np.savez_compressed(os.path.join(golden, "deflate_cases.npz"), **arrays)
    rng = np.random.default_rng(77)
    frames = {}
    for k in "uv":
        for i in range(9):
            frames[f"{k}_{i}"] = np.frombuffer(_jpeg_round_trip(_flow_plane(rng, 40, 56))[0], np.uint8)
    assert len(set(v.tobytes() for v in frames.values())) == 18
    np.savez(os.path.join(golden, "flow_frames.npz"), **frames)
    for f in ("deflate_cases.npz", "flow_frames.npz"):
        print(f, os.path.getsize(os.path.join(golden, f)), "bytes")


if __name__ == "__main__":
    main()
