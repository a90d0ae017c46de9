"""Writes tests/golden/jpeg_sync_cases.npz: the JPEG byte strings the device entropy decoder (csrc/jpeg_entropy.hip) is
tested on beyond tests/golden/jpeg_cases.npz.  Bytes only: the expected values are the host stage's coefficients at
test time.

    python scripts/make_jpeg_sync_golden.py
    python scripts/make_jpeg_sync_golden.py --dump DIR     # writes the byte strings as DIR/NAME.jpg (no Pillow needed);
                                                           # input of scripts/jpeg_sync_check.cpp

Needs Pillow.  The images are the seeded synthetic ones of scripts/make_jpeg_golden.py (sinusoids plus noise, sd 12):

  camera_256x456_420_q90opt   colour, 4:2:0, q90, optimize=True (its own Huffman tables), no restarts: several hundred
                              subsequences, so the lanes span several wavefronts
  camera_256x456_gray_q60     gray, q60, no restarts
  uniform_256x456_gray_q75    every pixel 128: every block is the same few bits, nothing synchronises except through
                              the chain, so the rounds equal the lanes (the worst case)
  ri1_264x264_gray_q75        gray with a restart marker after every block: 1089 intervals, more than the lane limit,
                              so it takes the host stage
  ri8_264x264_gray_q75        the same pixels with a restart marker every 8 blocks (137 intervals: decoded on the
  plain_264x264_gray_q75      device, many intervals per image) and with none: same geometry, for mixed batches
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_jpeg_golden import ROOT, encode, synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_sync_cases.npz")


def dump(directory):
    os.makedirs(directory, exist_ok=True)
    with np.load(OUT) as z:
        for k in z.files:
            with open(os.path.join(directory, k), "wb") as f:
                f.write(z[k].tobytes())


def main():
    out = {}
    out["camera_256x456_420_q90opt.jpg"] = encode(synth(256, 456, 3, 5001, 12.0), subsampling=2, quality=90, optimize=True)
    out["camera_256x456_gray_q60.jpg"] = encode(synth(256, 456, 1, 5002, 12.0), quality=60)
    out["uniform_256x456_gray_q75.jpg"] = encode(np.full((256, 456), 128, np.uint8), quality=75)
    out["ri1_264x264_gray_q75.jpg"] = encode(synth(264, 264, 1, 5003, 12.0), quality=75, restart_marker_blocks=1)
    out["ri8_264x264_gray_q75.jpg"] = encode(synth(264, 264, 1, 5003, 12.0), quality=75, restart_marker_blocks=8)
    out["plain_264x264_gray_q75.jpg"] = encode(synth(264, 264, 1, 5003, 12.0), quality=75)
    np.savez_compressed(OUT, **{k: np.frombuffer(v, np.uint8) for k, v in out.items()})
    print(OUT, os.path.getsize(OUT), "bytes;", {k: len(v) for k, v in out.items()})
    assert os.path.getsize(OUT) < 256 * 1024


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
    else:
        main()
