#!/usr/bin/env python
"""Golden fixture for the multi-crop test pipeline: the UNMODIFIED reference classes of core/dataset/transform.py
(`Rescale`, `FixedCrop`, `Stack`, `ToTensor`, `Normalize`) composed the way core/tools/test.py:136-171 composes them,
on seeded uint8 frames.

cv2 is absent: the same stub as make_golden.py stands in, with `cv2.resize` = oracle.transform.resize_linear_u8 (the
restated OpenCV INTER_LINEAR), so the fixture pins the window arithmetic, the order of the crops and their mirror
images, Stack, ToTensor and Normalize -- not the interpolation, which stays parity unpinned as before.

Outputs: fixedcrop.npz (in<k>: frames, out<k>: the reference's fp32 tensor), fixedcrop.json (the cases).
Usage:   python tests/golden/make_golden_fixedcrop.py      (build container only)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_stubs  # noqa: E402
from make_golden_trainstep import ref_module  # noqa: E402

# statistics with a non-trivial division, so that Normalize's second operation is pinned as well
RGB_STAT = ([0.408, 0.459, 0.502], [0.229, 0.224, 0.225])
FLOW_STAT = ([0.5], [0.226])
CASES = [
    # 41x57 frames, crop 24: both margins (17, 33) are odd -> the centre's floor division
    {"name": "a_rgb_five", "modality": "RGB", "n_img": 3, "hw": [41, 57], "rescale": None, "size": 24,
     "locations": [0, 1, 2, 3, 4], "horizontal_flip": False},
    {"name": "b_rgb_ten", "modality": "RGB", "n_img": 3, "hw": [41, 57], "rescale": None, "size": 24,
     "locations": [0, 1, 2, 3, 4], "horizontal_flip": True},
    {"name": "c_flow_five", "modality": "Flow", "n_img": 20, "hw": [41, 57], "rescale": None, "size": 24,
     "locations": [0, 1, 2, 3, 4], "horizontal_flip": False},
    # 100 list entries -> 10 stacks that alternate plain and mirrored images
    {"name": "d_flow_ten", "modality": "Flow", "n_img": 10, "hw": [41, 57], "rescale": None, "size": 24,
     "locations": [0, 1, 2, 3, 4], "horizontal_flip": True},
    {"name": "e_rgb_rescale", "modality": "RGB", "n_img": 3, "hw": [41, 57], "rescale": 32, "size": 24,
     "locations": [4, 0], "horizontal_flip": False},
    # 40 rows: more than one 32-row tile per output plane
    {"name": "f_rgb_tall", "modality": "RGB", "n_img": 3, "hw": [41, 57], "rescale": None, "size": [40, 24],
     "locations": [0, 1, 2, 3, 4], "horizontal_flip": False},
]


def main():
    install_stubs()
    import cv2
    from oracle.transform import resize_linear_u8
    cv2.resize = lambda img, dsize, interpolation=None: resize_linear_u8(img, dsize[0], dsize[1])
    rt = ref_module("core/dataset/transform.py")
    rng = np.random.RandomState(31)
    out, meta = {}, {"cases": []}
    for k, case in enumerate(CASES):
        m = case["modality"]
        mean, std = RGB_STAT if m == "RGB" else FLOW_STAT
        h, w = case["hw"]
        frames = [rng.randint(0, 256, (h, w, 3) if m == "RGB" else (h, w)).astype(np.uint8)
                  for _ in range(case["n_img"])]
        size = case["size"] if isinstance(case["size"], int) else tuple(case["size"])
        chain = ([rt.Rescale(case["rescale"])] if case["rescale"] else []) + [
            rt.FixedCrop(size, locations=case["locations"], horizontal_flip=case["horizontal_flip"]),
            rt.Stack(m), rt.ToTensor(), rt.Normalize(mean, std)]
        x = [f.copy() for f in frames]
        for t in chain:                      # torchvision.transforms.Compose
            x = t(x)
        out["in%d" % k] = np.stack(frames, 0)
        out["out%d" % k] = x.numpy()
        meta["cases"].append(dict(case, mean=mean, std=std, shape=list(x.shape)))
    np.savez_compressed(os.path.join(HERE, "fixedcrop.npz"), **out)
    with open(os.path.join(HERE, "fixedcrop.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("fixedcrop.npz", len(CASES), "cases", [c["shape"] for c in meta["cases"]])


if __name__ == "__main__":
    main()
