#!/usr/bin/env python
"""Generate tests/golden/bna_audio.npz and tests/golden/bna_keys.json by running the UNMODIFIED reference class
`BNInception_Audio` (reference core/models/bn_inception_audio.py) on the CPU.

The reference file is imported with importlib (it needs torch alone).  Every state-dict entry -- the separable stem
included -- is filled by oracle.fill.fill_state_dict from its key and shape, so a model with the same keys gets the same
weights.

  bna_keys.json   [[key, shape], ...] of the reference class's state dict, in its order
  bna_audio.npz   x = fp16-exact randn(2, 1, 96, 96); for mode in (eval, train): the output of pool1_3x3_s2, features, both
                  logits forms; after the train forward the running statistics of the two stem BatchNorms

Usage:  python tests/golden/make_golden_bna.py <path of the reference checkout>
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.fill import fill_state_dict  # noqa: E402

SEED = 9
STEM_BNS = ("conv1_1x3_s2_bn", "conv1_3x1_s2_bn")


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_bna", os.path.join(ref_root, "core/models/bn_inception_audio.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ref = mod.BNInception_Audio(num_classes=1000, attend=False)
    keys = [[k, list(v.shape)] for k, v in ref.state_dict().items()]
    with open(os.path.join(HERE, "bna_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    sd = fill_state_dict(ref.state_dict(), SEED)
    x = torch.randn(2, 1, 96, 96, generator=torch.Generator().manual_seed(SEED + 1)).half().float()
    res = {"seed": np.int64(SEED), "x": x.half().numpy()}
    for mode in ("eval", "train"):
        ref.load_state_dict(sd)
        ref.train(mode == "train")
        taps = {}
        hook = ref.pool1_3x3_s2.register_forward_hook(lambda m, i, o: taps.__setitem__("p1", o.detach().clone()))
        with torch.no_grad():
            feat = ref.features(x)
            ref.attend = True
            freq = ref.logits(feat)
            ref.attend = False
            glob = ref.logits(feat)
        hook.remove()
        res[mode + "_p1"] = taps["p1"].numpy()
        res[mode + "_feat"] = feat.numpy()
        res[mode + "_logits_freq"] = freq.numpy()
        res[mode + "_logits_global"] = glob.numpy()
    after = ref.state_dict()
    for bn in STEM_BNS:
        for stat in ("running_mean", "running_var"):
            res["train_%s.%s" % (bn, stat)] = after["%s.%s" % (bn, stat)].numpy()
        assert int(after[bn + ".num_batches_tracked"]) == 1
    np.savez_compressed(os.path.join(HERE, "bna_audio.npz"), **res)
    print({k: getattr(v, "shape", None) for k, v in res.items()})
    print("bna_audio.npz", os.path.getsize(os.path.join(HERE, "bna_audio.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
