#!/usr/bin/env python
"""Generate tests/golden/vis_info.{npz,json} by running the UNMODIFIED reference's `get_info` (core/tools/vis.py:30-93).

Runs only where make_golden.py runs (it needs the reference checkout).  The reference's modules are imported as they are; beside the
stubs of make_golden.py (cv2, torchvision, librosa, pretrainedmodels) the packages the visualiser imports but the image
lacks are stand-ins in sys.modules: qgrid (`show_grid` hands the DataFrame back), moviepy.editor, omegaconf and
tensorboardX.  A fake model (seeded logits and attention weights per clip) and a fake dataset are fed to it, on the CPU.

  vis_info.npz   verb (N, 7), noun (N, 11) logits, weights (N * 3, 8), gt_verb, gt_noun (N,)
  vis_info.json  the class names, the video ids and the table the reference made: one list per column
Usage:  python tests/golden/make_vis_golden.py
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

N, SEGMENTS, T = 12, 3, 8
VERBS = ["take", "put", "open", "close", "wash", "cut", "mix"]
NOUNS = ["pan", "tap", "plate", "knife", "spoon", "bowl", "fridge", "lid", "cup", "onion", "sponge"]


def install_vis_stubs():
    G.install_stubs()
    qgrid = types.ModuleType("qgrid")
    qgrid.show_grid = lambda df, **kw: df
    sys.modules["qgrid"] = qgrid
    moviepy = types.ModuleType("moviepy")
    moviepy.editor = types.ModuleType("moviepy.editor")
    sys.modules["moviepy"], sys.modules["moviepy.editor"] = moviepy, moviepy.editor
    omegaconf = types.ModuleType("omegaconf")
    omegaconf.OmegaConf = type("OmegaConf", (), {})
    omegaconf.dictconfig = types.ModuleType("omegaconf.dictconfig")
    omegaconf.dictconfig.DictConfig = dict
    sys.modules["omegaconf"], sys.modules["omegaconf.dictconfig"] = omegaconf, omegaconf.dictconfig
    tbx = types.ModuleType("tensorboardX")
    tbx.SummaryWriter = object
    sys.modules["tensorboardX"] = tbx


def write_class_files(path):
    import pandas as pd
    os.makedirs(path, exist_ok=True)
    pd.DataFrame({"verb_id": range(len(VERBS)), "class_key": VERBS, "verbs": [repr([v]) for v in VERBS]}).to_csv(
        os.path.join(path, "EPIC_verb_classes.csv"), index=False)
    pd.DataFrame({"noun_id": range(len(NOUNS)), "class_key": NOUNS, "nouns": [repr([v]) for v in NOUNS]}).to_csv(
        os.path.join(path, "EPIC_noun_classes.csv"), index=False)


class FakeDataset(torch.utils.data.Dataset):
    def __init__(self, gt_verb, gt_noun):
        self.gt_verb, self.gt_noun = gt_verb, gt_noun

    def __len__(self):
        return len(self.gt_verb)

    def __getitem__(self, i):
        data = {"vid_id": "P{:02d}_{:02d}".format(1 + i // 4, 1 + i % 4), "clip": torch.tensor(i)}
        target = {"class": {"verb": torch.tensor(int(self.gt_verb[i])), "noun": torch.tensor(int(self.gt_noun[i]))}}
        return data, target, i


class FakeModel(object):
    def __init__(self, verb, noun, weights):
        self.verb, self.noun, self.weights = verb, noun, weights

    def eval(self):
        return self

    def __call__(self, data):
        i = int(data["clip"][0])
        return {"verb": self.verb[i:i + 1], "noun": self.noun[i:i + 1],
                "weights": self.weights[i * SEGMENTS:(i + 1) * SEGMENTS].unsqueeze(1)}


def main():
    install_vis_stubs()
    spec = importlib.util.spec_from_file_location("ref_vis", G.REF + "/core/tools/vis.py")
    vis = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vis)
    from core.dataset import EpicClasses
    gen = torch.Generator().manual_seed(21)
    verb = torch.randn(N, len(VERBS), generator=gen) * 4
    noun = torch.randn(N, len(NOUNS), generator=gen) * 4
    weights = torch.softmax(torch.randn(N * SEGMENTS, T, generator=gen) * 2, 1)
    weights[0] = torch.nn.functional.one_hot(torch.tensor(3), T).float()      # Gumbel `hard` row
    weights[4] = 1.0 / T
    gt_verb = torch.randint(0, len(VERBS), (N,), generator=gen).numpy()
    gt_noun = torch.randint(0, len(NOUNS), (N,), generator=gen).numpy()
    with tempfile.TemporaryDirectory() as tmp:
        write_class_files(tmp)
        df = vis.get_info(FakeModel(verb, noun, weights), FakeDataset(gt_verb, gt_noun), EpicClasses(tmp),
                          torch.device("cpu"))
    assert df.index.name == "Index" and list(df.index) == list(range(1, N + 1))
    G.save("vis_info.npz", verb=verb, noun=noun, weights=weights, gt_verb=gt_verb, gt_noun=gt_noun)
    with open(os.path.join(HERE, "vis_info.json"), "w") as f:
        json.dump({"verbs": VERBS, "nouns": NOUNS, "segments": SEGMENTS, "columns": list(df.columns),
                   "table": {c: df[c].tolist() for c in df.columns}}, f, indent=1)
    print(df)


if __name__ == "__main__":
    main()
