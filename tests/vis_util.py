"""What the visualiser tests share: EPIC class files written into <root>/annotations and annotation files with the
`action` column the reference's action filter reads."""
import json
import os

import numpy as np

from tests import clip_loader_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# class id -> (class_key, words); ten of each, so every label of clip_loader_util.ROWS has a name
VERB_CLASSES = [("take", ["take", "grab", "pick-up"]), ("put", ["put", "place"]), ("open", ["open", "unscrew"]),
                ("close", ["close", "shut"]), ("wash", ["wash", "rinse"]), ("cut", ["cut", "slice"]), ("mix", ["mix"]),
                ("pour", ["pour"]), ("throw", ["throw"]), ("dry", ["dry"])]
NOUN_CLASSES = [("pan", ["pan", "skillet"]), ("tap", ["tap"]), ("plate", ["plate", "dish"]), ("knife", ["knife"]),
                ("spoon", ["spoon"]), ("bowl", ["bowl"]), ("fridge", ["fridge"]), ("lid", ["lid", "cover"]),
                ("cup", ["cup", "mug"]), ("onion", ["onion"])]
MANY_SHOT = [(3, "close", 7, "lid"), (5, "cut", 1, "tap")]


def write_class_files(root, verbs=None, nouns=None):
    """-> <root>/annotations with the three files `EpicClasses` reads; `verbs` / `nouns`: plain name lists instead"""
    path = os.path.join(str(root), "annotations")
    os.makedirs(path, exist_ok=True)
    verb_rows = VERB_CLASSES if verbs is None else [(v, [v]) for v in verbs]
    noun_rows = NOUN_CLASSES if nouns is None else [(v, [v]) for v in nouns]
    for name, col, rows in (("verb", "verbs", verb_rows), ("noun", "nouns", noun_rows)):
        with open(os.path.join(path, "EPIC_{}_classes.csv".format(name)), "w") as f:
            f.write("{}_id,class_key,{}\n".format(name, col))
            for i, (key, words) in enumerate(rows):
                f.write('{},{},"{}"\n'.format(i, key, repr(list(words))))
    with open(os.path.join(path, "EPIC_many_shot_actions.csv"), "w") as f:
        f.write("action_class,verb_class,verb,noun_class,noun\n")
        for verb_id, verb, noun_id, noun in MANY_SHOT:
            f.write('"({}, {})",{},{},{},{}\n'.format(verb_id, noun_id, verb_id, verb, noun_id, noun))
    return path


def write_annotations(root, name, vids, rows, labels=True):
    """rows of (uid, video index, start_frame, stop_frame, verb, noun) -> <root>/<name> in clip_loader_util's layout
    plus the `action` column ("verb_id,noun_id")"""
    with open(os.path.join(str(root), name), "w") as f:
        cols = "uid,video_id,start_timestamp,stop_timestamp,start_frame,stop_frame"
        f.write(cols + (",verb_class,noun_class,action_class,action\n" if labels else "\n"))
        for uid, vid, a, b, verb, noun in rows:
            line = "{},{},00:00:01.00,00:00:02.00,{},{}".format(uid, vids[vid], a, b)
            f.write(line + (',{},{},"{},{}","{},{}"\n'.format(verb, noun, verb, noun, verb, noun) if labels else "\n"))


ROWS5 = [(21, 0, 1, 16, 3, 7), (22, 1, 2, 15, 5, 1), (23, 0, 3, 14, 0, 9), (24, 1, 1, 12, 3, 7), (25, 0, 2, 13, 2, 2)]


def small_cfg(tmp_path, extra=()):
    """clip_loader_util's small dataset with five annotation rows that carry an `action` column, and the class files"""
    from attention_based_tbn_amd.config import load_config
    overrides = U.write_dataset(tmp_path)
    write_annotations(tmp_path, "ann_vis.csv", U.VIDS, ROWS5)
    write_class_files(tmp_path)
    return load_config(overrides + ["test.annotation_file=[ann_vis.csv]"] + list(extra))


class Names(object):
    def __init__(self, verbs, nouns):
        self.verbs, self.nouns = verbs, nouns


def fixture_expectations():
    """the committed fixture -> (inputs, exact fp64 top-1 and entropies, names, the reference's table)"""
    z = np.load(os.path.join(GOLDEN, "vis_info.npz"))
    with open(os.path.join(GOLDEN, "vis_info.json")) as f:
        meta = json.load(f)
    verb, noun, w = z["verb"].astype(np.float64), z["noun"].astype(np.float64), z["weights"].astype(np.float64)
    ent = (-(w * np.log(w + np.float64(np.float32(1e-6)))).sum(1)).reshape(-1, meta["segments"]).mean(1)
    return z, (verb.argmax(1), noun.argmax(1), ent), meta


def check_table(df, meta, rel=1e-6, atol=0.0):
    """names equal; entropies within `rel` of the reference's (its fp32 arithmetic) plus `atol` per row"""
    assert list(df.columns) == meta["columns"] == ["vid_id", "gt_verb", "gt_noun", "pred_verb", "pred_noun", "entropy"]
    assert df.index.name == "Index" and list(df.index) == list(range(1, len(df) + 1))
    for col in meta["columns"][:-1]:
        assert df[col].tolist() == meta["table"][col], col
    got, want = np.asarray(df["entropy"].tolist(), dtype=np.float64), np.asarray(meta["table"]["entropy"])
    assert np.all(np.abs(got - want) <= rel * np.abs(want) + atol), (got, want)
