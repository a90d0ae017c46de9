"""The visualisation module of the reference (`core/tools/vis.py:30-364`, README "Visualization Module"): `initialize`,
`create_dataset`, `get_info`, `visualize` and `save_action_segment` with the reference's positional signatures; what this
package adds is keyword-only.

`get_info` is the reference's table made at the loader's rate: batches from a prefetching `ClipLoader`, one
`ops.clip_summary` launch per batch into device rings (predicted classes, attention entropies; the targets ride in a
ring of their own) and ONE copy per ring after the loop, where the reference runs batch size 1 and reads five scalars per
clip.  `visualize` takes its top-5 names and softmax scores from the same operator."""
import datetime
import os

import numpy as np
import torch

from ... import ops
from ...config import get_modality, load_config_file
from ..dataset.dataset import Video_Dataset
from ..dataset.epic_class import EpicClasses
from ..dataset.frames import decode_frames
from ..dataset.transform import get_transforms
from ..models import build_model
from ..utils import ClipLoader

LINE = "----------------------------------------------------------"
COLUMNS = ("vid_id", "gt_verb", "gt_noun", "pred_verb", "pred_noun", "entropy")
UNKNOWN = "Unknown"


def info_table(vid_ids, gt_verb, gt_noun, pred_verb, pred_noun, entropy, epic_classes):
    """The reference's DataFrame (:55-62, :88-90) from host arrays, one entry per clip: class ids of the ground truth (-1:
    unlabelled, shown as "Unknown") and of the predictions, and the entropies (None: the model gave no weights, the
    column reads "N/A").  Needs no GPU."""
    import pandas as pd
    verbs, nouns = epic_classes.verbs, epic_classes.nouns

    def names(table, ids, unknown):
        return [unknown if int(i) < 0 else table[int(i)] for i in ids]

    n = len(vid_ids)
    data_dict = {
        "vid_id": list(vid_ids),
        "gt_verb": names(verbs, gt_verb, UNKNOWN),
        "gt_noun": names(nouns, gt_noun, UNKNOWN),
        "pred_verb": names(verbs, pred_verb, UNKNOWN),
        "pred_noun": names(nouns, pred_noun, UNKNOWN),
        "entropy": ["N/A"] * n if entropy is None else [float(e) for e in entropy],
    }
    df = pd.DataFrame.from_dict(data_dict)
    df.index += 1
    df.index.name = "Index"
    return df


def _show(df, widget):
    if widget is None:
        try:
            import qgrid  # noqa: F401
            widget = True
        except ImportError:
            widget = False
    if not widget:
        return df
    import qgrid
    return qgrid.show_grid(df, show_toolbar=False, column_options={"editable": False})


def get_info(model, dataset, epic_classes, device, *, batch_size=8, prefetch=2, widget=None):
    """reference :30-93 -> the table of `vid_id`, ground truth, top-1 predictions and attention entropy per clip, index
    from 1.  A pandas DataFrame; wrapped in a qgrid widget with `widget=True`, or with `widget=None` when qgrid is
    installed.  The host reads the device once per ring after the loop, however many batches there were."""
    n = len(dataset)
    loader = ClipLoader(dataset, batch_size, shuffle=False, prefetch=prefetch)
    idx = torch.full((n, 2, 1), -1, dtype=torch.int32, device=device)
    prob = torch.zeros((n, 2, 1), dtype=torch.float32, device=device)
    gt = torch.full((n, 2), -1, dtype=torch.int64, device=device)
    ent = None
    vid_ids, row = [], 0
    model.eval()
    try:
        with torch.no_grad():
            for data, target, _ in loader:
                out = model(data)
                scores = {"verb": out["verb"], "noun": out["noun"]}
                B = scores["verb"].shape[0]
                weights, segments = out.get("weights"), 1
                if weights is not None:
                    segments = weights.shape[0] // B
                    if ent is None:
                        ent = torch.zeros((n,), dtype=torch.float32, device=device)
                ops.clip_summary(scores, 1, weights, segments, out=(idx, prob, ent), row=row)
                cls = target["class"]
                if isinstance(cls, dict):
                    gt[row:row + B, 0] = cls["verb"]
                    gt[row:row + B, 1] = cls["noun"]
                vid_ids.extend(data["vid_id"])
                row += B
    finally:
        loader.close()
    idx_h = idx.cpu().numpy()
    gt_h = gt.cpu().numpy()
    ent_h = ent.cpu().numpy() if ent is not None else None
    df = info_table(vid_ids, gt_h[:row, 0], gt_h[:row, 1], idx_h[:row, 0, 0], idx_h[:row, 1, 0],
                    None if ent_h is None else ent_h[:row], epic_classes)
    return _show(df, widget)


def save_action_segment(data_dir, vid_id, start_time, stop_time, *, out_dir="results"):
    """reference :96-114: the trimmed action segment of `<data_dir>/vid_symlinks/<vid_id>.MP4` -> `<out_dir>/temp.MP4`"""
    try:
        import moviepy.editor as mpe
    except ImportError as e:
        raise ImportError("save_action_segment needs moviepy (moviepy.editor.VideoFileClip), which is not installed") from e
    vid_file = os.path.join(data_dir, f"vid_symlinks/{vid_id}.MP4")
    video = mpe.VideoFileClip(vid_file).subclip(start_time, stop_time)
    video.write_videofile(os.path.join(out_dir, "temp.MP4"), logger=None)
    video.close()


def visualize(cfg, model, criterion, dataset, index, epic_classes, device, *, out_dir="results", save_video=False):
    """reference :117-237: frames, spectrograms, attention weights and class scores of item `index` (from 1, as the
    table counts) on one 4 x cfg.test.num_segments figure, written to `<out_dir>/vis.png` -> (fig, info).  `info` is the
    plain data behind the figure: vid_id, verbs / nouns (ground truth first, then the top five), verb_scores /
    noun_scores, weights (n, 1, T), spectrograms (n, H, W), frame_indices, times."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    n_seg = cfg.test.num_segments
    data, target, _ = dataset.batch([index - 1])
    vid_id = data["vid_id"][0]
    rgb_indices = data["indices"]["RGB"].cpu().numpy().reshape(-1)
    spec = data["Audio"].detach().cpu().numpy().squeeze()
    if spec.ndim == 2:
        spec = spec[None]
    model.eval()
    with torch.no_grad():
        out = model(data)
        idx, prob, _ = ops.clip_summary({"verb": out["verb"], "noun": out["noun"]}, 5)
    idx, prob = idx.cpu().numpy()[0], prob.cpu().numpy()[0]
    cls = target["class"]
    gt_verb, gt_noun = (int(cls["verb"][0]), int(cls["noun"][0])) if isinstance(cls, dict) else (-1, -1)
    if gt_verb == -1 or gt_noun == -1:
        verb_gt, noun_gt, gt_score = UNKNOWN, UNKNOWN, 0.0
    else:
        verb_gt, noun_gt, gt_score = epic_classes.verbs[gt_verb], epic_classes.nouns[gt_noun], 1.0
    verbs = [verb_gt] + [epic_classes.verbs[int(i)] for i in idx[0]]
    nouns = [noun_gt] + [epic_classes.nouns[int(i)] for i in idx[1]]
    verb_scores = [gt_score] + [float(p) for p in prob[0]]
    noun_scores = [gt_score] + [float(p) for p in prob[1]]

    if "weights" in out.keys():
        weights = out["weights"].detach()
        if weights.dim() == 2:
            weights = weights.unsqueeze(1)
        weights = weights.cpu().numpy()
    else:
        weights = np.zeros((n_seg, 1, 25))      # a model without attention: dummy weights, as the reference

    blobs = []
    for i in rgb_indices[:n_seg]:
        name = "img_{:010d}.{}".format(int(i), cfg.data.rgb.file_ext)
        with open(os.path.join(cfg.data_dir, cfg.data.rgb.dir_prefix, vid_id, name), "rb") as f:
            blobs.append(f.read())
    frames = decode_frames(blobs, device=device).flip(-1).cpu().numpy()      # BGR -> RGB
    times = [str(datetime.timedelta(seconds=int(i) / cfg.data.vid_fps))[0:-3] for i in rgb_indices[:n_seg]]

    fig = Figure(figsize=(16, 16))
    FigureCanvasAgg(fig)
    axarr = np.asarray(fig.subplots(4, n_seg)).reshape(4, n_seg)
    axarr[0, 0].set_ylabel("RGB Frames", fontsize=10)
    axarr[1, 0].set_ylabel("Audio Spectrograms", fontsize=10)
    axarr[2, 0].set_ylabel("Attention Weights", fontsize=10)
    axarr[3, 0].set_ylabel("Classes")
    x = np.arange(weights.shape[2])
    for s in range(n_seg):
        axarr[0, s].imshow(frames[s], aspect="auto")
        axarr[0, s].set_title(f"Time: {times[s]}")
        axarr[1, s].imshow(spec[s], cmap="jet", origin="lower", aspect="auto")
        axarr[2, s].plot(x, weights[s].squeeze(0))
        axarr[2, s].set_ylim([0, 1])
        axarr[2, s].set_xlim([0, weights.shape[2] - 1])
    colours = ["red", "blue", "green", "green", "green", "green"]
    bars = [(verbs, verb_scores, "Verbs"), (nouns, noun_scores, "Nouns")]
    for col, (labels, scores, title) in enumerate(bars[:n_seg]):
        axarr[3, col].bar(np.arange(len(labels)), scores, width=0.5, align="center", alpha=1.0, color=colours)
        axarr[3, col].set_xticks(np.arange(len(labels)))
        axarr[3, col].set_xticklabels(labels)
        axarr[3, col].set_title(title)
    for col in range(2, n_seg):
        axarr[3, col].axis("off")
    fig.suptitle(f"Video Id: {vid_id}", fontsize=20)
    os.makedirs(out_dir, exist_ok=True)
    fig.savefig(os.path.join(out_dir, "vis.png"))
    if save_video:
        save_action_segment(cfg.data_dir, vid_id, data["start_time"][0], data["stop_time"][0], out_dir=out_dir)
    info = {"vid_id": vid_id, "verbs": verbs, "verb_scores": verb_scores, "nouns": nouns, "noun_scores": noun_scores,
            "weights": weights, "spectrograms": spec, "frame_indices": [int(i) for i in rgb_indices[:n_seg]],
            "times": times}
    return fig, info


def filter_actions(annotations, action_list, epic_classes):
    """reference core/dataset/dataset.py:94-112: the rows of `annotations` whose `action` column ("verb_id,noun_id") is
    one of `action_list`'s (verb, noun) word pairs; a word of no class raises ValueError."""
    verb_df, noun_df = epic_classes.verb_df, epic_classes.noun_df
    action_ids = []
    for verb, noun in action_list:
        verb_id = verb_df[verb_df["verbs"] == verb].verb_id.values
        noun_id = noun_df[noun_df["nouns"] == noun].noun_id.values
        if len(verb_id) == 0:
            raise ValueError(f"create_dataset: {verb!r} is a verb of no class in EPIC_verb_classes.csv")
        if len(noun_id) == 0:
            raise ValueError(f"create_dataset: {noun!r} is a noun of no class in EPIC_noun_classes.csv")
        action_ids.append(f"{verb_id[0]},{noun_id[0]}")
    return annotations[annotations["action"].isin(action_ids)]


def create_dataset(cfg, action_list=None, *, device="cuda", **dataset_kw):
    """reference :240-311 -> the test-mode dataset over `cfg.test.annotation_file[0]`, narrowed to `action_list`
    ((verb, noun) word pairs) when one is given; None, with the reference's message, when nothing is left."""
    modality = get_modality(cfg)
    transforms = get_transforms(cfg, modality, "test", device=device, flow_length=2 * cfg.data.flow.win_length)
    if cfg.test.vid_list:
        print("Reading list of test videos...")
        with open(os.path.join("./", cfg.test.vid_list)) as f:
            test_list = [x.strip() for x in f.readlines() if len(x.strip()) > 0]
        print("Done.")
        print(LINE)
    else:
        test_list = None
    annotation = cfg.test.annotation_file
    annotation = annotation if isinstance(annotation, str) else annotation[0]
    print("Creating the dataset using {}...".format(annotation))
    dataset = Video_Dataset(cfg, test_list, annotation, modality, transform=transforms, mode="test",
                            device=device, **dataset_kw)
    if action_list is not None and len(action_list) > 0 and cfg.data.dataset == "epic":
        epic_classes = EpicClasses(os.path.join(cfg.data_dir, "annotations"))
        dataset.annotations = filter_actions(dataset.annotations, action_list, epic_classes)
    print("Done.")
    print(LINE)
    if len(dataset) > 0:
        return dataset
    print("!!!! No data found for these videos and actions. Please try again !!!!")
    return None


def initialize(config_file):
    """reference :314-364 -> (cfg, model, criterion, epic_classes, device)"""
    cfg = load_config_file(config_file)
    np.random.seed(cfg.data.manual_seed)
    torch.manual_seed(cfg.data.manual_seed)
    modality = get_modality(cfg)
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    print("Initializing model...")
    model, criterion, num_gpus = build_model(cfg, modality, device)
    print("Model initialized.")
    print(LINE)
    if cfg.test.pre_trained:
        if os.path.exists(cfg.test.pre_trained):
            print("Loading pre-trained weights {}...".format(cfg.test.pre_trained))
            data_dict = torch.load(cfg.test.pre_trained, map_location="cpu")
            (model.module if num_gpus > 1 and hasattr(model, "module") else model).load_state_dict(data_dict["model"])
            print("Done.")
            print(LINE)
        else:
            raise Exception(f"{cfg.test.pre_trained} file not found.")
    epic_classes = EpicClasses(os.path.join(cfg.data_dir, "annotations"))
    return cfg, model, criterion, epic_classes, device
