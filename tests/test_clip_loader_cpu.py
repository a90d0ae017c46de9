"""Host half of the clip loader (core/dataset/dataset.py `Video_Dataset`, core/utils/create_dataloader.py `ClipLoader`,
`DevicePipeline._record_batch` / `_clip_table`): draw order, geometry table, file lists, the .wav reader, refusals and
the batch partition.  No GPU: everything here is recorded, nothing is launched.  Integer data: equality throughout."""
import logging
import os
import wave

import numpy as np
import pytest
import torch

from oracle import sampler as osamp
from oracle import transform as otf
from tests import clip_loader_util as U

MODALITY = ["RGB", "Flow", "Audio"]
SCALES = {"RGB": [1, 0.875, 0.75, 0.66], "Flow": [1, 0.875, 0.75]}


def _cfg(tmp_path, extra=(), **kw):
    from attention_based_tbn_amd.config import load_config
    return load_config(U.write_dataset(tmp_path, **kw) + list(extra))


def _expected_row(geo):
    """the arguments `_frames_to_tensor` hands tbn_frames_to_tensor for one recorded clip"""
    rw, rh = geo.resized if geo.resized is not None else (geo.box[2], geo.box[3])
    cx, cy, ow, oh = geo.crop if geo.crop is not None else (0, 0, rw, rh)
    return dict(box_x=geo.box[0], box_y=geo.box[1], box_w=geo.box[2], box_h=geo.box[3], resized_w=rw, resized_h=rh,
                crop_x=cx, crop_y=cy, flip=int(geo.flip)), (ow, oh)


@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("m", ["RGB", "Flow"])
def test_batch_geometry_table_equals_consecutive_per_clip_recordings(m, mode):
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import get_transforms
    cfg = load_config(["data.train_crop_size=16", "data.test_scale_size=20", "data.test_crop_size=16"])
    pipe = get_transforms(cfg, [m], mode, flow_length=4)[m]
    sizes = [(40, 56), (35, 50), (40, 56), (57, 45), (35, 50)]           # three source sizes in one batch
    clips = [[0, 2], [1, 4], [3]]                                         # the groups, by batch position
    per_clip = 3 if m == "RGB" else 8
    rows_per_clip = per_clip // pipe.stack
    for seed in range(20):
        np.random.seed(seed)
        geos = pipe._record_batch(sizes)
        after = np.random.random()
        table, starts, (ow, oh) = pipe._clip_table(geos, clips, per_clip)
        np.random.seed(seed)
        singles = [pipe._record(h, w) for h, w in sizes]                  # what B consecutive __call__s record
        assert after == np.random.random()
        assert starts == [0, 2, 4] and (ow, oh) == (16, 16)
        k = 0
        for part in clips:
            for slot, b in enumerate(part):
                want, size = _expected_row(singles[b])
                assert size == (16, 16)
                got = {f: getattr(table[k], f) for f in want}
                assert got == want, (seed, b, got, want)
                assert table[k].first_img == slot * per_clip and table[k].out_row == b * rows_per_clip
                assert table[k].reserved == 0 and (geos[b].src_h, geos[b].src_w) == sizes[b]
                k += 1
        if mode == "train":                                               # ... and those are the oracle's draws
            np.random.seed(seed)
            for b, (h, w) in enumerate(sizes):
                cw, ch, ox, oy = otf.sample_crop_size((h, w), (16, 16), SCALES[m])
                flip = np.random.random() < 0.5
                assert singles[b].box == [ox, oy, cw, ch] and singles[b].flip == flip


@pytest.mark.parametrize("sampling", ["async", "sync"])
def test_train_draw_order_is_the_reference_getitem_clip_after_clip(tmp_path, sampling):
    cfg = _cfg(tmp_path, ["data.sampling=" + sampling])
    ds = U.make_dataset(cfg, MODALITY, "train")
    assert len(ds) == 3
    for seed in (0, 1, 2, 3, 11):
        np.random.seed(seed)
        clips = ds.plan([2, 0, 1])
        state = np.random.get_state()
        np.random.seed(seed)
        for clip, row in zip(clips, (2, 0, 1)):
            _, vid, start, stop, _, _ = U.ROWS[row]
            first, num = osamp.frame_span(start, stop)
            want = {}
            for m_no, m in enumerate(MODALITY):
                if m_no > 0 and sampling == "sync":
                    want[m] = (want["RGB"] / 2).astype(np.int64) if m == "Flow" else want["RGB"]
                else:
                    want[m] = osamp.get_offsets(first[m], num[m], m, "train", 2, 2 if m == "Flow" else 1)
                assert clip.indices[m].dtype == np.int64 and clip.indices[m].tolist() == want[m].tolist(), (seed, m)
                if m != "Audio":        # this modality's transform draws right after this modality's offsets
                    cw, ch, ox, oy = otf.sample_crop_size((40, 56), (16, 16), SCALES[m])
                    flip = np.random.random() < 0.5
                    geo = clip.visual[m].geo
                    assert geo.box == [ox, oy, cw, ch] and geo.flip == flip, (seed, m)
            assert clip.vid_id == vid
        want_state = np.random.get_state()
        assert state[0] == want_state[0] and np.array_equal(state[1], want_state[1]) and state[2:] == want_state[2:]


def test_file_lists_rgb_flow_interleaved_sync_halving_and_val_centring(tmp_path):
    cfg = _cfg(tmp_path, ["data.sampling=sync"])
    ds = U.make_dataset(cfg, MODALITY, "train")
    np.random.seed(4)
    clip = ds.plan([1])[0]
    rgb, flow = clip.indices["RGB"], clip.indices["Flow"]
    root = str(tmp_path)
    assert clip.visual["RGB"].paths == [os.path.join(root, "rgb", "P01_02", "img_%010d.jpg" % i) for i in rgb]
    assert flow.tolist() == [int(i / 2) for i in rgb] and clip.indices["Audio"] is rgb
    want = []
    for i in flow:                       # win_length = 2 consecutive indices per segment, x then y
        for j in (i, i + 1):
            want += [os.path.join(root, "flow", "P01_02", "%s_%010d.jpg" % (a, j)) for a in ("x", "y")]
    assert clip.visual["Flow"].paths == want and len(want) == 8
    # val mode draws nothing: centre offsets, the Flow window centred (offset - win_length // 2, never negative)
    cfg = _cfg(tmp_path, ["data.sampling=async"])
    ds = U.make_dataset(cfg, MODALITY, "val")
    state = np.random.get_state()
    clips = ds.plan([0, 1, 2])
    assert np.array_equal(state[1], np.random.get_state()[1])
    for clip, (_, vid, start, stop, _, _) in zip(clips, U.ROWS):
        first, num = osamp.frame_span(start, stop)
        for m in MODALITY:
            want = osamp.get_offsets(first[m], num[m], m, "val", 2, 2 if m == "Flow" else 1)
            assert clip.indices[m].tolist() == want.tolist()
    assert clips[0].indices["RGB"].tolist() == [3, 10]          # 14 frames from 0: segments of 7, centre 3
    assert clips[0].indices["Flow"].tolist() == [0, 3]          # 7 frames from 0: segments of 3, centre 1, minus 2 // 2
    assert clips[0].visual["Flow"].paths[:4] == [os.path.join(root, "flow", "P01_01", "%s_%010d.jpg" % (a, j))
                                                 for j in (0, 1) for a in ("x", "y")]
    # test-mode geometry: Rescale(20) of 40x56 -> 20x28, centre crop 16
    geo = clips[0].visual["RGB"].geo
    assert geo.resized == (28, 20) and geo.crop == [6, 2, 16, 16] and not geo.flip


def _write_wav(path, pcm, rate, width=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(pcm.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


def test_wav_reader(tmp_path):
    from attention_based_tbn_amd.core.dataset import read_wav
    rng = np.random.RandomState(1)
    pcm = rng.randint(-32768, 32768, (5000, 2)).astype("<i2")
    pcm[0], pcm[1] = (-32768, -32768), (32767, 32766)
    _write_wav(tmp_path / "s.wav", pcm, 24000)
    got = read_wav(str(tmp_path / "s.wav"), 24000)
    want = (pcm.astype(np.float64).mean(axis=1) / 32768.0).astype(np.float32)      # exact: 17-bit sums, powers of two
    assert got.dtype == np.float32 and got.shape == (5000,) and np.array_equal(got, want)
    assert got[0] == -1.0 and got.max() < 1.0
    _write_wav(tmp_path / "m.wav", pcm[:, :1], 24000)
    assert np.array_equal(read_wav(str(tmp_path / "m.wav"), 24000), pcm[:, 0].astype(np.float32) / np.float32(32768))
    with pytest.raises(ValueError, match="resampling"):
        read_wav(str(tmp_path / "s.wav"), 16000)
    _write_wav(tmp_path / "b.wav", (pcm[:, :1] >> 8).astype(np.uint8), 24000, width=1)
    with pytest.raises(ValueError, match="8-bit"):
        read_wav(str(tmp_path / "b.wav"), 24000)


def test_refusals(tmp_path):
    from attention_based_tbn_amd.core.dataset import Video_Dataset, get_transforms
    cfg = _cfg(tmp_path)
    tfs = get_transforms(cfg, MODALITY, "train", flow_length=4)
    with pytest.raises(NotImplementedError, match="EpicClasses"):
        Video_Dataset(cfg, list(U.VIDS), "ann.csv", MODALITY, transform=tfs, mode="train", action_list=[("take", "plate")])
    with pytest.raises(TypeError, match="DevicePipeline"):
        Video_Dataset(cfg, list(U.VIDS), "ann.csv", MODALITY, transform={"RGB": lambda x: x}, mode="train")
    ds = Video_Dataset(cfg, ["P01_02"], "ann.csv", MODALITY, transform=tfs, mode="val")
    assert len(ds) == 1                                           # `video_id in vid_list`
    ds = U.make_dataset(cfg, MODALITY, "val")
    missing = ds.plan([0])[0].visual["Flow"].paths[3]            # val mode: the same files at every call
    assert missing.startswith(os.path.join(str(tmp_path), "flow", "P01_01", "y_"))
    os.remove(missing)
    with pytest.raises(Exception) as e:
        ds.plan([0])
    assert missing in str(e.value)


def test_clip_loader_partition_and_train_order(tmp_path):
    from attention_based_tbn_amd.core.utils import ClipLoader, create_dataloader
    cfg = _cfg(tmp_path)
    log = logging.getLogger("clip_loader_test")
    seen = []
    for mode in ("val", "test", "train"):
        loader = create_dataloader(cfg, log, MODALITY, mode)
        assert isinstance(loader, ClipLoader) and len(loader) == 2 and loader.batch_size == 2
        assert len(loader.dataset) == 3 and loader.dataset.mode == mode
        assert loader.dataset.transform["Flow"].stack == 4
        loader.dataset.batch = lambda part: seen.append(list(part)) or part       # no GPU here: record the partition
        if mode != "train":
            assert list(loader) == [[0, 1], [2]]                  # sequential, the last shorter batch kept
        else:
            for seed in (0, 1, 5):
                torch.manual_seed(seed)
                got = list(loader)
                torch.manual_seed(seed)
                order = torch.randperm(3).tolist()
                assert got == [order[:2], order[2:]]
    assert len(seen) == 2 * 2 + 3 * 2


def test_batch_entry_validates_the_table_on_the_host_before_any_launch():
    """every refusal of tbn_frames_to_tensor_batch is host code: it needs no GPU and never dereferences a device pointer"""
    from attention_based_tbn_amd._lib import FramesClip, lib
    L = lib()
    bad = 0x1000

    def call(rows, n_img=6, per_clip=2, stack=2, out_rows=3, dev=bad, n_clips=None):
        host = (FramesClip * max(1, len(rows)))(*[FramesClip(*r) for r in rows])
        rc = L.tbn_frames_to_tensor_batch(bad, n_img, 37, 53, 1, host, dev, len(rows) if n_clips is None else n_clips,
                                          per_clip, 16, 16, stack, None, None, 0, 1, bad, out_rows, None)
        return rc, L.tbn_last_error().decode()

    good = [(0, 5, 3, 30, 20, 24, 18, 4, 1, 0, 0, 0), (2, 0, 0, 16, 16, 16, 16, 0, 0, 1, 1, 0),
            (4, 1, 1, 9, 11, 16, 16, 0, 0, 0, 2, 0)]

    def edit(i, **kw):
        names = [f for f, _ in FramesClip._fields_]
        rows = [list(r) for r in good]
        for k, v in kw.items():
            rows[i][names.index(k)] = v
        return [tuple(r) for r in rows]

    assert call([], n_clips=0)[0] == 0
    for rows, needle, kw in [
            (edit(2, first_img=5), "clip 2: images 5..6 outside the 6 frames", {}),
            (edit(0, first_img=-1), "clip 0: images", {}),
            (edit(1, box_x=40), "clip 1: source box (40,0,16,16) outside the 53x37 frame", {}),
            (edit(1, box_w=2 ** 31 - 1), "clip 1: source box", {}),
            (edit(2, crop_x=1), "clip 2: crop window (1,0,16,16) outside the resized 16x16 box", {}),
            (edit(1, out_row=3), "clip 1: output rows 3..3 outside the 3 rows", {}),
            (edit(0, out_row=-1), "clip 0: output rows", {}),
            (edit(1, out_row=2), "clip 1 and clip 2 write overlapping output rows", {}),
            (good[:2], "clip 0: 3 images per clip is not a positive multiple of the stack length 2", dict(per_clip=3)),
            (good, "null argument", dict(dev=None)),
            (good, "output width", dict())]:
        if needle == "output width":
            host = (FramesClip * 3)(*[FramesClip(*r) for r in good])
            rc = L.tbn_frames_to_tensor_batch(bad, 6, 37, 53, 1, host, bad, 3, 2, 1025, 16, 2, None, None, 0, 1, bad, 3, None)
            msg = L.tbn_last_error().decode()
        else:
            rc, msg = call(rows, **kw)
        assert rc < 0 and needle in msg, (needle, rc, msg)
    # mean / std missing with n_stat > 0
    host = (FramesClip * 3)(*[FramesClip(*r) for r in good])
    rc = L.tbn_frames_to_tensor_batch(bad, 6, 37, 53, 1, host, bad, 3, 2, 16, 16, 2, None, None, 1, 1, bad, 3, None)
    assert rc < 0 and "mean/std missing" in L.tbn_last_error().decode()
