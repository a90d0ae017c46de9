"""`Video_Dataset`: the reference's dataset (`core/dataset/dataset.py:18-192`, `core/dataset/epic_record.py`) at BATCH
level, on the device.

The reference's `__getitem__` reads and transforms one trimmed action segment on the host and the DataLoader collates B
of them.  Here `batch(indices)` makes the collated batch directly: it first *records* the batch on the host -- per clip,
per modality, the segment indices and then the transform's geometry, in exactly the reference's NumPy draw order
(`plan`) -- and then runs each stage once for the whole batch:

  RGB / Flow   every file of the batch goes through ONE `decode_jpegs` call per modality (files are grouped by the
               geometry `tbn_jpeg_parse` reports: a batch with two frame sizes costs two decodes and two launches; files
               of one size but different chroma sampling decode separately and still launch together) and
               ONE `tbn_frames_to_tensor_batch` launch per group applies each clip's own crop box and flip
               (`DevicePipeline._run_batch`);
  Audio        untrimmed waveforms live on the device in an LRU keyed by video id; one `AudioSegments` call cuts the
               windows of every clip, computes the spectrograms and the attention prior.

`__getitem__(i)` is `batch([i])` without the batch dimension: the reference's item, already on the device.
"""
import os
import wave
from collections import OrderedDict

import numpy as np
import torch

from ..._lib import TbnHipError
from .audio import AudioSegments
from .audio_file import load_audio
from .frames import (PNG_HEADER_BYTES, FrameReader, decode_jpegs, decode_pngs, geometry_key, is_png, jpeg_geometry,
                     png_frame_size, png_geometry)
from .npz_file import load_npz_arrays, npz_member
from .sampler import frame_span, get_offsets
from .transform import DevicePipeline


class EpicVideoRecord(object):
    """One annotation row (reference core/dataset/epic_record.py): the same properties, the frame arithmetic of
    `sampler.frame_span`."""

    def __init__(self, record):
        self._series = record
        self._first, self._num = frame_span(record["start_frame"], record["stop_frame"])

    @property
    def action_id(self):
        return self._series["uid"]

    @property
    def untrimmed_video_name(self):
        return self._series["video_id"]

    @property
    def start_time(self):
        return self._series["start_timestamp"]

    @property
    def stop_time(self):
        return self._series["stop_timestamp"]

    @property
    def start_frame(self):
        return dict(self._first)

    @property
    def end_frame(self):
        return {m: self._first[m] + self._num[m] for m in self._first}

    @property
    def num_frames(self):
        return dict(self._num)

    @property
    def label(self):
        keys = self._series.keys().tolist()
        if "verb_class" in keys and "noun_class" in keys and "action_class" in keys:
            return {"verb": self._series["verb_class"], "noun": self._series["noun_class"]}
        return -1          # the test sets carry no labels


def read_wav(path, sampling_rate):
    """A 16-bit PCM .wav file -> mono float32 in [-1, 1): the mean of the channels, scaled by 1 / 32768.  The reference
    calls librosa.load(sr=sampling_rate, mono=True) (dataset.py:401-414), which also resamples and reads other sample
    formats; both are out of scope here, so another width or rate raises instead of returning different samples."""
    with wave.open(path, "rb") as f:
        width, rate, channels = f.getsampwidth(), f.getframerate(), f.getnchannels()
        if width != 2:
            raise ValueError(f"{path}: {8 * width}-bit samples; only 16-bit PCM is read (librosa's other sample "
                             "formats and its resampling are out of scope)")
        if rate != sampling_rate:
            raise ValueError(f"{path}: sampling rate {rate}, data.audio.sampling_rate is {sampling_rate} (librosa's "
                             "resampling is out of scope: resample the file beforehand)")
        raw = f.readframes(f.getnframes())
    pcm = np.frombuffer(raw, dtype="<i2").reshape(-1, channels).astype(np.float32)
    mono = pcm[:, 0] if channels == 1 else pcm.mean(axis=1, dtype=np.float32)
    return mono * np.float32(1.0 / 32768.0)


_SOF = frozenset(range(0xC0, 0xD0)) - {0xC4, 0xC8, 0xCC}
_HEADER_BYTES = 1 << 16


def jpeg_frame_size(path):
    """(H, W) of a JPEG file from its frame header alone: the markers are walked up to the first SOFn segment over the
    file's first 64 KiB (the whole file only when application segments push the header past that).  What `plan` reads of
    a clip it does not keep: the transform's draw needs the frame size and nothing else."""
    try:
        with open(path, "rb") as f:
            head = f.read(_HEADER_BYTES)
            size = _sof_size(head)
            if size is None and len(head) == _HEADER_BYTES:
                size = _sof_size(head + f.read())
    except OSError:
        raise Exception(f"Problem reading file {path}")
    if size is None:
        raise TbnHipError(f"jpeg_frame_size: {path}: no frame header")
    return size


def _sof_size(b):
    if b[:2] != b"\xff\xd8":
        return None
    at = 2
    while at + 4 <= len(b):
        if b[at] != 0xFF:
            return None
        marker = b[at + 1]
        if marker == 0xFF:                                  # fill byte
            at += 1
        elif marker == 0x01 or 0xD0 <= marker <= 0xD8:      # stand-alone markers
            at += 2
        elif marker in _SOF:
            if at + 9 > len(b):
                return None
            return (b[at + 5] << 8 | b[at + 6], b[at + 7] << 8 | b[at + 8])
        elif marker in (0xD9, 0xDA):                        # the scan begins: no frame header in front of it
            return None
        else:
            at += 2 + (b[at + 2] << 8 | b[at + 3])
    return None


class _Visual(object):
    """what `plan` records for one clip and one visual modality"""

    def __init__(self, paths, blobs, arrays, key, hw, geo, file_keys, records=None):
        self.paths = paths      # the files, in frame order (Flow: x, y interleaved; pickles: one per segment)
        self.blobs = blobs      # their bytes (JPEG; flow pickles with flow_load="device"), or None
        self.arrays = arrays    # flow pickles read on the host: uint8 (n_img, H, W, 1), or None
        self.records = records  # flow pickles with flow_load="device": the `npz_member` record of every file
        self.key = key          # clips of one key (kind, H, W) launch together
        self.file_keys = file_keys   # JPEG: per file, what makes files one `decode_jpegs` call (size, components, sampling)
        self.hw = hw            # source frame size
        self.geo = geo          # the recorded `_Geometry`


class _Clip(object):
    """what `plan` records for one clip"""

    def __init__(self, record):
        self.record = record
        self.kept = True        # False: a clip outside `keep` -- its draws were made, its files were not read
        self.vid_id = record.untrimmed_video_name
        self.indices = OrderedDict()
        self.visual = OrderedDict()


class Video_Dataset(object):
    """The reference's constructor `(cfg, vid_list, annotation_file, modality, transform, mode, action_list=None)` plus
    keyword-only `device`, `threads` / `entropy` (handed to `decode_jpegs`), `inflate` (handed to `decode_pngs`: frames
    are JPEG or PNG by content, as cv2.imread reads them), `audio_cache_bytes` (cap of the device
    waveform cache) and `audio_load`: "host" (the default) reads a raw audio file with `read_wav` -- 16-bit PCM at
    data.audio.sampling_rate, anything else raises; "device" sends the file through `audio_file.load_audio`, which decodes
    any PCM width or float32, downmixes and resamples on the device like the reference's librosa.load (.wav files only;
    audio pickles are read as before).  `flow_load` matters only with data.flow.read_flow_pickle: "host" (the default)
    reads each frame_XXXXXXXXXX.npz with np.load inside `plan`; "device" keeps the files' bytes and inflates every pickle
    of a batch with one `npz_file.load_npz_arrays` call (`flow_fallbacks` counts the members that still took np.load);
    pickles written with a chunk index (`write_npz_files(chunk_index=True)`) are inflated one wavefront per chunk there.
    `transform` is the dictionary `get_transforms` returns: RGB / Flow need a
    `DevicePipeline`; the Audio entry is not called, the spectrograms are born on the device as the fp32 tensor it would
    return.
    `action_list` (the reference's `EpicClasses` filter) raises here; `core.tools.vis.create_dataset` applies it."""

    def __init__(self, cfg, vid_list, annotation_file, modality=["RGB"], transform=None, mode="train", action_list=None,
                 *, device="cuda", threads=8, entropy="host", audio_cache_bytes=4 << 30, audio_load="host",
                 flow_load="host", inflate="host"):
        import pandas as pd
        if action_list is not None and len(action_list) > 0:
            raise NotImplementedError("Video_Dataset: action_list needs the reference's EpicClasses verb / noun tables, "
                                      "which are out of scope here")
        if mode not in ("train", "val", "test"):
            raise ValueError(f"Video_Dataset: unknown mode {mode!r}")
        if audio_load not in ("host", "device"):
            raise ValueError(f"Video_Dataset: audio_load={audio_load!r} is not 'host' or 'device'")
        if flow_load not in ("host", "device"):
            raise ValueError(f"Video_Dataset: flow_load={flow_load!r} is not 'host' or 'device'")
        self.flow_load, self.flow_fallbacks = flow_load, 0
        self.cfg = cfg
        self.root_dir = cfg.data_dir
        self.rgb_prefix, self.flow_prefix = cfg.data.rgb.dir_prefix, cfg.data.flow.dir_prefix
        self.audio_prefix = cfg.data.audio.dir_prefix
        self.vis_file_ext, self.aud_file_ext = cfg.data.rgb.file_ext, cfg.data.audio.file_ext
        self.aud_sampling_rate = cfg.data.audio.sampling_rate
        self.modality, self.mode = list(modality), mode
        self.read_flow_pickle = cfg.data.flow.read_flow_pickle
        self.read_audio_pickle = cfg.data.audio.read_audio_pickle
        self.use_attention = cfg.model.attention.enable
        self.transform = transform if transform is not None else {}
        self.num_segments = {"train": cfg.train.num_segments, "val": cfg.val.num_segments,
                             "test": cfg.test.num_segments}[mode]
        self.frame_len = {m: (cfg.data.flow.win_length if m == "Flow" else 1) for m in self.modality}
        for m in self.modality:
            if m not in ("RGB", "Flow", "Audio"):
                raise ValueError(f"Video_Dataset: unknown modality {m!r}")
            if m != "Audio" and not isinstance(self.transform.get(m), DevicePipeline):
                raise TypeError(f"Video_Dataset: transform[{m!r}] must be a DevicePipeline (get_transforms makes one); "
                                "the batch is transformed by one kernel launch, not sample by sample")
        path = os.path.join(self.root_dir, annotation_file)
        if annotation_file.endswith("csv"):
            self.annotations = pd.read_csv(path)
        elif annotation_file.endswith("pkl"):
            self.annotations = pd.read_pickle(path)
        else:
            raise ValueError(f"Video_Dataset: annotation file {annotation_file!r} is neither .csv nor .pkl")
        if vid_list:
            self.annotations = self.annotations[self.annotations["video_id"].isin(list(vid_list))]
        self.device = torch.device(device)
        if entropy not in ("host", "device"):
            raise ValueError(f"Video_Dataset: entropy={entropy!r} is not 'host' or 'device'")
        if inflate not in ("host", "device"):
            raise ValueError(f"Video_Dataset: inflate={inflate!r} is not 'host' or 'device'")
        self.threads, self.entropy, self.inflate = threads, entropy, inflate
        if audio_load == "device" and "Audio" in self.modality and not self.read_audio_pickle \
                and str(self.aud_file_ext).lower() != "wav":
            raise ValueError(f"Video_Dataset: audio_load='device' reads .wav files, data.audio.file_ext is "
                             f"{self.aud_file_ext!r} (compressed audio is out of scope)")
        self.audio_load = audio_load
        self.audio_cache_bytes = int(audio_cache_bytes)
        self._waves, self._wave_bytes = OrderedDict(), 0
        self._audio = None

    def __len__(self):
        return self.annotations.shape[0]

    # ------------------------------------------------------------------ the host half: record a batch
    def _frame_files(self, m, vid_id, indices):
        """the files of one clip and modality in frame order (reference dataset.py:166-177, 302-370)"""
        if m == "RGB":
            d = os.path.join(self.root_dir, self.rgb_prefix, vid_id)
            return [os.path.join(d, "img_{:010d}.{}".format(int(i), self.vis_file_ext)) for i in indices]
        d = os.path.join(self.root_dir, self.flow_prefix, vid_id)
        if self.read_flow_pickle:
            return [os.path.join(d, "frame_{:010d}.npz".format(int(i))) for i in indices]
        L = self.frame_len[m]
        frames = (indices.repeat(L) + np.tile(np.arange(L), self.num_segments)).astype(np.int64)
        return [os.path.join(d, "{}_{:010d}.{}".format(axis, int(i), self.vis_file_ext)) for i in frames
                for axis in ("x", "y")]

    @staticmethod
    def _read_flow_pickle(path):
        try:
            with np.load(path) as z:
                flow = np.asarray(z["flow"])
        except Exception as e:
            raise Exception("Failed to load flow file {} with error {}.".format(path, e))
        if flow.dtype != np.uint8 or flow.ndim != 3:
            raise Exception(f"Failed to load flow file {path} with error: 'flow' is {flow.dtype} {flow.shape}, expected "
                            "uint8 (H, W, 2 * win_length).")
        return np.ascontiguousarray(flow.transpose(2, 0, 1))[:, :, :, None]      # channel c = gray frame c

    def _read_flow_pickle_records(self, paths):
        """flow_load="device": the bytes of every pickle and its `npz_member` record; nothing is inflated here.  The frame
        size `plan` needs comes from the record; a member the record sends to the host is read by `_read_flow_pickle` at
        once (its size has to come from somewhere, and whatever it raises is the host path's message)."""
        blobs, records, shapes = [], [], []
        for p in paths:
            try:
                with open(p, "rb") as f:
                    blob = f.read()
                record = npz_member(blob)
            except Exception as e:
                raise Exception("Failed to load flow file {} with error {}.".format(p, e))
            if record.host:
                planes = self._read_flow_pickle(p)                 # (C, H, W, 1)
                shapes.append((int(planes.shape[1]), int(planes.shape[2]), int(planes.shape[0])))
            else:
                shapes.append(tuple(int(v) for v in record.shape))
            blobs.append(blob)
            records.append(record)
        for p, shape in zip(paths, shapes):
            if shape[:2] != shapes[0][:2]:
                raise TbnHipError(f"Video_Dataset: the flow pickles of one clip differ in size: {paths[0]} is "
                                  f"{shapes[0][1]}x{shapes[0][0]}, {p} is {shape[1]}x{shape[0]}")
        hw = shapes[0][:2]
        v = _Visual(paths, blobs, None, ("npz",) + hw, hw, None, None, records)
        v.shapes = shapes
        return v

    def _inflate_pickles(self, visuals):
        """every pickle of a launch group -> uint8 (n_img, H, W, 1) on the device: one `load_npz_arrays` call per run of
        files of one (H, W, C) -- one call for a dataset written with one win_length"""
        paths = [p for v in visuals for p in v.paths]
        blobs = [b for v in visuals for b in v.blobs]
        records = [r for v in visuals for r in v.records]
        shapes = [s for v in visuals for s in v.shapes]
        parts, first = [], 0
        while first < len(paths):
            last = first
            while last < len(paths) and shapes[last] == shapes[first]:
                last += 1

            def host_read(i, first=first):
                return self._read_flow_pickle(paths[first + i])[:, :, :, 0].transpose(1, 2, 0)

            planes, statuses = load_npz_arrays(blobs[first:last], device=self.device, records=records[first:last], planes=True,
                                               host_read=host_read)
            self.flow_fallbacks += sum(1 for s in statuses if s != 0)
            parts.append(planes)
            first = last
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    def _read_visual(self, m, vid_id, indices):
        paths = self._frame_files(m, vid_id, indices)
        if m == "Flow" and self.read_flow_pickle and self.flow_load == "device":
            return self._read_flow_pickle_records(paths)
        if m == "Flow" and self.read_flow_pickle:
            arrays = np.concatenate([self._read_flow_pickle(p) for p in paths], 0)
            hw = (int(arrays.shape[1]), int(arrays.shape[2]))
            return _Visual(paths, None, arrays, ("npz",) + hw, hw, None, None)
        blobs = [FrameReader._read(p) for p in paths]
        keys = [geometry_key(png_geometry(b) if is_png(b) else jpeg_geometry(b)) for b in blobs]
        for p, k in zip(paths, keys):
            if k[:2] != keys[0][:2]:
                raise TbnHipError(f"Video_Dataset: the frames of one clip differ in size: {paths[0]} is "
                                  f"{keys[0][0]}x{keys[0][1]}, {p} is {k[0]}x{k[1]}")
        hw = (keys[0][1], keys[0][0])
        return _Visual(paths, blobs, None, ("jpg",) + hw, hw, None, keys)

    def _frame_size(self, m, vid_id, indices):
        """the source frame size (H, W) of a clip that is not kept, from ONE file's header: the first JPEG's frame header,
        or the first pickle's `npz_member` record (the member itself only when the record sends it to the host)"""
        path = self._frame_files(m, vid_id, indices)[0]         # names only: nothing is opened
        if m == "Flow" and self.read_flow_pickle:
            try:
                with open(path, "rb") as f:
                    record = npz_member(f.read())
            except Exception as e:
                raise Exception("Failed to load flow file {} with error {}.".format(path, e))
            if record.host:
                planes = self._read_flow_pickle(path)
                return (int(planes.shape[1]), int(planes.shape[2]))
            return tuple(int(v) for v in record.shape[:2])
        if str(self.vis_file_ext).lower() == "png":          # a PNG needs only its first 33 bytes; anything else in a
            try:                                             # .png file is a JPEG's business, as cv2.imread reads by content
                with open(path, "rb") as f:
                    head = f.read(PNG_HEADER_BYTES)
            except OSError:
                raise Exception(f"Problem reading file {path}")
            if is_png(head):
                return png_frame_size(head)
        return jpeg_frame_size(path)

    def plan(self, indices, rng=None, keep=None):
        """The host half of `batch`: for every clip, in order, and every modality, in order, the segment indices (when
        that modality draws any) and THEN that modality's transform geometry -- the draw order of the reference's
        `__getitem__` (dataset.py:157-178) called clip after clip, under data.sampling "sync" and "async" alike.  Reads
        the frame files (the geometry needs the frame size) but touches no GPU.  Returns one record per clip with
        `.indices[m]`, `.visual[m].paths` and `.visual[m].geo`.  Every draw comes from `rng` (a `np.random.RandomState`);
        None: from the global `np.random`, the same calls in the same order.

        `keep` (positions into `indices`; None: all of them) names the clips this caller goes on to decode -- a rank's
        share of a global batch (`ClipLoader(shard=)`).  EVERY draw is still made for EVERY clip, in the same order, so
        the generator leaves in the state it would without `keep`; of a clip outside `keep` only the frame size the
        transform's draw needs is read (`_frame_size`: one JPEG header or one `npz_member` record per visual modality,
        no audio), its record carries `.kept = False` and `.visual[m]` without files."""
        draw = np.random if rng is None else rng
        keep = None if keep is None else {int(k) for k in keep}
        if keep is not None and not keep <= set(range(len(indices))):
            raise ValueError(f"Video_Dataset.plan: keep {sorted(keep)} is not within the {len(indices)} clips")
        clips = []
        for pos, i in enumerate(indices):
            clip = _Clip(EpicVideoRecord(self.annotations.iloc[int(i)]))
            clip.kept = keep is None or pos in keep
            first, num = clip.record.start_frame, clip.record.num_frames
            for m_no, m in enumerate(self.modality):
                if m_no > 0 and self.cfg.data.sampling == "sync":
                    idx = clip.indices[self.modality[0]]
                    clip.indices[m] = (idx / 2).astype(np.int64) if m == "Flow" else idx
                else:
                    clip.indices[m] = get_offsets(first[m], num[m], m, self.mode, self.num_segments, self.frame_len[m],
                                                  rng=draw)
                if m != "Audio":
                    if clip.kept:
                        v = self._read_visual(m, clip.vid_id, clip.indices[m])
                    else:
                        hw = self._frame_size(m, clip.vid_id, clip.indices[m])
                        v = _Visual(None, None, None, None, hw, None, None)
                    v.geo = self.transform[m]._record(*v.hw, rng=rng)
                    clip.visual[m] = v
            clips.append(clip)
        return clips

    # ------------------------------------------------------------------ the device half
    def _visual_batch(self, m, clips):
        """one decode per geometry group, one launch per group, every clip with its own recorded geometry"""
        order = OrderedDict()
        for b, clip in enumerate(clips):
            order.setdefault(clip.visual[m].key, []).append(b)
        groups = []
        for key, part in order.items():
            if key[0] == "npz" and self.flow_load == "device":
                groups.append(self._inflate_pickles([clips[b].visual[m] for b in part]))
            elif key[0] == "npz":
                arr = np.concatenate([clips[b].visual[m].arrays for b in part], 0)
                groups.append(torch.from_numpy(arr).to(self.device, non_blocking=True))
            else:
                blobs = [blob for b in part for blob in clips[b].visual[m].blobs]
                keys = [k for b in part for k in clips[b].visual[m].file_keys]
                groups.append(self._decode(blobs, keys, gray=(m == "Flow")))
        return self.transform[m]._run_batch(groups, list(order.values()), [clip.visual[m].geo for clip in clips])

    def _decode(self, blobs, keys, gray):
        """files of one frame size -> uint8 (n, H, W, C): ONE `decode_jpegs` call when they share components and
        sampling (a dataset written by one encoder does); otherwise one call per kind, scattered into place.  A kind of
        PNG files (`geometry_key`: "png" in third place) goes through `decode_pngs` instead."""
        kinds = OrderedDict()
        for i, k in enumerate(keys):
            kinds.setdefault(k, []).append(i)
        kw = dict(gray=gray, device=self.device, threads=self.threads, entropy=self.entropy)
        png_kw = dict(gray=gray, device=self.device, threads=self.threads, inflate=self.inflate)

        def decode(kind, part):
            return decode_pngs(part, **png_kw) if kind[2] == "png" else decode_jpegs(part, **kw)

        if len(kinds) == 1:
            return decode(keys[0], blobs)
        frames = None
        for kind, where in kinds.items():
            part = decode(kind, [blobs[i] for i in where])
            if frames is None:
                frames = torch.empty((len(blobs),) + tuple(part.shape[1:]), dtype=torch.uint8, device=self.device)
            frames.index_copy_(0, torch.tensor(where, device=self.device), part)
        return frames

    def _waveform(self, vid_id):
        """the untrimmed waveform of a video on the device; least recently used ones leave when the cap is passed"""
        if vid_id in self._waves:
            self._waves.move_to_end(vid_id)
            return self._waves[vid_id]
        if self.read_audio_pickle:
            path = os.path.join(self.root_dir, self.audio_prefix, "{}.npy".format(vid_id))
            try:
                sample = np.load(path)
            except Exception as e:
                raise Exception("Failed to read audio sample {} with error {}".format(path, e))
        else:
            path = os.path.join(self.root_dir, self.audio_prefix, "{}.{}".format(vid_id, self.aud_file_ext))
            try:
                sample = (load_audio(path, self.aud_sampling_rate, device=self.device) if self.audio_load == "device"
                          else read_wav(path, self.aud_sampling_rate))
            except Exception as e:
                raise Exception("Failed to read audio sample {} with error {}".format(path, e))
        if torch.is_tensor(sample):
            wave_dev = sample
        else:
            wave_dev = torch.from_numpy(np.ascontiguousarray(sample, dtype=np.float32).reshape(-1)).to(self.device)
        size = wave_dev.numel() * 4
        if size <= self.audio_cache_bytes:
            self._waves[vid_id] = wave_dev
            self._wave_bytes += size
            while self._wave_bytes > self.audio_cache_bytes:
                _, old = self._waves.popitem(last=False)
                self._wave_bytes -= old.numel() * 4
        return wave_dev

    def _audio_batch(self, clips):
        if self._audio is None:
            self._audio = AudioSegments.from_config(self.cfg)
        waves = [self._waveform(clip.vid_id) for clip in clips]
        return self._audio(waves, np.stack([clip.indices["Audio"] for clip in clips], 0))

    def batch(self, indices, rng=None, keep=None):
        """`(data, target)` in train mode, `(data, target, action_id)` otherwise: what `default_collate` makes of the
        reference's items `[dataset[i] for i in indices]`, already on the device --
          data[m]            (B, n, C, H, W) fp32 per modality;
          data["indices"][m] (B, n) int64;  data["vid_id"], data["start_time"], data["stop_time"]: lists;
          data["weights"]    (B, n, T, 1) with attention and use_fixed; target["weights"] with attention and use_prior;
          target["class"]    {"verb", "noun"}: int64 (B,), or an int64 (B,) of -1 when the label columns are missing;
          action_id          int64 (B,) when the uids are integers, else a list.
        `rng`, `keep`: handed to `plan`.  With `keep` (positions into `indices`) the batch holds the kept clips only, in
        their order, while the generator advances as for the whole of `indices`; an empty `keep` makes the draws and
        returns None."""
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("Video_Dataset.batch: no indices")
        att = self.cfg.model.attention
        wants_weights = self.use_attention and (att.use_fixed or att.use_prior)
        if wants_weights and "Audio" not in self.modality:
            raise ValueError("Video_Dataset: the attention weights come from the Audio modality, which is not enabled")
        clips = self.plan(indices, rng, keep)
        if keep is not None:
            clips = [clip for clip in clips if clip.kept]
            if not clips:
                return None
        data, target = OrderedDict(), OrderedDict()
        data["vid_id"] = [clip.vid_id for clip in clips]
        data["start_time"] = [clip.record.start_time for clip in clips]
        data["stop_time"] = [clip.record.stop_time for clip in clips]
        weights = None
        for m in self.modality:
            if m == "Audio":
                out = self._audio_batch(clips)
                data[m], weights = out["Audio"], out.get("weights")
            else:
                data[m] = self._visual_batch(m, clips)
        data["indices"] = OrderedDict(
            (m, torch.from_numpy(np.stack([clip.indices[m] for clip in clips], 0).astype(np.int64)).to(self.device))
            for m in self.modality)
        labels = [clip.record.label for clip in clips]
        if isinstance(labels[0], dict):
            target["class"] = {k: torch.tensor([int(lab[k]) for lab in labels], dtype=torch.int64, device=self.device)
                               for k in labels[0]}
        else:
            target["class"] = torch.tensor([int(lab) for lab in labels], dtype=torch.int64, device=self.device)
        if self.use_attention:
            if att.use_fixed:
                data["weights"] = weights
            elif att.use_prior:
                target["weights"] = weights
        if self.mode == "train":
            return data, target
        ids = [clip.record.action_id for clip in clips]
        if all(isinstance(u, (int, np.integer)) for u in ids):
            ids = torch.tensor([int(u) for u in ids], dtype=torch.int64, device=self.device)
        return data, target, ids

    def __getitem__(self, index):
        """the reference's item: `batch([index])` with the batch dimension removed"""
        def first(v):
            if isinstance(v, dict):
                return type(v)((k, first(x)) for k, x in v.items())
            return v[0]
        return tuple(first(part) for part in self.batch([index]))
