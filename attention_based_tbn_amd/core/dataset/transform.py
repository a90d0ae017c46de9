"""Visual input pipeline on the MI355X (reference `core/dataset/transform.py:9-543`, composed by
`core/utils/create_dataloader.py:19-81`).

The reference transforms a Python list of uint8 HxWxC frames on the host, image by image (crop, `cv2.resize`, flip,
stack, `/255`, normalise) and ships fp32 tensors to the GPU.  Here every transform only *records* its decision
(same constructor arguments, same NumPy RNG draws in the same order, so a seeded run picks the same crop box and
flip); the pixels move to the device as uint8 (4x fewer PCIe bytes) and ONE HIP kernel (`tbn_frames_to_tensor`)
produces the normalised fp32 NCHW tensor.  `get_transforms(cfg, modality, mode)` returns the same dictionary of
callables as the reference.  No CPU fallback: the pipeline raises without a GPU.  `DevicePipeline.batch` does the
same for every clip of a batch in one launch (`tbn_frames_to_tensor_batch`), one recorded geometry per clip.

`FixedCrop` (the reference's multi-crop test-time augmentation) records a list of windows; the pipeline then calls
`tbn_frames_to_tensor_crops`, one launch for all of them.  The reference's own compositions (`core/tools/test.py:136-171`:
`Compose([Rescale, CenterCrop or FixedCrop, Stack, ToTensor, Normalize])`) work as well: given a list of frames
instead of a `_Geometry`, a geometry class returns a recorded sample that the next transform takes; `ToTensor` runs
the kernel and `Normalize` finishes on the device, bit for bit what the fused `DevicePipeline` gives.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from ..._lib import FramesClip, TbnHipError, call, ptr, stream_ptr


class _Geometry:
    """what the recorded transforms do to a frame of (h, w): source box -> resized size -> crop window -> flip.
    `rng` is what the random transforms recorded into it draw from (`randint`, `random`): the global `np.random` module,
    or a `np.random.RandomState` of the caller's."""

    def __init__(self, h, w, rng=None):
        self.rng = np.random if rng is None else rng
        self.src_h, self.src_w = h, w   # the frames the geometry was recorded for
        self.h, self.w = h, w           # current logical size
        self.box = [0, 0, w, h]         # x, y, w, h in the SOURCE frame (only valid before a resize)
        self.resized = None             # (w, h) once a resize happened
        self.crop = None                # x, y, w, h inside the resized box
        self.flip = False
        self.windows = None             # FixedCrop: [(x, y)] inside the resized box (the source box without a resize)
        self.mirror_pairs = False       # FixedCrop(horizontal_flip=True): every window is followed by its mirror image

    def _open(self, what):
        if self.windows is not None:
            raise TbnHipError(f"input pipeline: {what} after FixedCrop -- FixedCrop is the last geometry transform of "
                              "a pipeline (one launch takes every window from one resized box)")

    def do_flip(self):
        self._open("a flip")
        self.flip = not self.flip

    def do_windows(self, origins, w, h, mirror_pairs):
        """FixedCrop: `origins` are (x, y) in the current logical frame; all windows are w x h"""
        self._open("a second FixedCrop")
        for x, y in origins:
            if x < 0 or y < 0 or x + w > self.w or y + h > self.h:
                raise TbnHipError(f"input pipeline: FixedCrop window ({x},{y},{w},{h}) outside the {self.w}x{self.h} frame")
        if self.flip:        # the frames were mirrored beforehand: window x of the mirrored frame, seen from the source
            origins = [(self.w - x - w, y) for x, y in origins]
        ox, oy = (self.crop[0], self.crop[1]) if self.crop is not None else (0, 0)
        self.windows = [(ox + x, oy + y) for x, y in origins]
        self.mirror_pairs = bool(mirror_pairs)
        self.w, self.h = w, h

    @property
    def mirror(self):
        """mirror mode of tbn_frames_to_tensor_crops (include/tbn_hip.h)"""
        if self.mirror_pairs:
            return 3 if self.flip else 2
        return 1 if self.flip else 0

    def do_crop(self, x, y, w, h):
        self._open("a crop")
        if self.resized is None:
            self.box = [self.box[0] + x, self.box[1] + y, w, h]
        else:
            c = self.crop or [0, 0, self.resized[0], self.resized[1]]
            self.crop = [c[0] + x, c[1] + y, w, h]
        self.w, self.h = w, h

    def do_resize(self, new_w, new_h):
        self._open("a resize")
        if self.resized is not None:
            raise TbnHipError("input pipeline: at most one resize per pipeline (as in the reference's compositions)")
        if (new_h, new_w) != (self.h, self.w):
            self.resized = (new_w, new_h)
            self.w, self.h = new_w, new_h


class _Recorded:
    """what the reference-style chain passes along: the untouched uint8 frames of one sample, the geometry recorded so
    far and, after `Stack`, the modality and stack length"""

    def __init__(self, frames, geo):
        self.frames, self.geo = frames, geo
        self.modality, self.length = None, None


def _frame_hw(frames):
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4:
            raise TbnHipError(f"input pipeline: expected frames (n, H, W, C), got {tuple(frames.shape)}")
        return int(frames.shape[1]), int(frames.shape[2])
    if not (isinstance(frames, list) and len(frames) > 0):
        raise TbnHipError("input pipeline: expected a non-empty list of uint8 frames or a uint8 tensor (n, H, W, C)")
    return int(frames[0].shape[0]), int(frames[0].shape[1])


class _GeometryTransform(object):
    """Called with a `_Geometry` a geometry transform records into it; called with the reference's argument (a list of
    uint8 frames, or a uint8 tensor (n, H, W, C)) or with the recorded sample an earlier transform returned, it
    records into that sample's geometry and returns the sample."""

    def __call__(self, x):
        if isinstance(x, _Geometry):
            self.record(x)
            return x
        if not isinstance(x, _Recorded):
            x = _Recorded(x, _Geometry(*_frame_hw(x)))
        self.record(x.geo)
        return x


class MultiScaleCrop(_GeometryTransform):
    """reference transform.py:284-413 -- same constructor, same two `np.random.randint` draws"""

    def __init__(self, input_size, scales=[1, 0.875, 0.75, 0.66], max_distort=1, fix_crop=True, more_fix_crop=True):
        self.scales, self.max_distort, self.fix_crop, self.more_fix_crop = scales, max_distort, fix_crop, more_fix_crop
        assert isinstance(input_size, (int, tuple))
        self.input_size = input_size if isinstance(input_size, tuple) else (input_size, input_size)

    def record(self, geo):
        crop_w, crop_h, off_w, off_h = self._sample_crop_size((geo.h, geo.w), geo.rng)
        geo.do_crop(off_w, off_h, crop_w, crop_h)
        Rescale(self.input_size).record(geo)

    def _sample_crop_size(self, im_size, rng=np.random):
        img_h, img_w = im_size[0], im_size[1]
        base_size = min(img_w, img_h)
        crop_sizes = [int(base_size * x) for x in self.scales]
        crop_h = [self.input_size[1] if abs(x - self.input_size[1]) < 3 else x for x in crop_sizes]
        crop_w = [self.input_size[0] if abs(x - self.input_size[0]) < 3 else x for x in crop_sizes]
        pairs = [(w, h) for i, h in enumerate(crop_h) for j, w in enumerate(crop_w) if abs(i - j) <= self.max_distort]
        crop_pair = pairs[rng.randint(len(pairs))]
        if not self.fix_crop:
            w_offset = rng.randint(0, img_w - crop_pair[0])
            h_offset = rng.randint(0, img_h - crop_pair[1])
        else:
            offsets = self.fill_fix_offset(self.more_fix_crop, img_w, img_h, crop_pair[0], crop_pair[1])
            w_offset, h_offset = offsets[rng.randint(len(offsets))]
        return crop_pair[0], crop_pair[1], int(w_offset), int(h_offset)

    @staticmethod
    def fill_fix_offset(more_fix_crop, image_w, image_h, crop_w, crop_h):
        w_step, h_step = (image_w - crop_w) / 4, (image_h - crop_h) / 4
        ret = [(0, 0), (4 * w_step, 0), (0, 4 * h_step), (4 * w_step, 4 * h_step), (2 * w_step, 2 * h_step)]
        if more_fix_crop:
            ret += [(0, 2 * h_step), (4 * w_step, 2 * h_step), (2 * w_step, 4 * h_step), (2 * w_step, 0 * h_step),
                    (1 * w_step, 1 * h_step), (3 * w_step, 1 * h_step), (1 * w_step, 3 * h_step),
                    (3 * w_step, 3 * h_step)]
        return ret


class Rescale(_GeometryTransform):
    """reference transform.py:222-281 (size: int = smaller edge, or (h, w))"""

    def __init__(self, size, interpolation=1):
        assert isinstance(size, (int, tuple))
        self.size = size

    def record(self, geo):
        h, w = geo.h, geo.w
        if isinstance(self.size, int):
            new_h, new_w = (self.size * h / w, self.size) if h > w else (self.size, self.size * w / h)
        else:
            new_h, new_w = self.size
        geo.do_resize(int(new_w), int(new_h))


class CenterCrop(_GeometryTransform):
    """reference transform.py:60-103"""

    def __init__(self, size):
        self.size = (size, size) if isinstance(size, int) else size

    def record(self, geo):
        h, w = self.size
        geo.do_crop((geo.w - w) // 2, (geo.h - h) // 2, w, h)


class FixedCrop(_GeometryTransform):
    """reference transform.py:106-179, the multi-crop test-time augmentation: same constructor.  `locations` lists
    0 = centre (floor division, as CenterCrop), 1 = top left, 2 = top right, 3 = bottom left, 4 = bottom right;
    `size` is an int or (h, w).  With `horizontal_flip` every crop is followed by its mirror image.

    The reference returns a flat list, windows outermost: entry (location * n_img + img) * F + f, F = 2 with
    `horizontal_flip`.  `Stack` then makes `length` consecutive entries one Flow sample, so with `horizontal_flip` a
    Flow stack alternates plain and mirrored images (x0, mirrored x0, y0, mirrored y0, ...): that is what the
    reference computes and what the kernel reproduces.  The output has n_img * len(locations) * F / stack rows,
    location-major; `TBNModel.forward` tiles the audio feature over them (reference model.py:243-248).

    Last geometry transform of a pipeline: a crop, resize or flip recorded after it raises.  A
    `RandomHorizontalFlip` before it mirrors every window.  At most 16 locations per call (kernel design limit)."""

    def __init__(self, size, locations=[0, 1, 2, 3, 4], horizontal_flip=False):
        assert isinstance(size, (int, tuple))
        self.size = (size, size) if isinstance(size, int) else size
        assert len(self.size) == 2
        self.locations = list(locations)
        for loc in self.locations:
            if loc not in (0, 1, 2, 3, 4):
                raise TbnHipError(f"FixedCrop: unknown location {loc!r} (0 centre, 1 top left, 2 top right, "
                                  "3 bottom left, 4 bottom right)")
        if not 1 <= len(self.locations) <= 16:
            raise TbnHipError(f"FixedCrop: {len(self.locations)} locations, 1..16 supported")
        self.horizontal_flip = horizontal_flip

    def windows(self, img_h, img_w):
        """[(x1, y1)] per location for frames of (img_h, img_w)"""
        h, w = self.size
        table = {0: ((img_w - w) // 2, (img_h - h) // 2), 1: (0, 0), 2: (img_w - w, 0), 3: (0, img_h - h),
                 4: (img_w - w, img_h - h)}
        return [table[loc] for loc in self.locations]

    def record(self, geo):
        h, w = self.size
        geo.do_windows(self.windows(geo.h, geo.w), w, h, self.horizontal_flip)


class RandomCrop(_GeometryTransform):
    """reference transform.py:9-57"""

    def __init__(self, size):
        self.size = (size, size) if isinstance(size, int) else size

    def record(self, geo):
        th, tw = self.size
        x1 = geo.rng.randint(0, geo.w - tw)
        y1 = geo.rng.randint(0, geo.h - th)
        if not (geo.w == tw and geo.h == th):
            geo.do_crop(x1, y1, tw, th)


class RandomHorizontalFlip(_GeometryTransform):
    """reference transform.py:182-219 -- one `np.random.random()` draw per sample"""

    def __init__(self, prob=0.5):
        self.prob = prob

    def record(self, geo):
        if geo.rng.random() < self.prob:
            geo.do_flip()
        else:
            geo._open("a flip")


def _frames_to_tensor(img_list, geo, channels, stack, mean, std, div255, device):
    """the one kernel: uint8 frames (the reference's list of HxW(xC) arrays, or a tensor (n, H, W, C)) + recorded
    geometry -> fp32 (rows, C * stack, h, w) on `device`; mean / std None: ToTensor alone"""
    if not torch.cuda.is_available():
        raise TbnHipError("input pipeline: needs an MI355X (no CPU fallback)")
    if isinstance(img_list, torch.Tensor):
        frames = img_list
    else:
        assert isinstance(img_list, list) and len(img_list) > 0
        arr = np.stack([np.asarray(im).reshape(im.shape[0], im.shape[1], channels) for im in img_list], 0)
        frames = torch.from_numpy(np.ascontiguousarray(arr))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != channels:
        raise TbnHipError(f"input pipeline: expected uint8 frames (n, H, W, {channels}), got "
                          f"{frames.dtype} {tuple(frames.shape)}")
    frames = frames.to(device, non_blocking=True).contiguous()
    n, H, W, C = frames.shape
    if (H, W) != (geo.src_h, geo.src_w):
        raise TbnHipError(f"input pipeline: geometry recorded for {geo.src_h}x{geo.src_w} frames, got {H}x{W}")
    rw, rh = geo.resized if geo.resized is not None else (geo.box[2], geo.box[3])
    n_stat = 0 if mean is None else mean.numel()
    if geo.windows is None:
        if n % stack != 0:
            raise TbnHipError(f"input pipeline: {n} frames is not a multiple of the stack length {stack}")
        cx, cy, ow, oh = geo.crop if geo.crop is not None else (0, 0, rw, rh)
        out = torch.empty((n // stack, C * stack, oh, ow), dtype=torch.float32, device=device)
        call("tbn_frames_to_tensor", ptr(frames), n, H, W, C, geo.box[0], geo.box[1], geo.box[2], geo.box[3], rw, rh,
             cx, cy, ow, oh, int(geo.flip), stack, ptr(mean), ptr(std), n_stat, int(div255), ptr(out), stream_ptr())
        return out
    k = len(geo.windows)
    entries = n * k * (2 if geo.mirror_pairs else 1)           # FixedCrop's flat list, which Stack cuts into samples
    if entries % stack != 0:
        raise TbnHipError(f"input pipeline: {entries} crops ({n} frames x {k} windows"
                          f"{' x 2 mirror images' if geo.mirror_pairs else ''}) is not a multiple of the stack "
                          f"length {stack}")
    ow, oh = geo.w, geo.h
    xs = (ctypes.c_int * k)(*[x for x, _ in geo.windows])
    ys = (ctypes.c_int * k)(*[y for _, y in geo.windows])
    out = torch.empty((entries // stack, C * stack, oh, ow), dtype=torch.float32, device=device)
    call("tbn_frames_to_tensor_crops", ptr(frames), n, H, W, C, geo.box[0], geo.box[1], geo.box[2], geo.box[3], rw, rh,
         xs, ys, k, ow, oh, geo.mirror, stack, ptr(mean), ptr(std), n_stat, int(div255), ptr(out), stream_ptr())
    return out


class DevicePipeline(object):
    """A composed visual pipeline: geometry transforms (recorded) + Stack + ToTensor + Normalize (executed by one
    kernel).  Call with the reference's argument -- a list of uint8 HxW(xC) arrays of one sample -- or with a
    uint8 tensor (n_img, H, W, C); returns the fp32 (n_img / stack, C * stack, h, w) tensor on the device."""

    def __init__(self, modality, geometry, mean, std, length=10, device="cuda"):
        self.modality, self.geometry = modality, list(geometry)
        self.stack = length if modality == "Flow" else 1
        self.channels = 3 if modality == "RGB" else 1
        self.device = torch.device(device)
        self.mean = torch.tensor(mean, dtype=torch.float32)
        self.std = torch.tensor(std, dtype=torch.float32)
        self._stat_dev = None

    def _stats(self):
        if self._stat_dev is None:
            self._stat_dev = (self.mean.to(self.device), self.std.to(self.device))
        return self._stat_dev

    def __call__(self, img_list):
        geo = _Geometry(*_frame_hw(img_list))
        for t in self.geometry:
            t(geo)
        mean, std = self._stats()
        return _frames_to_tensor(img_list, geo, self.channels, self.stack, mean, std, True, self.device)

    def _record(self, h, w, rng=None):
        """the recorded geometry of ONE clip of (h, w) frames: the NumPy draws of one `__call__`, no GPU; `rng`: where
        they are drawn from (None: the global generator)"""
        geo = _Geometry(h, w, rng)
        for t in self.geometry:
            t(geo)
        return geo

    def _record_batch(self, sizes, rng=None):
        """sizes: (h, w) per clip, in batch order -> one `_Geometry` per clip, recorded clip after clip: the NumPy draws
        of len(sizes) consecutive `__call__`s.  Host only."""
        return [self._record(int(h), int(w), rng) for h, w in sizes]

    def batch(self, frames, n_clips, clips=None):
        """The clips of a whole batch in one launch (`tbn_frames_to_tensor_batch`): the reference applies
        `_transform_data` once per sample (dataset.py:512-532), each with its own crop box and flip.

        frames   a uint8 tensor (n_clips * imgs_per_clip, H, W, C), or a list of such tensors, one per GROUP of clips
                 that share a source frame size (a batch with two frame sizes: two groups, two launches into the same
                 output);
        clips    with a list: per group, the batch positions of its clips (`[[0, 2], [1]]`), each clip's images
                 consecutive in its group's tensor; default: the groups hold the clips in batch order.
        Returns fp32 (n_clips, imgs_per_clip / stack, C * stack, h, w) on the device.  One geometry is recorded per clip,
        clip after clip in batch order, so the NumPy draws are those of n_clips consecutive `__call__`s, and every row
        equals what `__call__` returns for that clip, bit for bit.

        A pipeline ending in `FixedCrop` (5 / 10-crop testing) has no batched kernel: it loops over the existing
        `tbn_frames_to_tensor_crops` entry, one launch per clip, and stacks the results."""
        groups = list(frames) if isinstance(frames, (list, tuple)) else [frames]
        if n_clips < 1 or not groups:
            raise TbnHipError(f"input pipeline: a batch of {n_clips} clips in {len(groups)} groups")
        for g in groups:
            if not isinstance(g, torch.Tensor) or g.dim() != 4:
                raise TbnHipError("input pipeline: batch() takes uint8 tensors (n, H, W, C)")
        total = sum(int(g.shape[0]) for g in groups)
        if total % n_clips != 0:
            raise TbnHipError(f"input pipeline: {total} frames do not divide into {n_clips} clips")
        per_clip = total // n_clips
        if clips is None:
            clips, first = [], 0
            for g in groups:
                if int(g.shape[0]) % per_clip != 0:
                    raise TbnHipError(f"input pipeline: a group of {int(g.shape[0])} frames for clips of {per_clip}")
                clips.append(list(range(first, first + int(g.shape[0]) // per_clip)))
                first += len(clips[-1])
        if sorted(b for part in clips for b in part) != list(range(n_clips)) or len(clips) != len(groups) or \
                any(len(part) * per_clip != int(g.shape[0]) for part, g in zip(clips, groups)):
            raise TbnHipError(f"input pipeline: the groups {clips} do not hold each of the {n_clips} clips once")
        sizes = [None] * n_clips
        for part, g in zip(clips, groups):
            for b in part:
                sizes[b] = (int(g.shape[1]), int(g.shape[2]))
        return self._run_batch(groups, clips, self._record_batch(sizes))

    def _clip_table(self, geos, clips, per_clip):
        """The geometry table of `tbn_frames_to_tensor_batch` (include/tbn_hip.h tbn_frames_clip), group after group:
        row k is a clip's recorded geometry, its first image inside its group's tensor and its first output row.
        Returns (table, first table row per group, (out_w, out_h)).  Host only."""
        rows_per_clip = per_clip // self.stack
        table = (FramesClip * len(geos))()
        ow = oh = None
        k, starts = 0, []
        for part in clips:
            starts.append(k)
            for slot, b in enumerate(part):
                geo = geos[b]
                rw, rh = geo.resized if geo.resized is not None else (geo.box[2], geo.box[3])
                cx, cy, w, h = geo.crop if geo.crop is not None else (0, 0, rw, rh)
                if ow is None:
                    ow, oh = w, h
                if (w, h) != (ow, oh):
                    raise TbnHipError(f"input pipeline: clip {b} comes out {w}x{h}, clip {clips[0][0]} {ow}x{oh}: the "
                                      "clips of a batch must share one output size")
                table[k] = FramesClip(slot * per_clip, geo.box[0], geo.box[1], geo.box[2], geo.box[3], rw, rh, cx, cy,
                                      int(geo.flip), b * rows_per_clip, 0)
                k += 1
        return table, starts, (ow, oh)

    def _run_batch(self, groups, clips, geos):
        """groups / clips as in `batch`, geos: the recorded `_Geometry` per clip in batch order -> the batch tensor"""
        if not torch.cuda.is_available():
            raise TbnHipError("input pipeline: needs an MI355X (no CPU fallback)")
        n_clips = len(geos)
        per_clip = sum(int(g.shape[0]) for g in groups) // n_clips
        mean, std = self._stats()
        if any(geo.windows is not None for geo in geos):        # FixedCrop: the per-clip multi-window entry, stacked
            rows = [None] * n_clips
            for part, g in zip(clips, groups):
                for slot, b in enumerate(part):
                    rows[b] = _frames_to_tensor(g[slot * per_clip:(slot + 1) * per_clip], geos[b], self.channels,
                                                self.stack, mean, std, True, self.device)
            return torch.stack(rows, 0)
        if per_clip % self.stack != 0:
            raise TbnHipError(f"input pipeline: {per_clip} frames per clip is not a multiple of the stack length "
                              f"{self.stack}")
        rows_per_clip = per_clip // self.stack
        for part, g in zip(clips, groups):
            for b in part:
                if (int(g.shape[1]), int(g.shape[2])) != (geos[b].src_h, geos[b].src_w):
                    raise TbnHipError(f"input pipeline: geometry recorded for {geos[b].src_h}x{geos[b].src_w} frames, "
                                      f"got {int(g.shape[1])}x{int(g.shape[2])}")
        table, starts, (ow, oh) = self._clip_table(geos, clips, per_clip)
        out = torch.empty((n_clips, rows_per_clip, self.channels * self.stack, oh, ow), dtype=torch.float32,
                          device=self.device)
        with torch.cuda.device(self.device):
            # the one copy of the table; every group's launch reads its own rows of it
            table_dev = torch.frombuffer(table, dtype=torch.uint8).to(self.device, non_blocking=False)
            row = ctypes.sizeof(FramesClip)
            for start, part, g in zip(starts, clips, groups):
                if g.dtype != torch.uint8 or g.shape[3] != self.channels:
                    raise TbnHipError(f"input pipeline: expected uint8 frames (n, H, W, {self.channels}), got "
                                      f"{g.dtype} {tuple(g.shape)}")
                g = g.to(self.device, non_blocking=True).contiguous()
                host_rows = ctypes.cast(ctypes.addressof(table) + start * row, ctypes.POINTER(FramesClip))
                call("tbn_frames_to_tensor_batch", ptr(g), int(g.shape[0]), int(g.shape[1]), int(g.shape[2]),
                     self.channels, host_rows, ptr(table_dev) + start * row, len(part), per_clip, ow, oh, self.stack,
                     ptr(mean), ptr(std), mean.numel(), 1, ptr(out), n_clips * rows_per_clip, stream_ptr())
        return out


class AudioToTensor(object):
    """Stack + ToTensor(is_audio=True) of the reference for spectrograms: list of (256, W) arrays -> (n, 1, 256, W)"""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)

    def __call__(self, img_list):
        arr = np.stack([np.asarray(im).reshape(im.shape[0], im.shape[1], 1) for im in img_list], 0)
        return torch.from_numpy(arr).permute(0, 3, 1, 2).contiguous().float().to(self.device, non_blocking=True)


class Stack(object):
    """reference transform.py:415-461 -- same constructor.  RGB / Flow: records the modality and the stack length in
    the sample (Flow: `length` consecutive single-channel images become the channels of one row); the pixels stay
    uint8 until `ToTensor`.  Audio: the spectrograms are not 8-bit images and take no kernel: the list of (H, W)
    arrays becomes the fp32 (n, 1, H, W) device tensor right here, as `AudioToTensor` does."""

    def __init__(self, modality, length=10, device="cuda"):
        self.modality, self.length = modality, length
        self.device = torch.device(device)

    def __call__(self, x):
        if self.modality == "Audio":
            return AudioToTensor(self.device)(x)
        if self.modality not in ("RGB", "Flow"):
            raise TbnHipError(f"Stack: unknown modality {self.modality!r}")
        if not isinstance(x, _Recorded):
            x = _Recorded(x, _Geometry(*_frame_hw(x)))
        x.modality, x.length = self.modality, (self.length if self.modality == "Flow" else 1)
        return x


class ToTensor(object):
    """reference transform.py:464-499 -- same constructor.  Runs the one kernel on a recorded sample: uint8 frames in,
    fp32 (rows, C * stack, h, w) on the device out, `/ 255` unless `is_audio`, no statistics.  An Audio sample is
    already the fp32 NCHW tensor `Stack("Audio")` made and passes through (`is_audio`: nothing is divided)."""

    def __init__(self, is_audio=False, device="cuda"):
        self.is_audio = is_audio
        self.device = torch.device(device)

    def __call__(self, x):
        if isinstance(x, torch.Tensor) and self.is_audio and x.dim() == 4 and x.dtype == torch.float32:
            return x
        if not isinstance(x, _Recorded) or x.modality is None:
            raise TbnHipError("ToTensor: expected the sample Stack(modality) returns (Stack comes first, as in the "
                              "reference's compositions)")
        channels = 3 if x.modality == "RGB" else 1
        return _frames_to_tensor(x.frames, x.geo, channels, x.length, None, None, not self.is_audio, self.device)


class Normalize(object):
    """reference transform.py:502-543 -- same constructor: (x - mean) / std per channel on the fp32 NCHW tensor, mean
    and std repeated over the channels when there are fewer of them.  The same two fp32 operations the kernel's
    table applies in the fused `DevicePipeline`, so the two agree bit for bit."""

    def __init__(self, mean, std):
        self.mean = torch.tensor(list(mean), dtype=torch.float32)
        self.std = torch.tensor(list(std), dtype=torch.float32)

    def __call__(self, tensor):
        if not (isinstance(tensor, torch.Tensor) and tensor.dim() == 4 and tensor.dtype == torch.float32):
            raise TbnHipError("Normalize: expected the fp32 (n, C, h, w) tensor ToTensor returns")
        c = tensor.size(1)
        stats = []
        for v in (self.mean, self.std):
            if v.numel() < c:
                v = v.repeat(c)          # repeat(c), not ceil(c / len): the reference's over-long vector ...
            if v.numel() != c:           # ... then fails to broadcast unless len == 1; say so instead
                raise TbnHipError(f"Normalize: {v.numel()} statistics for {c} channels")
            stats.append(v.to(tensor.device).view(1, c, 1, 1))
        return (tensor - stats[0]) / stats[1]


class TransferTensorDict(object):
    """reference transform.py:546-584 -- same constructor: every tensor of a (nested) dictionary goes to `device`,
    dtype kept (uint8 frames cross PCIe as uint8), `non_blocking=True`; other values are left alone"""

    def __init__(self, device):
        assert isinstance(device, torch.device)
        self.device = device

    def __call__(self, tensor_dict):
        assert isinstance(tensor_dict, dict)
        for key, value in tensor_dict.items():
            if isinstance(value, dict):
                tensor_dict[key] = self(value)
            elif isinstance(value, torch.Tensor):
                tensor_dict[key] = value.to(self.device, non_blocking=True)
        return tensor_dict


def get_transforms(cfg, modality, mode="test", device="cuda", test_crops=1, flow_length=10):
    """reference create_dataloader.py:19-81: the same compositions per modality and mode.  `test_crops` (modes other
    than train): 1 = CenterCrop, 5 = FixedCrop at the centre and the four corners, 10 = the same, each followed by
    its mirror image (the block commented out at reference core/tools/test.py:142-146).  `flow_length`: the images
    `Stack("Flow")` makes one sample of; the reference leaves it at Stack's default of 10 = 2 * win_length at the
    default win_length of 5, `create_dataloader` here passes 2 * cfg.data.flow.win_length."""
    if mode != "train" and test_crops not in (1, 5, 10):
        raise TbnHipError(f"get_transforms: test_crops={test_crops!r}, expected 1, 5 or 10")
    transforms = OrderedDict()
    for m in modality:
        if m in ("RGB", "Flow"):
            node = cfg.data.rgb if m == "RGB" else cfg.data.flow
            if mode == "train":
                scales = [1, 0.875, 0.75, 0.66] if m == "RGB" else [1, 0.875, 0.75]
                geometry = [MultiScaleCrop(cfg.data.train_crop_size, scales), RandomHorizontalFlip(prob=0.5)]
            elif test_crops == 1:
                geometry = [Rescale(cfg.data.test_scale_size), CenterCrop(cfg.data.test_crop_size)]
            else:
                geometry = [Rescale(cfg.data.test_scale_size),
                            FixedCrop(cfg.data.test_crop_size, [0, 1, 2, 3, 4], horizontal_flip=test_crops == 10)]
            transforms[m] = DevicePipeline(m, geometry, list(node.mean), list(node.std), length=flow_length,
                                           device=device)
        elif m == "Audio":
            transforms[m] = AudioToTensor(device)
    return transforms
