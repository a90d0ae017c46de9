"""The audio side of the reference data layer on the device (`core/dataset/dataset.py:421-575`: `_get_audio_segment`,
`_get_spectrogram`, `_get_attn_weights`): untrimmed waveforms on the GPU in, the model's `"Audio"` input and `"weights"`
prior out, with no host round trip of audio or spectrograms and no vendor-library kernel in between.

  window cut   the table of window starts is host arithmetic (`audio_windows`, the reference's own clamps); it goes to the
               device as one copy of nseg 64-bit addresses and the STFT kernel reads each window where it lies in its
               clip (`tbn_stft_windows`) -- clips are never sliced, stacked or concatenated;
  spectrogram  `spec_type="stft"`: one launch; `"logms"`: the STFT writing |X|^2 + one mel / dB kernel;
  prior        `"loud"`: one launch, one wave per segment (`tbn_attn_prior_loud`), bit-equal to the host
               `attention_prior`; `"gaussian"` / `"uniform"`: a broadcast of the host function's constant vector.
"""
import numpy as np
import torch

from ..._lib import call, ptr, stream_ptr, TbnHipError
from .prior import attention_prior, gaussian_kernel
from .spectrogram import Spectrogram, STFT_LOGMEL, STFT_LOGPOWER  # noqa: F401


def audio_windows(clip_lengths, frame_idx, audio_length, sampling_rate=24000, vid_fps=60):
    """`trim_audio_window` for B clips x n frames at once: clip_lengths (B,) samples per clip, frame_idx (B, n) centre
    frames -> (starts (B, n) int64, length).  Element for element what the scalar function returns -- the same IEEE
    double operations in the same order (frame / fps, minus half the window, times the rate, truncated) and the same
    clamps, so a clip shorter than the window gets its NEGATIVE start here too (reference dataset.py:441-451)."""
    length = int(audio_length * sampling_rate)
    n_samples = np.asarray(clip_lengths, dtype=np.int64).reshape(-1, 1)
    frames = np.asarray(frame_idx)
    if frames.ndim != 2 or frames.shape[0] != n_samples.shape[0]:
        raise ValueError(f"audio_windows: frame_idx {frames.shape} does not match {n_samples.shape[0]} clips")
    start_sec = frames.astype(np.float64) / np.float64(vid_fps) - (audio_length / 2)
    starts = np.maximum(0.0, start_sec * np.float64(sampling_rate)).astype(np.int64)     # int(): truncation
    starts = np.where(starts + length > n_samples, n_samples - length, starts)
    return starts, length


def window_table(clips, starts, length):
    """The device addresses of the windows `clips[b][starts[b, j] : starts[b, j] + length]`, (B * n,) int64 on the host --
    after refusing everything the kernel must never see: it reads `length` samples from each address unchecked against
    the clip, so a window that leaves its clip, or a clip that is not a contiguous float32 device vector, raises here,
    before any launch.  A clip shorter than the window is the reference's empty sample (dataset.py:441-451): ValueError,
    like `Spectrogram` raises for it."""
    starts = np.asarray(starts, dtype=np.int64)
    if starts.ndim != 2 or starts.shape[0] != len(clips):
        raise TbnHipError(f"window_table: starts {starts.shape} for {len(clips)} clips")
    table = np.empty(starts.shape, dtype=np.int64)
    for b, clip in enumerate(clips):
        if not getattr(clip, "is_cuda", False):
            raise TbnHipError(f"window_table: clip {b} is not on the GPU (the STFT kernel reads device memory, no CPU fallback)")
        if clip.dtype != torch.float32 or clip.dim() != 1 or not clip.is_contiguous():
            raise TbnHipError(f"window_table: clip {b} must be a contiguous 1-D float32 tensor "
                              f"(got {clip.dtype}, shape {tuple(clip.shape)})")
        n = int(clip.shape[0])
        if n < length:
            raise ValueError(f"AudioSegments: empty audio sample (clip {b} has {n} samples, shorter than the window of "
                             f"{length}, reference dataset.py:441-451)")
        if (starts[b] < 0).any() or (starts[b] + length > n).any():
            raise TbnHipError(f"window_table: a window of clip {b} ({n} samples) leaves the clip: starts "
                              f"{starts[b].tolist()}, length {length}")
        table[b] = clip.data_ptr() + 4 * starts[b]
    return table.reshape(-1)


class AudioSegments:
    """`out = AudioSegments(audio_length, ...)(clips, frame_idx)`: clips = B untrimmed 1-D float32 GPU waveforms,
    frame_idx (B, n) centre frames of the segments ->
      out["Audio"]    (B, n, 1, F, W) float32, F = 256 (`stft`) or 128 (`logms`): `TBNModel.forward`'s input["Audio"];
      out["weights"]  (B, n, T, 1) float32 when `prior_type` is set, T = round(audio_length * 25 / 4): the reference's
                      input["weights"] / target["weights"].
    Loud prior: ties between block maxima take the highest block index -- NumPy's `argsort()[-1]` for up to 16 blocks;
    for more blocks NumPy's order among EXACT ties is an implementation detail of its sort, the device rule stays."""

    def __init__(self, audio_length, sampling_rate=24000, vid_fps=60, spec_type="stft", prior_type=None, eps=1e-6):
        if prior_type not in (None, "gaussian", "uniform", "loud"):
            raise ValueError(f"unknown attention prior '{prior_type}'")
        self.audio_length = audio_length
        self.sampling_rate = sampling_rate
        self.vid_fps = vid_fps
        self.prior_type = prior_type
        self.spectrogram = Spectrogram(eps=eps, spec_type=spec_type, sampling_rate=sampling_rate)
        self._prior = {}

    @classmethod
    def from_config(cls, cfg):
        """data.audio.{audio_length,sampling_rate,spec_type}, data.vid_fps; the prior only when the attention is enabled
        (model.attention.{enable,prior_type}; the reference builds the weights under the same condition, dataset.py:68,
        174-187, and hands them to the model as input["weights"] (use_fixed) or target["weights"] (use_prior))"""
        att = cfg.model.attention
        return cls(cfg.data.audio.audio_length, cfg.data.audio.sampling_rate, cfg.data.vid_fps, cfg.data.audio.spec_type,
                   att.prior_type if att.enable else None)

    @property
    def num_weights(self):
        return round(self.audio_length * (25 / 4))

    def _constant(self, device, kind):
        """host-computed (T,) float32 vectors on the device: the Gaussian the loud kernel selects from, or a whole prior"""
        if (device, kind) not in self._prior:
            T = self.num_weights
            host = (torch.tensor(gaussian_kernel(T, 1)).float() if kind == "loud"
                    else attention_prior(None, self.audio_length, kind))
            self._prior[(device, kind)] = host.reshape(T).to(device)
        return self._prior[(device, kind)]

    def prior(self, spec):
        """spec (nseg, F, W) on the device -> (nseg, T, 1)"""
        nseg, F, W = spec.shape
        T = self.num_weights
        if self.prior_type != "loud":
            return self._constant(spec.device, self.prior_type).view(1, T, 1).expand(nseg, T, 1).contiguous()
        if W < T:       # the host function indexes an empty argsort here
            raise ValueError(f"AudioSegments: no full block of {T} frames in a spectrogram {W} frames wide")
        out = torch.empty(nseg, T, 1, device=spec.device, dtype=torch.float32)
        call("tbn_attn_prior_loud", ptr(spec), nseg, F, W, T, ptr(self._constant(spec.device, "loud")), ptr(out),
             stream_ptr())
        return out

    def __call__(self, clips, frame_idx):
        clips = list(clips)
        frames = np.asarray(frame_idx.cpu() if torch.is_tensor(frame_idx) else frame_idx)
        starts, length = audio_windows([int(c.shape[0]) for c in clips], frames, self.audio_length, self.sampling_rate,
                                       self.vid_fps)
        table = window_table(clips, starts, length)
        device = clips[0].device
        if any(c.device != device for c in clips):
            raise TbnHipError("AudioSegments: the clips of one call must live on one device")
        B, n = starts.shape
        with torch.cuda.device(device):
            windows = torch.from_numpy(table).to(device)         # the one host-to-device copy: B * n addresses
            spec = self.spectrogram.windows(windows, None, B * n, length, device)
            out = {"Audio": spec.view(B, n, 1, spec.shape[1], spec.shape[2])}
            if self.prior_type is not None:
                out["weights"] = self.prior(spec).view(B, n, self.num_weights, 1)
        return out
