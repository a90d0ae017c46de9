"""Log-power STFT spectrogram on the GPU (replaces the per-item CPU librosa call in the
reference's DataLoader workers, core/dataset/dataset.py:461-495) + the audio window trim of
`_get_audio_segment` (:421-459, host integer arithmetic)."""
import numpy as np
import torch

from ..._lib import call, lib, ptr, stream_ptr, TbnHipError


STFT_LOGPOWER, STFT_LOGMEL = 0, 1      # include/tbn_hip.h TBN_STFT_*: the `mode` of tbn_stft_windows


def trim_audio_window(num_samples, frame_idx, audio_length, sampling_rate=24000, vid_fps=60):
    """(start, length) of the `audio_length` s window centred on frame_idx / fps, clamped like the reference
    (dataset.py:439-451): `sample = aud_sample[start : start + length]`.
    A clip SHORTER than the window (`num_samples < length`, dataset.py:441-446): the reference zero-pads the array to
    `length` samples but keeps clamping with the UN-updated `max_len`, so start = num_samples - length is NEGATIVE and the
    slice of the padded array runs from index `num_samples` to index `num_samples` -- an empty sample (which its librosa
    call then rejects).  The same (start, length) come back here; `trim_audio` applies them exactly as the reference does."""
    length = int(audio_length * sampling_rate)
    start_sec = float(frame_idx / vid_fps) - (audio_length / 2)
    start = int(max(0, start_sec * sampling_rate))
    if start + length > num_samples:
        start = num_samples - length
    return start, length


def trim_audio(aud_sample, frame_idx, audio_length, sampling_rate=24000, vid_fps=60):
    """reference `_get_audio_segment` (core/dataset/dataset.py:439-451) on a 1-D waveform -- NumPy array or torch tensor,
    host or device (a view, no copy, unless the clip must be padded): the `audio_length`-second window centred on
    frame_idx / fps, clamped to the clip.  A clip shorter than the window is zero-padded at its end (:441-442) and then
    sliced with the reference's own un-updated `max_len` (:447-450) -- Python's negative-start slice of the padded array,
    which is EMPTY; `Spectrogram` refuses an empty sample like the reference's librosa call does.  Nothing is "fixed"."""
    start, length = trim_audio_window(int(aud_sample.shape[0]), frame_idx, audio_length, sampling_rate, vid_fps)
    if aud_sample.shape[0] < length:
        pad = length - int(aud_sample.shape[0])
        if torch.is_tensor(aud_sample):
            aud_sample = torch.nn.functional.pad(aud_sample, (0, pad))
        else:
            aud_sample = np.pad(aud_sample, (0, pad))
    return aud_sample[start:start + length]


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(m >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (m - min_log_hz / f_sp)), f_sp * m)


def mel_filterbank(sr=24000, n_fft=511, n_mels=128):
    """librosa.filters.mel(sr, n_fft, n_mels) (Slaney scale and normalisation): (n_mels, 256) float32"""
    fmax = sr / 2.0
    freqs = np.linspace(0, fmax, 1 + n_fft // 2, endpoint=True)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - freqs[None, :]
    w = np.maximum(0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    return (w * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]).astype(np.float32)


N_FFT = 511


def stft_geometry(sampling_rate, window_ms=10, step_ms=5):
    """(win, hop) in samples as the reference derives them from the rate (dataset.py:483-484): Python 3's
    `int(round(...))`, ties to even -- 22 050 Hz -> (220, 110), 44 100 Hz -> (441, 220), 24 000 Hz -> (240, 120)."""
    return int(round(window_ms * sampling_rate / 1e3)), int(round(step_ms * sampling_rate / 1e3))


class Spectrogram:
    """`spec = Spectrogram()(wave)`: wave (nseg, L) float32 on the GPU -> (nseg, 256, 1+(L-1)//hop) log-power STFT
    (`spec_type="stft"`, the reference default) or (nseg, 128, T) log-mel dB (`spec_type="logms"`,
    dataset.py:496-506: librosa melspectrogram + power_to_db(ref=max) of each segment; two HIP launches, no torch op).
    `AudioSegments` (audio.py) runs the same code on windows of untrimmed clips through `windows()`.
    Window and hop follow `sampling_rate` (`stft_geometry`; n_fft stays 511, 256 bins): (240, 120) at 24 kHz runs the
    kernel written for it, every other geometry with 8 <= win <= 511 and 1 <= hop <= win the general one
    (`tbn_stft_rate_windows`)."""

    _force_general = False    # tests / scripts/stft_rates_profile.py: send (240, 120) through the general kernel too

    def __init__(self, eps=1e-6, spec_type="stft", sampling_rate=24000, window_ms=10, step_ms=5):
        if spec_type not in ("stft", "logms"):
            raise Exception("Unknown spectrogram representation")
        self.eps = eps
        self.spec_type = spec_type
        self.sampling_rate = sampling_rate
        self.win_length, self.hop_length = stft_geometry(sampling_rate, window_ms, step_ms)
        if self.win_length > N_FFT:     # librosa (reference dataset.py:487-495) refuses win_length > n_fft
            raise ValueError(f"Spectrogram: sampling rate {sampling_rate} Hz gives a window of {self.win_length} samples "
                             f"({window_ms} ms), longer than n_fft = {N_FFT}")
        if self.win_length < 8 or not 1 <= self.hop_length <= self.win_length:
            raise ValueError(f"Spectrogram: sampling rate {sampling_rate} Hz gives window {self.win_length} / hop "
                             f"{self.hop_length} samples; the STFT kernel takes 8 <= window <= {N_FFT}, 1 <= hop <= window")
        self._tw = {}
        self._mel = {}

    def _melbasis(self, device):
        if device not in self._mel:
            self._mel[device] = torch.from_numpy(mel_filterbank(self.sampling_rate)).to(device)
        return self._mel[device]

    def _twiddle(self, device, general=False):
        """one table per (device, win); the general kernel's table of win = 240 has the same bits as the other one"""
        key = (device, self.win_length)
        if key not in self._tw:
            if general:
                host = np.empty(lib().tbn_stft_rate_twiddle_floats(self.win_length), dtype=np.float32)
                call("tbn_stft_rate_make_twiddle", self.win_length, host.ctypes.data)
            else:
                host = np.empty(lib().tbn_stft_twiddle_floats(), dtype=np.float32)
                call("tbn_stft_make_twiddle", host.ctypes.data)
            self._tw[key] = torch.from_numpy(host).to(device)
        return self._tw[key]

    def windows(self, window_ptrs, wave, nseg, L, device):
        """The one code path of both representations: nseg windows of L samples, either `window_ptrs` (a device int64
        tensor of nseg window addresses inside untrimmed clips, `core/dataset/audio.py`) or `wave`, a contiguous
        (nseg, L) batch -- the special case "window s starts at wave + s * L"."""
        if L < 1:       # librosa 0.7.2 (reference dataset.py:487-495) rejects it too: "Input is too short" (util.frame)
            raise ValueError("Spectrogram: empty audio sample (a clip shorter than audio_length, reference dataset.py:441-451)")
        W = 1 + (L - 1) // self.hop_length
        if self._force_general or (self.win_length, self.hop_length) != (240, 120):
            return self._windows_general(window_ptrs, wave, nseg, L, W, device)
        tw = self._twiddle(device)
        if self.spec_type == "stft":
            spec = torch.empty(nseg, 256, W, device=device, dtype=torch.float32)
            if window_ptrs is None:      # same kernel, same bits; this entry's launch stays outside the library profiler,
                                         # whose entries bench.py sums up as the conv stage
                call("tbn_stft_logpower", ptr(wave), nseg, L, ptr(tw), ptr(spec), float(self.eps), stream_ptr())
            else:
                call("tbn_stft_windows", ptr(window_ptrs), 0, nseg, L, ptr(tw), ptr(spec), float(self.eps), STFT_LOGPOWER, 0, 0,
                     stream_ptr())
            return spec
        # log-mel: the STFT kernel writes |X|^2, one more kernel projects it onto the mel basis and converts to dB relative
        # to each segment's own maximum (librosa.power_to_db(S, ref=np.max), top_db = 80)
        power = torch.empty(nseg, 256, W, device=device, dtype=torch.float32)
        spec = torch.empty(nseg, 128, W, device=device, dtype=torch.float32)
        call("tbn_stft_windows", ptr(window_ptrs), ptr(wave), nseg, L, ptr(tw), ptr(spec), 0.0, STFT_LOGMEL,
             ptr(self._melbasis(device)), ptr(power), stream_ptr())
        return spec

    def _windows_general(self, window_ptrs, wave, nseg, L, W, device):
        """`windows` for any (win, hop): one entry for both representations and both ways to name the windows"""
        tw = self._twiddle(device, general=True)
        stft = self.spec_type == "stft"
        spec = torch.empty(nseg, 256 if stft else 128, W, device=device, dtype=torch.float32)
        power = None if stft else torch.empty(nseg, 256, W, device=device, dtype=torch.float32)
        call("tbn_stft_rate_windows", ptr(window_ptrs), ptr(wave), nseg, L, self.win_length, self.hop_length, ptr(tw),
             ptr(spec), float(self.eps) if stft else 0.0, STFT_LOGPOWER if stft else STFT_LOGMEL,
             0 if stft else ptr(self._melbasis(device)), ptr(power), stream_ptr())
        return spec

    def __call__(self, wave):
        if not wave.is_cuda:
            raise TbnHipError("Spectrogram: the STFT kernel needs the waveform on the GPU (no CPU fallback)")
        wave = wave.contiguous().float()
        nseg, L = wave.shape
        return self.windows(None, wave, nseg, L, wave.device)
