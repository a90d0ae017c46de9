"""Host side of the device audio data layer (attention_based_tbn_amd/core/dataset/audio.py; reference
core/dataset/dataset.py:421-459 `_get_audio_segment`): the vectorised window table against the scalar function and the
oracle, and the refusals that keep the STFT kernel inside its clips -- all before any launch, no GPU needed."""
import re
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_LENGTHS = [30000, 30695, 30696, 31003, 40001, 50400, 50401, 70002, 123457, 200001]
AUDIO_LENGTHS = [1.279, 2.1]


def _frames(num_samples, sampling_rate=24000, vid_fps=60):
    """clip start, around the middle and the end of a clip of num_samples samples (the last frames lie past the audio)"""
    last = int(num_samples / sampling_rate * vid_fps)
    return [max(0, f) for f in (0, 1, 2, 37, 38, 39, 75, 76, 77, last // 2 - 1, last // 2, last // 2 + 1, last // 2 + 2,
                                last // 2 + 3, last - 80, last - 77, last - 40, last - 2, last - 1, last, last + 1, last + 30)]


@pytest.mark.parametrize("audio_length", AUDIO_LENGTHS)
def test_audio_windows_equal_scalar_function_and_oracle(audio_length):
    from attention_based_tbn_amd.core.dataset import audio_windows, trim_audio_window
    from oracle.stft import trim_audio
    frames = np.array([_frames(n) for n in CLIP_LENGTHS])
    assert (frames >= 0).all()
    starts, length = audio_windows(CLIP_LENGTHS, frames, audio_length)
    assert starts.shape == frames.shape and starts.dtype == np.int64 and length == int(audio_length * 24000)
    seen_short = False
    for b, n in enumerate(CLIP_LENGTHS):
        marker = np.arange(n, dtype=np.float64)          # sample value = its index: the slice names its own start
        for j, f in enumerate(frames[b]):
            assert (int(starts[b, j]), length) == trim_audio_window(n, int(f), audio_length), (n, f)
            if n >= length:
                piece, _ = trim_audio(marker, int(f), audio_length)
                assert len(piece) == length and int(piece[0]) == starts[b, j], (n, f)
                assert 0 <= starts[b, j] <= n - length
            else:
                seen_short = True
                assert starts[b, j] == n - length < 0      # the reference's un-updated max_len (dataset.py:447-450)
    assert seen_short == (30000 < length)
    # other rates, and integer inputs of any container type
    s2, l2 = audio_windows(torch.tensor([48000, 99999]), [[0, 50, 200], [7, 90, 140]], 1.279, sampling_rate=16000, vid_fps=25)
    for b, n in enumerate((48000, 99999)):
        for j, f in enumerate(([0, 50, 200], [7, 90, 140])[b]):
            assert (int(s2[b, j]), l2) == trim_audio_window(n, f, 1.279, 16000, 25)


class _FakeClip:
    """stands in for a device tensor so that the table and its refusals can be reached without a GPU (window_table only
    asks a clip for these attributes); nothing here is ever handed to the library"""

    def __init__(self, n, dtype=torch.float32, contiguous=True, cuda=True):
        self.shape = (n,)
        self.dtype = dtype
        self.is_cuda = cuda
        self._c = contiguous

    def dim(self):
        return 1

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return 4096


def test_window_table_refusals(monkeypatch):
    from attention_based_tbn_amd import _lib
    from attention_based_tbn_amd.core.dataset import audio as audio_mod, spectrogram as spec_mod
    from attention_based_tbn_amd.core.dataset import AudioSegments, window_table

    def no_call(*a, **k):
        raise AssertionError("library call before the table was checked")
    monkeypatch.setattr(audio_mod, "call", no_call)
    monkeypatch.setattr(spec_mod, "call", no_call)
    L = 30696
    good = window_table([_FakeClip(40001), _FakeClip(L)], [[0, 9305], [0, 0]], L)
    assert good.tolist() == [4096, 4096 + 4 * 9305, 4096, 4096] and good.dtype == np.int64
    with pytest.raises(_lib.TbnHipError, match="leaves the clip"):
        window_table([_FakeClip(40001)], [[0, 9306]], L)              # one sample past the end
    with pytest.raises(_lib.TbnHipError, match="leaves the clip"):
        window_table([_FakeClip(40001)], [[-1, 0]], L)
    with pytest.raises(_lib.TbnHipError, match="float32"):
        window_table([_FakeClip(40001, dtype=torch.float64)], [[0]], L)
    with pytest.raises(_lib.TbnHipError, match="contiguous"):
        window_table([_FakeClip(40001, contiguous=False)], [[0]], L)
    with pytest.raises(ValueError, match="empty audio sample"):           # the reference's short-clip case
        window_table([_FakeClip(L - 1)], [[-1]], L)
    # real CPU tensors: refused, whole layer, before any library call
    layer = AudioSegments(1.279)
    with pytest.raises(_lib.TbnHipError, match="not on the GPU"):
        layer([torch.zeros(40001)], [[0, 100]])
    with pytest.raises(_lib.TbnHipError, match="not on the GPU"):
        layer([np.zeros(40001, dtype=np.float32)], [[0, 100]])
    with pytest.raises(ValueError):
        AudioSegments(1.279, prior_type="quiet")


def test_short_clip_raises_value_error_like_spectrogram():
    from attention_based_tbn_amd.core.dataset import window_table, audio_windows
    starts, length = audio_windows([20000], [[100, 300]], 1.279)
    assert (starts == 20000 - length).all()
    with pytest.raises(ValueError):
        window_table([_FakeClip(20000)], starts, length)


def test_header_lib_and_signatures_agree_on_the_audio_entries():
    from attention_based_tbn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tbn_hip.h")).read()
    for name in ("tbn_stft_windows", "tbn_attn_prior_loud"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name) is not None
    for name, val in (("TBN_STFT_LOGPOWER", 0), ("TBN_STFT_LOGMEL", 1), ("TBN_CAP_AUDIO_LAYER", 32)):
        assert re.search(r"^#define %s %d$" % (name, val), header, re.M), name
    from attention_based_tbn_amd.core.dataset import audio
    assert (audio.STFT_LOGPOWER, audio.STFT_LOGMEL) == (0, 1)
    assert _lib.lib().tbn_capabilities() & 32
    # the entry whose bits must not move keeps its signature
    assert re.search(r"int tbn_stft_logpower\(const float\* wave, int nseg, int len, const float\* twiddle, float\* spec, "
                     r"float eps,\s+void\* stream\);", header)


def test_from_config_reads_the_audio_and_attention_keys():
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import AudioSegments
    layer = AudioSegments.from_config(load_config(["data.audio.audio_length=1.279", "model.attention.prior_type=loud"]))
    assert (layer.audio_length, layer.sampling_rate, layer.vid_fps, layer.prior_type) == (1.279, 24000, 60, "loud")
    assert layer.spectrogram.spec_type == "stft" and layer.num_weights == 8
    layer = AudioSegments.from_config(load_config(["model.attention.enable=False", "data.audio.spec_type=logms"]))
    assert layer.prior_type is None and layer.spectrogram.spec_type == "logms" and layer.num_weights == 13
