"""Inputs of the STFT-at-any-rate tests (tests/test_stft_rates_cpu.py, tests/test_stft_rates_gpu.py) and an fp32 NumPy
restatement of the general kernel's contraction: the library's own twiddle table, tap j of frame t = sample
t * hop - win // 2 + j, accumulated in fp32 in groups of 8 taps.  The restatement is no reference (oracle/stft.py is); it
says how far fp32 arithmetic of this shape lies from the oracle, which is where a tolerance may come from."""
import functools

import numpy as np

RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 51100)


def geometry(rate):
    return int(round(10 * rate / 1e3)), int(round(5 * rate / 1e3))


def lengths(rate):
    """one frame, two frames, the first frame of a second 64-frame block, a ragged tail with L % 4 != 0 somewhere"""
    hop = geometry(rate)[1]
    return (1, hop, 64 * hop + 1, 130 * hop + 3)


@functools.lru_cache(maxsize=None)
def three_signals(rate, L):
    """the three signals of test_kernels_gpu.py::test_stft_logpower_vs_oracle with t = arange(L) / rate; never modified"""
    rng = np.random.RandomState(0)
    t = np.arange(L) / float(rate)
    waves = np.stack([
        0.1 * rng.randn(L),
        0.3 * np.sin(2 * np.pi * (200 + 3000 * t) * t) + 0.01 * rng.randn(L),
        0.5 * np.cos(2 * np.pi * 40 * 24000 / 511.0 * t) + 0.02 * rng.randn(L),
    ]).astype(np.float32)
    waves.setflags(write=False)
    return waves


@functools.lru_cache(maxsize=None)
def mel_signals(rate):
    """3 x int(1.279 * rate) samples: noise, and a 1.5 kHz tone on the second (test_log_mel_spectrogram_vs_oracle's)"""
    import torch
    g = torch.Generator().manual_seed(3)
    L = int(1.279 * rate)
    wave = torch.randn(3, L, generator=g) * 0.1
    wave[1] += torch.sin(2 * np.pi * 1500.0 * (torch.arange(L) / float(rate)))
    out = wave.numpy().copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twiddle(win):
    """[part][tap][bin] float32 from tbn_stft_rate_make_twiddle (host code: needs no GPU)"""
    from attention_based_tbn_amd._lib import call, lib
    kg = (win + 7) // 8
    host = np.empty(lib().tbn_stft_rate_twiddle_floats(win), dtype=np.float32)
    call("tbn_stft_rate_make_twiddle", win, host.ctypes.data)
    return host.reshape(2, kg, 256, 8).transpose(0, 1, 3, 2).reshape(2, kg * 8, 256).copy()


def power_fp32(wave, rate):
    """|X|^2 (256, W) float32 of one waveform the way the kernel forms it"""
    win, hop = geometry(rate)
    tw = twiddle(win)
    taps = tw.shape[1]
    L = len(wave)
    W = 1 + (L - 1) // hop
    idx = hop * np.arange(W)[None, :] - win // 2 + np.arange(taps)[:, None]          # (taps, W) sample numbers
    frames = np.where((idx >= 0) & (idx < L), wave[np.clip(idx, 0, L - 1)], np.float32(0)).astype(np.float32)
    re = np.zeros((256, W), dtype=np.float32)
    im = np.zeros((256, W), dtype=np.float32)
    for g in range(0, taps, 8):
        re += tw[0, g:g + 8].T @ frames[g:g + 8]
        im += tw[1, g:g + 8].T @ frames[g:g + 8]
    return re * re + im * im


def log_power_fp32(wave, rate, eps=1e-6):
    return np.log(power_fp32(wave, rate) + np.float32(eps))


def log_mel_fp32(wave, rate):
    from attention_based_tbn_amd.core.dataset.spectrogram import mel_filterbank
    mel = mel_filterbank(rate) @ power_fp32(wave, rate)
    amin = np.float32(1e-10)
    db = np.float32(10) * np.log10(np.maximum(amin, mel)) - np.float32(10) * np.log10(np.maximum(amin, mel.max()))
    return np.maximum(db, np.float32(-80)).astype(np.float32)
