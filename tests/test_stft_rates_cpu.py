"""CPU: the STFT geometry at any audio sampling rate (reference core/dataset/dataset.py:483-495: window and hop from the
rate, n_fft = 511) -- `stft_geometry`, `Spectrogram`'s construction errors, and the host twiddle table of the general
kernel (`tbn_stft_rate_make_twiddle`) against the NumPy fp64 formula."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rate,want", [(16000, (160, 80)), (22050, (220, 110)), (44100, (441, 220)), (48000, (480, 240)),
                                       (51100, (511, 256)), (2500, (25, 12)), (24000, (240, 120)), (8000, (80, 40)),
                                       (11025, (110, 55)), (32000, (320, 160))])
def test_geometry_table(rate, want):
    """Python 3's round: ties to even (220.5 -> 220, 255.5 -> 256, 12.5 -> 12)"""
    from attention_based_tbn_amd.core.dataset import stft_geometry
    from attention_based_tbn_amd.core.dataset.spectrogram import stft_geometry as same
    assert stft_geometry is same
    assert stft_geometry(rate) == want
    assert stft_geometry(rate, 10, 5) == want
    assert all(type(v) is int for v in stft_geometry(rate))


def test_geometry_follows_window_and_step():
    from attention_based_tbn_amd.core.dataset import stft_geometry
    assert stft_geometry(16000, window_ms=20, step_ms=10) == (320, 160)
    assert stft_geometry(24000, window_ms=5, step_ms=2.5) == (120, 60)


def test_construction_errors_and_kept_geometry():
    from attention_based_tbn_amd.core.dataset import Spectrogram
    with pytest.raises(ValueError) as e:
        Spectrogram(sampling_rate=51200)            # window 512 > n_fft: librosa refuses win_length > n_fft
    assert "51200" in str(e.value) and "512" in str(e.value)
    with pytest.raises(ValueError):
        Spectrogram(sampling_rate=96000)
    with pytest.raises(ValueError):
        Spectrogram(sampling_rate=700)              # window 7: below one tap group
    s = Spectrogram(sampling_rate=24000)
    assert (s.win_length, s.hop_length) == (240, 120) and Spectrogram._force_general is False
    s = Spectrogram()
    assert (s.win_length, s.hop_length) == (240, 120)
    for rate in (800, 16000, 44100, 51100):         # the ends of the accepted domain at 10 / 5 ms
        s = Spectrogram(sampling_rate=rate, spec_type="logms")
        assert (s.win_length, s.hop_length) == (int(round(rate / 100)), int(round(rate / 200)))
    s = Spectrogram(sampling_rate=16000, window_ms=20, step_ms=10)
    assert (s.win_length, s.hop_length) == (320, 160)


def _table(win):
    from attention_based_tbn_amd._lib import call, lib
    n = lib().tbn_stft_rate_twiddle_floats(win)
    assert n == 2 * ((win + 7) // 8) * 256 * 8
    host = np.full(n + 16, 7.0, dtype=np.float32)   # guard words behind the table
    call("tbn_stft_rate_make_twiddle", win, host.ctypes.data)
    assert (host[n:] == 7.0).all()
    return host[:n].copy()


def test_twiddle_240_is_the_24khz_table():
    from attention_based_tbn_amd._lib import call, lib
    n = lib().tbn_stft_twiddle_floats()
    assert lib().tbn_stft_rate_twiddle_floats(240) == n
    old = np.empty(n, dtype=np.float32)
    call("tbn_stft_make_twiddle", old.ctypes.data)
    assert np.array_equal(_table(240).view(np.uint32), old.view(np.uint32))


@pytest.mark.parametrize("win", [80, 441, 511, 8, 25])
def test_twiddle_against_numpy(win):
    """fp64 formula rounded to fp32; the two libms may round one fp32 ulp apart on values below 1 -> 2**-23"""
    kg = (win + 7) // 8
    got = _table(win).reshape(2, kg, 256, 8).transpose(0, 1, 3, 2).reshape(2, kg * 8, 256)   # [part][tap][bin]
    lpad = (511 - win) // 2
    j = np.arange(win)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / win)
    m = ((j[:, None] + lpad) * np.arange(256)[None, :]) % 511          # exact phase reduction
    ang = 2.0 * np.pi * m / 511.0
    want = np.stack([hann[:, None] * np.cos(ang), -hann[:, None] * np.sin(ang)]).astype(np.float32)
    assert np.abs(got[:, :win].astype(np.float64) - want).max() <= 2.0 ** -23
    pad = got[:, win:]
    assert pad.size == 2 * (8 * kg - win) * 256 and (pad.view(np.uint32) == 0).all()      # exact +0.0
    assert (got[:, 0] == 0).all()                                      # periodic Hann: tap 0 is zero


def test_twiddle_refusals():
    from attention_based_tbn_amd._lib import lib
    handle = lib()
    buf = np.zeros(16, dtype=np.float32)
    for win in (0, 7, 512, -3):
        assert handle.tbn_stft_rate_twiddle_floats(win) == 0
        assert handle.tbn_stft_rate_make_twiddle(win, buf.ctypes.data) != 0
    assert handle.tbn_stft_rate_make_twiddle(240, None) != 0
    assert (buf == 0).all()


def test_header_declares_the_new_entries():
    from attention_based_tbn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tbn_hip.h")).read()
    handle = _lib.lib()
    for name, nargs in (("tbn_stft_rate_twiddle_floats", 1), ("tbn_stft_rate_make_twiddle", 2), ("tbn_stft_rate_windows", 13)):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs and getattr(handle, name) is not None
    assert "dataset.py:461-510" in header[header.index("The STFT at any sampling rate"):header.index("tbn_stft_rate_twiddle_floats(int win);")]


@pytest.mark.parametrize("rate", [11025, 22050, 44100, 51100])
def test_table_and_tap_rule_reproduce_the_oracle(rate):
    """the library's table, tap j of frame t = sample t * hop - win // 2 + j and zero padding, contracted in fp32 NumPy
    (tests/stft_rates_util.py), land on oracle/stft.py at the rates with an odd win // 2, a rounded hop or a rounded window --
    the geometry the kernel implements, pinned without a GPU"""
    from oracle.stft import log_power_spectrogram
    from tests.stft_rates_util import geometry, lengths, log_power_fp32, three_signals
    hop = geometry(rate)[1]
    for L in lengths(rate)[:3]:
        waves = three_signals(rate, L)
        for i in range(3):
            ref = log_power_spectrogram(waves[i], sampling_rate=rate)
            got = log_power_fp32(waves[i], rate)
            assert got.shape == ref.shape == (256, 1 + (L - 1) // hop)
            assert np.abs(got - ref).max() < 2e-3
