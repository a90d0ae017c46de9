"""Host-side tests of the audio-file path (no GPU): the float64 restatement of the resampler against an analytic ground
truth, the library's polyphase bank against the restatement's, the RIFF / WAVE walker, and the refusals that must come
before any GPU use."""
import math
import os
import wave

import numpy as np
import pytest

from tests import audio_load_ref as R


@pytest.mark.parametrize("sr_orig,sr_new,tol", [(48000, 24000, 1e-5), (16000, 24000, 1e-5), (22050, 24000, 1e-5),
                                                (44100, 24000, 5e-3)])
def test_restatement_resamples_band_limited_sinusoids(sr_orig, sr_new, tol):
    """A sum of three sinusoids below 0.4 * min(sr_orig, sr_new), 6000 input frames: away from the ends the resampled signal
    must be the same sum sampled at the new rate.  No library is the reference here, the ground truth is analytic.  This
    pins two facts about the restated algorithm: the filter is a UNIT-GAIN LOW-PASS with its cutoff in the right place (a
    wrong rolloff, window or ratio scaling changes the amplitude or lets an image through), and the INDEX ARITHMETIC is
    right (a tap shifted by one sample or a phase taken from the wrong side shifts the output by a fraction of a sample,
    which at these frequencies is an error of 1e-1).  44100 -> 24000 is held to 5e-3 only: resampy's truncated table step
    (278 for 278.6) leaves a gain error of about 1.7e-3, which is reproduced on purpose."""
    frames = 6000
    top = 0.4 * min(sr_orig, sr_new)
    tones = [(0.5, top, 0.3), (0.3, 0.57 * top, 1.1), (0.2, 0.11 * top, 2.0)]

    def signal(rate, count):
        m = np.arange(count, dtype=np.float64)
        return sum(a * np.sin(2 * np.pi * f * m / rate + ph) for a, f, ph in tones)

    y, _ = R.resample(signal(sr_orig, frames), sr_orig, sr_new)
    assert len(y) == R.out_length(frames, sr_orig, sr_new)
    ratio = sr_new / sr_orig
    edge = math.ceil(64 * max(1.0, sr_orig / sr_new) * ratio) + 2
    want = signal(sr_new, len(y))
    err = float(np.abs(y - want)[edge + 1:len(y) - edge - 1].max())
    print(f"{sr_orig} -> {sr_new}: max interior error {err:.3g}")
    assert len(y) > 4 * edge and err < tol, err


def test_restatement_bank_equals_its_tap_loop():
    """the polyphase form (what the kernel reads) against the tap loop, both float64: only the summation order differs"""
    rng = np.random.RandomState(3)
    for sr_orig, sr_new in R.RATIOS[:6]:
        x = rng.rand(700) * 2 - 1
        y, _ = R.resample(x, sr_orig, sr_new)
        W, L = R.geometry(sr_orig, sr_new)
        b = R.bank(sr_orig, sr_new)
        t = np.arange(len(x) * sr_new // sr_orig, dtype=np.int64)
        src = (t * sr_orig // sr_new)[:, None] - W + 1 + np.arange(2 * W)[None, :]
        xs = np.where((src >= 0) & (src < len(x)), x[np.clip(src, 0, len(x) - 1)], 0.0)
        got = (b[:, t % L].T * xs).sum(1)
        assert np.abs(got - y[:len(t)]).max() < 1e-14


@pytest.mark.parametrize("sr_orig,sr_new", R.RATIOS)
def test_library_bank_equals_the_restatement(sr_orig, sr_new):
    """same geometry (W, L); every float32 entry within 1 ulp: both sides are float64 results rounded once, so more than
    that is a bug (different I0 / sin implementations may flip a rounding here and there)"""
    from attention_based_tbn_amd.core.dataset import audio_file as A
    W, L = R.geometry(sr_orig, sr_new)
    assert (W, L) == R.GEOMETRY[(sr_orig, sr_new)]
    taps, phases, floats = A.bank_geometry(sr_orig, sr_new)
    assert (taps, phases, floats) == (2 * W, L, 2 * W * L)
    got = A.make_bank(sr_orig, sr_new)
    want = R.bank(sr_orig, sr_new).astype(np.float32)
    assert got.shape == want.shape == (2 * W, L)
    differ = int((got != want).sum())
    print(f"{sr_orig} -> {sr_new}: (W, L) = ({W}, {L}), {differ} of {got.size} entries differ")
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    assert ((got >= lo) & (got <= hi)).all()
    assert np.abs(got).max() > 0.9 * min(1.0, sr_new / sr_orig)          # the centre tap: rolloff * min(1, ratio)


def test_bank_entries_refuse_what_they_cannot_build():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset import audio_file as A
    assert A.bank_geometry(24000, 24000) == (0, 0, 0)
    with pytest.raises(TbnHipError, match="64 MiB"):
        A.bank_geometry(24000, 1000003)           # a million phases of 130 taps
    with pytest.raises(TbnHipError, match="positive"):
        A.bank_geometry(0, 24000)
    with pytest.raises(ValueError, match="no bank"):
        A.make_bank(24000, 24000)
    assert A.output_tile() >= 64


def test_launch_entry_validates_on_the_host():
    """every refusal of the launch entry comes before the launch: no GPU here, and none is needed"""
    from attention_based_tbn_amd._lib import lib
    L = lib()
    bad = 0x1000        # never dereferenced

    def fails(rc, needle):
        assert rc < 0, rc
        msg = L.tbn_last_error().decode()
        assert needle in msg, msg

    fails(L.tbn_audio_load(bad, 2000, 1000, 1, 7, 48000, 24000, bad, bad, 500, None), "format code 7")
    fails(L.tbn_audio_load(bad, 0, 1000, 0, 1, 48000, 24000, bad, bad, 500, None), "channels")
    fails(L.tbn_audio_load(bad, 18000, 1000, 9, 1, 48000, 24000, bad, bad, 500, None), "channels")
    fails(L.tbn_audio_load(bad, 2000, 1000, 1, 1, 48000, 24000, bad, bad, 501, None), "out_len")
    fails(L.tbn_audio_load(bad, 2002, 1001, 1, 1, 48000, 24000, bad, bad, 500, None), "out_len")     # ceil: 501
    fails(L.tbn_audio_load(bad, 2000, 1000, 1, 1, 48000, 24000, None, bad, 500, None), "needs the bank")
    fails(L.tbn_audio_load(bad, 1999, 1000, 1, 1, 48000, 24000, bad, bad, 500, None), "bytes of PCM")
    fails(L.tbn_audio_load(bad, 2000, 1000, 1, 1, 0, 24000, bad, bad, 500, None), "positive")
    fails(L.tbn_audio_load(bad, 0, 0, 1, 1, 48000, 24000, bad, bad, 0, None), "frames")
    fails(L.tbn_audio_load(bad, 2 ** 62, 2 ** 61, 1, 1, 48000, 24000, bad, bad, 2 ** 60, None), "overflow")
    fails(L.tbn_audio_load(bad + 2, 2000, 1000, 1, 1, 48000, 24000, bad, bad, 500, None), "aligned")
    fails(L.tbn_audio_load(bad, 2000, 1000, 1, 1, 480000, 24000, bad, bad, 50, None), "stages")       # 20 : 1


# ------------------------------------------------------------------------------------------------------------ wav_info
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32"])
def test_wav_info_reads_files_written_by_the_wave_module(tmp_path, fmt, channels):
    from attention_based_tbn_amd.core.dataset import audio_file as A
    from attention_based_tbn_amd.core.dataset import wav_info
    s = R.random_samples(fmt, 37, channels, 1)
    path = str(tmp_path / "a.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(R.WIDTH[fmt])
        f.setframerate(44100)
        f.writeframes(R.to_bytes(fmt, s))
    info = wav_info(path)
    assert info.format == getattr(A, fmt.upper()) and A.FORMAT_NAMES[info.format] == fmt
    assert (info.channels, info.rate, info.frames) == (channels, 44100, 37)
    assert info.data_bytes == 37 * channels * R.WIDTH[fmt]
    with open(path, "rb") as f:
        f.seek(info.data_offset)
        assert f.read(info.data_bytes) == R.to_bytes(fmt, s) and f.read() in (b"", b"\0")


def test_wav_info_reads_float_extensible_padded_and_streamed_files(tmp_path):
    from attention_based_tbn_amd.core.dataset import audio_file as A
    from attention_based_tbn_amd.core.dataset import wav_info
    p = str(tmp_path / "a.wav")
    f32 = R.random_samples("f32", 21, 2, 2)
    off = R.write_wav(p, "f32", f32, 48000)
    assert wav_info(p) == A.WavInfo(A.F32, 2, 48000, 21, off, 21 * 8)
    s24 = R.random_samples("s24", 19, 6, 3)
    off = R.write_wav(p, "s24", s24, 96000, extensible=True)
    assert wav_info(p) == A.WavInfo(A.S24, 6, 96000, 19, off, 19 * 18)
    off = R.write_wav(p, "f32", f32, 22050, extensible=True)
    assert wav_info(p) == A.WavInfo(A.F32, 2, 22050, 21, off, 21 * 8)
    s16 = R.random_samples("s16", 11, 1, 4)
    # a LIST chunk of odd size before the data: its pad byte is skipped (without that the walker reads "\0dat" as a name)
    off = R.write_wav(p, "s16", s16, 24000, chunks_before_data=[(b"LIST", b"INFOabc")])
    assert wav_info(p) == A.WavInfo(A.S16, 1, 24000, 11, off, 22) and off == 12 + 24 + 8 + 8 + 8
    with open(p, "rb") as f:
        f.seek(off)
        assert f.read() == R.to_bytes("s16", s16)
    # a streamed file whose writer never patched the sizes: the data runs to the end of the file; also a declared 0
    for declared in (0xFFFFFFFF, 0):
        off = R.write_wav(p, "s16", s16, 24000, data_size=declared)
        assert wav_info(p) == A.WavInfo(A.S16, 1, 24000, 11, off, 22)
    # a data chunk that claims more than the file holds is clamped; a trailing partial frame is dropped
    off = R.write_wav(p, "s16", R.random_samples("s16", 10, 2, 5), 24000, cut=44 + 4 * 7 + 3)
    assert wav_info(p) == A.WavInfo(A.S16, 2, 24000, 7, 44, 28)


def test_wav_info_refusals_name_the_path(tmp_path):
    import struct
    from attention_based_tbn_amd.core.dataset import wav_info
    p = str(tmp_path / "odd name.wav")
    s16 = R.random_samples("s16", 8, 2, 6)

    def patched(edit, **kw):
        R.write_wav(p, kw.pop("fmt", "s16"), kw.pop("samples", s16), 24000, **kw)
        with open(p, "rb") as f:
            blob = bytearray(f.read())
        edit(blob)
        with open(p, "wb") as f:
            f.write(bytes(blob))

    def refused(needle):
        with pytest.raises(ValueError) as e:
            wav_info(p)
        assert p in str(e.value) and needle in str(e.value), str(e.value)

    def fmt_field(offset, code, value):          # the fmt body starts at byte 20
        return lambda blob: blob.__setitem__(slice(20 + offset, 20 + offset + struct.calcsize(code)), struct.pack(code, value))

    patched(fmt_field(14, "<H", 64), fmt="f32", samples=R.random_samples("f32", 8, 1, 1))
    refused("64-bit float")
    patched(fmt_field(0, "<H", 0x55))            # MPEG layer 3
    refused("format tag 0x55")
    patched(fmt_field(0, "<H", 6))               # A-law
    refused("format tag 0x6")
    patched(fmt_field(14, "<H", 12))             # 12-bit PCM
    refused("12-bit")
    patched(fmt_field(2, "<H", 0))
    refused("0 channels")
    patched(fmt_field(2, "<H", 9))
    refused("9 channels")
    patched(fmt_field(12, "<H", 6))
    refused("block_align 6")
    patched(lambda blob: blob.__setitem__(slice(0, 4), b"RIFX"))
    refused("not a RIFF")
    patched(lambda blob: blob.__setitem__(slice(8, 12), b"AVI "))
    refused("not a RIFF")
    for cut, needle in ((7, "not a RIFF"), (12, "truncated"), (30, "truncated"), (40, "truncated")):
        R.write_wav(p, "s16", s16, 24000, cut=cut)      # inside the RIFF header, before / inside fmt, before the data header
        refused(needle)
    R.write_wav(p, "s24", R.random_samples("s24", 4, 2, 1), 24000, extensible=True, cut=12 + 8 + 20)
    refused("truncated")
    with pytest.raises(OSError):
        wav_info(str(tmp_path / "missing.wav"))


# ---------------------------------------------------------------------------------------------------------- API refusals
def test_api_refusals_need_no_gpu(tmp_path):
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import Video_Dataset, load_audio
    from attention_based_tbn_amd.core.dataset.audio_file import resample_pcm
    import torch
    p = str(tmp_path / "a.wav")
    R.write_wav(p, "s16", R.random_samples("s16", 100, 2, 1), 48000)
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        load_audio(p, 24000, device="cpu")
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        resample_pcm(torch.zeros(400, dtype=torch.uint8), 100, 2, 1, 48000, 24000)
    cfg = load_config([])
    with pytest.raises(ValueError, match="audio_load='bogus'"):
        Video_Dataset(cfg, None, "ann.csv", ["Audio"], mode="train", audio_load="bogus")
    from tests import clip_loader_util as U
    cfg = load_config(U.write_dataset(tmp_path / "ds") + ["data.audio.read_audio_pickle=False", "data.audio.file_ext=mp3"])
    with pytest.raises(ValueError, match="'mp3'"):
        U.make_dataset(cfg, ["Audio"], "val", audio_load="device")
    assert U.make_dataset(cfg, ["Audio"], "val").audio_load == "host"        # the default path does not look at it
    cfg.data.audio.file_ext = "wav"
    assert U.make_dataset(cfg, ["Audio"], "val", audio_load="device").audio_load == "device"
    assert not os.path.exists(os.path.join(str(tmp_path), "ds", "audio", U.VIDS[0] + ".wav"))   # nothing was read


def test_error_bound_of_the_gpu_tests_has_teeth():
    """the bound tests/test_audio_load_gpu.py holds the kernel to, on a float32 emulation of the kernel's sum over the
    LIBRARY's bank (sequential, tap order): the right sum stays far inside it, a bank shifted by one tap or read at the
    neighbouring phase misses it by orders of magnitude -- so passing it says the indices are right"""
    from attention_based_tbn_amd.core.dataset import audio_file as A
    for sr_orig, sr_new in ((48000, 24000), (44100, 24000), (16000, 24000)):
        W, L = R.geometry(sr_orig, sr_new)
        x = R.mono32("s16", R.random_samples("s16", 900, 1, 7))
        want, mass = R.resample(x, sr_orig, sr_new)
        bound = R.error_bound(mass, W)
        n_out = len(x) * sr_new // sr_orig
        t = np.arange(n_out, dtype=np.int64)
        src = (t * sr_orig // sr_new)[:, None] - W + 1 + np.arange(2 * W)[None, :]
        xs = np.where((src >= 0) & (src < len(x)), x[np.clip(src, 0, len(x) - 1)], np.float32(0))
        bank = A.make_bank(sr_orig, sr_new)

        def emulate(b, phase_shift=0):
            w = b[:, (t + phase_shift) % L].T
            acc = np.zeros(n_out, dtype=np.float32)
            for k in range(2 * W):
                acc = (acc + (w[:, k] * xs[:, k]).astype(np.float32)).astype(np.float32)
            return np.abs(acc.astype(np.float64) - want[:n_out]) / bound[:n_out]

        assert emulate(bank).max() < 0.25
        assert emulate(np.roll(bank, 1, axis=0)).max() > 1e3           # every tap one sample late
        if L > 1:
            assert emulate(bank, 1).max() > 1e3                        # the neighbouring phase's weights
