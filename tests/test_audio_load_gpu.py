"""`load_audio` (decode, downmix and resampling in one HIP launch) against the float64 restatement of tests/audio_load_ref.py,
the dataset's opt-in `audio_load="device"` path and the `create_audio_pickle` tool.

Every output buffer lies inside a larger one filled with NaN: the sentinels in front of and behind it must survive.

Resampled outputs are held to a DERIVED bound, not a chosen tolerance.  The kernel sums 2W products of float32 inputs and
float32-rounded weights in float32: per sample |y - y_ref| <= (2W + 3) * 2^-24 * sum_k |w_k| |x_k| + 2^-126, for any
summation order and with or without fused multiply-adds; the sum is taken from the restatement's own weights and inputs
(`audio_load_ref.error_bound`).  A tap shifted by one sample or a phase taken from the wrong row misses it by orders of
magnitude."""
import os
import wave

import numpy as np
import pytest
import torch

from tests import audio_load_ref as R
from tests import clip_loader_util as U

pytestmark = pytest.mark.gpu

PAD = 96      # NaN sentinels on each side


def _load(path, sr, out_len):
    """`load_audio` into the middle of a NaN buffer -> the samples (host float32); the sentinels survive"""
    from attention_based_tbn_amd.core.dataset import load_audio
    big = torch.full((out_len + 2 * PAD,), float("nan"), device="cuda")
    got = load_audio(path, sr, out=big[PAD:PAD + out_len])
    torch.cuda.synchronize()
    assert got.data_ptr() == big.data_ptr() + 4 * PAD and got.shape == (out_len,)
    host = big.cpu().numpy()
    assert np.isnan(host[:PAD]).all() and np.isnan(host[PAD + out_len:]).all(), "a sentinel was overwritten"
    assert not np.isnan(host[PAD:PAD + out_len]).any(), "an output sample was not written"
    return host[PAD:PAD + out_len].copy()


def _check_resampled(path, x, sr_orig, sr_new, what):
    """x: the mono float32 samples the kernel filters (exactly) -> asserts length, bound and the zero tail"""
    frames = len(x)
    want, mass = R.resample(x, sr_orig, sr_new)
    assert len(want) == R.out_length(frames, sr_orig, sr_new)
    got = _load(path, sr_new, len(want))
    W = R.geometry(sr_orig, sr_new)[0]
    bound = R.error_bound(mass, W)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    print(f"{what}: {frames} frames -> {len(want)}, max |err| {err.max():.3g}, worst err / bound {worst:.3g}")
    assert (err <= bound).all(), (what, frames, int(np.argmax(err / bound)), worst)
    n_out = frames * sr_new // sr_orig
    assert len(want) - n_out in (0, 1)
    if len(want) > n_out:
        assert got[-1] == 0.0 and not np.signbit(got[-1])          # librosa's fix_length pads with exactly 0
    return got


def _frames_for_outputs(count, sr_orig, sr_new):
    """the smallest frame count whose output has at least `count` samples (every count is not reachable when up-sampling)"""
    n = max(1, (count - 1) * sr_orig // sr_new - 2)
    while R.out_length(n, sr_orig, sr_new) < count:
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------- a. equal rate
@pytest.mark.parametrize("frames", [5000, 1])
@pytest.mark.parametrize("channels", [1, 2])
def test_equal_rate_s16_equals_read_wav(tmp_path, channels, frames):
    from attention_based_tbn_amd.core.dataset import read_wav
    p = str(tmp_path / "a.wav")
    s = R.random_samples("s16", frames, channels, 10 + channels)
    with wave.open(p, "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(24000)
        f.writeframes(R.to_bytes("s16", s))
    got = _load(p, 24000, frames)
    want = read_wav(p, 24000)
    assert want.dtype == np.float32 and torch.equal(torch.from_numpy(got), torch.from_numpy(want))


# ----------------------------------------------------------------------------------------------- b. decode at equal rate
@pytest.mark.parametrize("channels", [1, 2, 3, 6])
@pytest.mark.parametrize("fmt", ["u8", "s24", "s32", "f32"])
def test_decode_and_downmix_every_format(tmp_path, fmt, channels):
    """exact where float32 holds every intermediate (integers of at most 16 bits, at most 2 channels); otherwise within
    (channels + 1) * 2^-24 * mean|x| of the float64 mean: one rounding per addition, one for the division, one for the
    int32 -> float32 conversion"""
    frames = 1000
    p = str(tmp_path / "a.wav")
    s = R.random_samples(fmt, frames, channels, 20 + channels)
    R.write_wav(p, fmt, s, 16000, extensible=(channels > 2))
    got = _load(p, 16000, frames).astype(np.float64)
    exact = R.decode(fmt, s).astype(np.float64) if fmt == "f32" else (
        (np.asarray(s, dtype=np.float64) - 128) / 128 if fmt == "u8" else np.asarray(s, dtype=np.float64) / 2.0 ** (8 * R.WIDTH[fmt] - 1))
    want = exact.mean(axis=1)
    err = np.abs(got - want)
    if fmt == "u8" and channels <= 2:
        assert (err == 0).all()
    else:
        assert (err <= (channels + 1) * 2.0 ** -24 * np.abs(exact).mean(axis=1)).all(), float(err.max())
    assert np.array_equal(got.astype(np.float32), R.mono32(fmt, s))        # and bit for bit the float32 restatement


# ----------------------------------------------------------------------------------------------------------- c. resample
@pytest.mark.parametrize("sr_orig,sr_new", R.RATIOS)
def test_resample_noise_at_the_sizes_that_can_go_wrong(tmp_path, sr_orig, sr_new):
    """uniform noise, s16 mono.  1, 2 and 5 frames: both wings clipped by the clip's ends; W and 2W + 1: a wing just (not)
    reaching an end; output counts T - 1, T, T + 1, 2T + 1 around the kernel's tile T: the last tile full, one short, one
    sample into the next, and a second seam; 23999 -> 24000 with 600 frames is the large bank (24000 phases)"""
    from attention_based_tbn_amd.core.dataset.audio_file import output_tile
    W, L = R.geometry(sr_orig, sr_new)
    T = output_tile()
    sizes = [1, 2, 5, W, 2 * W + 1] + [_frames_for_outputs(c, sr_orig, sr_new) for c in (T - 1, T, T + 1, 2 * T + 1)]
    if (sr_orig, sr_new) == (23999, 24000):
        sizes.append(600)
    p = str(tmp_path / "a.wav")
    tails = 0
    for frames in sizes:
        s = R.random_samples("s16", frames, 1, frames)
        R.write_wav(p, "s16", s, sr_orig)
        got = _check_resampled(p, R.mono32("s16", s), sr_orig, sr_new, f"{sr_orig} -> {sr_new}")
        tails += len(got) > frames * sr_new // sr_orig
        if frames >= 2 * W:
            assert np.abs(got).max() > 0.05         # noise in, noise out: not an all-zero output inside a generous bound
    assert tails == sum((f * sr_new) % sr_orig != 0 for f in sizes)
    if sr_new % sr_orig:
        assert tails > 0                             # the padded tail sample was met (integer up-sampling has none)


# ----------------------------------------------------------------------------------------------------- d. 64-bit positions
def test_positions_past_32_bits(tmp_path):
    """48000 -> 24000, 200 001 frames: t * sr_orig passes 2^32 at t = 89 479; every output against the chunked restatement"""
    frames = 200001
    p = str(tmp_path / "a.wav")
    s = R.random_samples("s16", frames, 1, 4)
    R.write_wav(p, "s16", s, 48000)
    got = _check_resampled(p, R.mono32("s16", s), 48000, 24000, "48000 -> 24000 long")
    assert len(got) == 100001 and 89479 * 48000 > 2 ** 32 and got[-1] == 0.0


# ----------------------------------------------------------------------------------------------------- e. everything at once
def test_s24_stereo_44100(tmp_path):
    """byte-granular frames (6 bytes), 80 phases and the downmix in one launch"""
    p = str(tmp_path / "a.wav")
    s = R.random_samples("s24", 3001, 2, 5)
    R.write_wav(p, "s24", s, 44100)
    _check_resampled(p, R.mono32("s24", s), 44100, 24000, "s24 stereo 44100 -> 24000")


def test_launches_are_counted_under_their_kernel_names(tmp_path):
    import ctypes as C
    from attention_based_tbn_amd._lib import lib
    from attention_based_tbn_amd.core.dataset import load_audio
    L = lib()
    p = str(tmp_path / "a.wav")
    R.write_wav(p, "s16", R.random_samples("s16", 3000, 2, 6), 48000)
    load_audio(p, 24000)                  # first use: the bank goes up
    torch.cuda.synchronize()
    L.tbn_profile_reset()
    L.tbn_profile_enable(1)
    try:
        load_audio(p, 24000)
        load_audio(p, 48000)
        load_audio(p, 44100)
        torch.cuda.synchronize()
    finally:
        L.tbn_profile_enable(0)
    seen = {}
    name = C.create_string_buffer(160)
    for i in range(L.tbn_profile_num_entries()):
        cnt, ms, fl = C.c_long(), C.c_double(), C.c_double()
        L.tbn_profile_entry(i, name, 160, C.byref(cnt), C.byref(ms), C.byref(fl))
        seen[name.value.decode()] = cnt.value
    L.tbn_profile_reset()
    assert seen == {"audio_load_kernel<uniform>": 1, "audio_decode_kernel": 1, "audio_load_kernel<phases>": 1}, seen


# ------------------------------------------------------------------------------------------------------------ f. dataset
MODALITY = ["RGB", "Flow", "Audio"]


def _write_camera_audio(root):
    """the fixture's audio as extracted from the camera files: 48 kHz stereo s16, twice AUDIO_SAMPLES frames"""
    for k, vid in enumerate(U.VIDS):
        s = R.random_samples("s16", 2 * U.AUDIO_SAMPLES, 2, 30 + k) // 4
        R.write_wav(os.path.join(str(root), "audio", vid + ".wav"), "s16", s, 48000)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b)
    elif isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert a == b


def test_dataset_reads_camera_audio_on_the_device(tmp_path):
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import AudioSegments, load_audio
    from attention_based_tbn_amd.core.utils import ClipLoader
    cfg = load_config(U.write_dataset(tmp_path) + ["data.audio.read_audio_pickle=False", "model.attention.enable=False"])
    _write_camera_audio(tmp_path)
    # the default dataset still refuses the file, with the message it always had
    with pytest.raises(Exception, match="resampling is out of scope: resample the file beforehand"):
        U.make_dataset(cfg, ["Audio"], "val").batch([0, 1])
    ds = U.make_dataset(cfg, ["Audio"], "val", audio_load="device")
    data = ds.batch([0, 1, 2])[0]
    waves = {vid: load_audio(os.path.join(str(tmp_path), "audio", vid + ".wav"), 24000) for vid in U.VIDS}
    assert all(w.shape == (U.AUDIO_SAMPLES,) and w.is_cuda for w in waves.values())
    want = AudioSegments.from_config(cfg)([waves[row[1]] for row in U.ROWS], data["indices"]["Audio"])["Audio"]
    assert data["Audio"].shape[:2] == (3, 2) and torch.equal(data["Audio"], want)
    assert sorted(ds._waves) == sorted(U.VIDS) and all(torch.equal(ds._waves[v], waves[v]) for v in U.VIDS)
    # inside the prefetch producer (its own thread, a side stream) as on the calling thread
    full = U.make_dataset(cfg, MODALITY, "train", audio_load="device")
    torch.manual_seed(3)
    twin = list(ClipLoader(full, 2, shuffle=True, prefetch=0, rng="private"))
    full = U.make_dataset(cfg, MODALITY, "train", audio_load="device")          # a cold waveform cache for the producer
    torch.manual_seed(3)
    got = list(ClipLoader(full, 2, shuffle=True, prefetch=2))
    assert len(got) == len(twin) == 2
    for a, b in zip(got, twin):
        _same(a, b)


def test_create_dataloader_passes_audio_load_through(tmp_path):
    import logging
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.utils import create_dataloader
    cfg = load_config(U.write_dataset(tmp_path) + ["data.audio.read_audio_pickle=False", "model.attention.enable=False"])
    _write_camera_audio(tmp_path)
    log = logging.getLogger("test_audio_load")
    loader = create_dataloader(cfg, log, ["Audio"], "val", audio_load="device")
    assert loader.dataset.audio_load == "device"
    assert next(iter(loader))[0]["Audio"].shape[:2] == (2, 2)
    assert create_dataloader(cfg, log, ["Audio"], "val").dataset.audio_load == "host"


# --------------------------------------------------------------------------------------------------------------- g. tool
def test_create_audio_pickle_tool(tmp_path, capsys):
    from attention_based_tbn_amd.core.dataset import load_audio
    from attention_based_tbn_amd.preprocessing import create_audio_pickle as tool
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    R.write_wav(str(src / "P01_01.wav"), "s16", R.random_samples("s16", 5000, 2, 1), 48000)
    R.write_wav(str(src / "P01_02.wav"), "f32", R.random_samples("f32", 3000, 1, 2), 44100)
    R.write_wav(str(src / "P01_03.wav"), "s16", R.random_samples("s16", 5000, 2, 3), 48000, cut=30)     # ends inside fmt
    (src / "notes.txt").write_text("not audio")
    written, rejected = tool.main(tool.parse_args([str(src), "--out-dir", str(dst)]))
    assert rejected == ["P01_03.wav"] and sorted(os.listdir(str(dst))) == ["P01_01.npy", "P01_02.npy"]
    assert sorted(written) == [str(dst / "P01_01.npy"), str(dst / "P01_02.npy")]
    for name, n in (("P01_01", 2500), ("P01_02", R.out_length(3000, 44100, 24000))):
        saved = np.load(str(dst / (name + ".npy")))
        assert saved.dtype == np.float32 and saved.shape == (n,)
        assert torch.equal(torch.from_numpy(saved), load_audio(str(src / (name + ".wav")), 24000).cpu())
    out = capsys.readouterr().out
    assert "Failed to read audio file P01_03.wav" in out and "List of rejected files: ['P01_03.wav']" in out
    other = tool.parse_args([str(src), "--sr", "16000", "--out-dir", str(dst), "--ext", "wav"])
    assert (other.sr, other.ext) == (16000, "wav") and tool.parse_args([str(src)]).sr == 24000
