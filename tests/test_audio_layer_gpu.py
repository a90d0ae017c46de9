"""The audio data layer on the device (attention_based_tbn_amd/core/dataset/audio.py; reference
core/dataset/dataset.py:421-575): windows cut inside the STFT launch (tbn_stft_windows), log-mel as HIP kernels and the
loud prior (tbn_attn_prior_loud) -- against the shipped per-segment path, the NumPy oracle and the host prior.

Untrimmed clips whose lengths are no multiples of 4 (all but the first start 4, 8 or 12 bytes off a 16-byte boundary), four
segments each: a window clamped to the clip start, two further in, one clamped to the clip end -- between them `start % 4`
and the absolute window addresses modulo 16 bytes take every value.  audio_length 1.279 s (L = 30 695, W = 256: four full
blocks of 64 frames), 2.1 s (W = 420: a partial last block; clips longer than its 50 400-sample window) and 0.32005 s
(L = 7681, W = 65: the second frame block holds a single frame).  At 60 fps and 24 kHz an unclamped start is
400 f - 12000 * audio_length: for 1.279 s that is a multiple of 4, and an end clamp `len - 30695` reaches start % 4 == 1
only from a length that IS a multiple of 4 -- hence the fourth clip of that case."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CLIP_LENGTHS = {1.279: (40001, 31003, 70002, 50000), 2.1: (70002, 60001, 91003), 0.32005: (40001, 31003, 70002)}
AUDIO_LENGTHS = sorted(CLIP_LENGTHS)
WIDTH = {1.279: 256, 2.1: 420, 0.32005: 65}
OFFSETS = (0, 2, 1, 3)    # floats between a clip's first sample and its allocation (which is at least 16-byte aligned)


@functools.lru_cache(maxsize=None)
def _case(audio_length):
    """host clips (float32 NumPy, never modified), their device copies and the frame table"""
    rng = np.random.RandomState(int(audio_length * 1000))
    host, frames = [], []
    for i, n in enumerate(CLIP_LENGTHS[audio_length]):
        t = np.arange(n) / 24000.0
        x = 0.1 * rng.randn(n) + (0.0, 0.6, 0.3, 0.05)[i] * np.sin(2 * np.pi * (300.0 + 900.0 * i + 2000.0 * i * t) * t)
        host.append(x.astype(np.float32))
        last = int(n / 24000.0 * 60)
        frames.append([0, last // 3, last // 2 + 1, last + 5])           # start clamp, inside, inside, end clamp
    dev = []
    for i, x in enumerate(host):
        buf = torch.zeros(len(x) + 8, device=DEV)
        clip = buf[OFFSETS[i]: OFFSETS[i] + len(x)]                      # 0, 8, 4, 12 bytes off 16-byte alignment
        clip.copy_(torch.from_numpy(x))
        dev.append(clip)
    return host, dev, np.array(frames)


def _old_waves(host, frames, audio_length):
    from attention_based_tbn_amd.core.dataset import trim_audio
    return [trim_audio(x, int(f), audio_length) for x, fr in zip(host, frames) for f in fr]


@functools.lru_cache(maxsize=None)
def _layer_out(audio_length, spec_type):
    from attention_based_tbn_amd.core.dataset import AudioSegments
    host, dev, frames = _case(audio_length)
    return AudioSegments(audio_length, spec_type=spec_type)(dev, frames)["Audio"]


@pytest.mark.parametrize("audio_length", AUDIO_LENGTHS)
def test_windows_cover_clamps_and_every_alignment(audio_length):
    from attention_based_tbn_amd.core.dataset import audio_windows, window_table
    host, dev, frames = _case(audio_length)
    starts, L = audio_windows([len(x) for x in host], frames, audio_length)
    assert 1 + (L - 1) // 120 == WIDTH[audio_length]
    assert all(n % 4 for n in CLIP_LENGTHS[audio_length][:3])
    inside = 0
    for b, x in enumerate(host):
        assert starts[b, 0] == 0 and starts[b, 3] == len(x) - L and (np.diff(starts[b]) >= 0).all()
        inside += int(((starts[b] > 0) & (starts[b] < len(x) - L)).sum())
    assert inside >= 2                                                    # windows that no clamp touched
    table = window_table(dev, starts, L)
    assert set(((table // 4) % 4).tolist()) == {0, 1, 2, 3}              # absolute addresses: every residue of 16 B
    assert set((starts % 4).reshape(-1).tolist()) == {0, 1, 2, 3}        # and every start % 4


@pytest.mark.parametrize("audio_length", AUDIO_LENGTHS)
def test_stft_bit_identical_with_the_shipped_path(audio_length):
    from attention_based_tbn_amd.core.dataset import Spectrogram
    host, dev, frames = _case(audio_length)
    got = _layer_out(audio_length, "stft")
    W = WIDTH[audio_length]
    B = len(host)
    assert got.shape == (B, 4, 1, 256, W) and got.dtype == torch.float32
    want = Spectrogram()(torch.from_numpy(np.stack(_old_waves(host, frames, audio_length))).to(DEV))
    for s in range(4 * B):
        assert torch.equal(got.reshape(4 * B, 256, W)[s], want[s]), s


@pytest.mark.parametrize("audio_length", AUDIO_LENGTHS)
def test_padding_is_zeros_not_neighbouring_audio(audio_length):
    """every sample outside one window overwritten with NaN: that window's spectrogram must not move by a bit"""
    from attention_based_tbn_amd.core.dataset import AudioSegments, audio_windows
    host, dev, frames = _case(audio_length)
    clean = _layer_out(audio_length, "stft")
    clean_mel = _layer_out(audio_length, "logms")
    starts, L = audio_windows([len(x) for x in host], frames, audio_length)
    stft, logms = AudioSegments(audio_length), AudioSegments(audio_length, spec_type="logms")
    for b in range(len(host)):
        for j in range(4):
            buf = torch.full((len(host[b]) + 8,), float("nan"), device=DEV)
            off, s = OFFSETS[b], int(starts[b, j])
            buf[off + s: off + s + L] = dev[b][s: s + L]
            clip = buf[off: off + len(host[b])]
            assert torch.isnan(clip[:s]).all() and torch.isnan(clip[s + L:]).all() and clip.data_ptr() % 16 == dev[b].data_ptr() % 16
            got = stft([clip], frames[b:b + 1, j:j + 1])["Audio"][0, 0]
            assert torch.isfinite(got).all(), (b, j)
            assert torch.equal(got, clean[b, j]), (b, j)
            got = logms([clip], frames[b:b + 1, j:j + 1])["Audio"][0, 0]
            assert torch.isfinite(got).all() and torch.equal(got, clean_mel[b, j]), (b, j)


@pytest.mark.parametrize("audio_length", AUDIO_LENGTHS)
def test_stft_vs_oracle(audio_length):
    from oracle.stft import log_power_spectrogram, trim_audio
    host, dev, frames = _case(audio_length)
    got = _layer_out(audio_length, "stft").cpu().numpy()
    worst = 0.0
    for b in range(len(host)):
        for j in range(4):
            want = log_power_spectrogram(trim_audio(host[b], int(frames[b, j]), audio_length)[0])
            assert got[b, j, 0].shape == want.shape
            worst = max(worst, float(np.abs(got[b, j, 0] - want).max()))
    print(f"audio_length {audio_length}: max |stft - oracle| = {worst:.3e}")
    assert worst < 2e-3       # the bound of test_kernels_gpu.py::test_stft_logpower_vs_oracle


@pytest.mark.parametrize("audio_length", AUDIO_LENGTHS)
def test_log_mel_vs_oracle(audio_length):
    from oracle.stft import log_mel_spectrogram, trim_audio
    from attention_based_tbn_amd.core.dataset import AudioSegments
    host, dev, frames = _case(audio_length)
    out = _layer_out(audio_length, "logms")
    W = WIDTH[audio_length]
    assert out.shape == (len(host), 4, 1, 128, W)
    again = AudioSegments(audio_length, spec_type="logms")(dev, frames)["Audio"]
    assert torch.equal(out, again)                                        # fixed-order maximum: same bits every run
    got = out.cpu().numpy()
    worst = 0.0
    for b in range(len(host)):
        for j in range(4):
            want = log_mel_spectrogram(trim_audio(host[b], int(frames[b, j]), audio_length)[0])
            seg = got[b, j, 0]
            worst = max(worst, float(np.abs(seg - want).max()))
            assert abs(float(seg.max())) <= 1e-5 and float(seg.min()) >= -80.0 - 1e-3, (b, j, seg.max(), seg.min())
    print(f"audio_length {audio_length}: max |logms - oracle| = {worst:.3e} dB")
    assert worst < 2e-3       # dB, the bound of test_kernels_gpu.py::test_log_mel_spectrogram_vs_oracle


def test_log_mel_of_silence_is_exactly_zero_db():
    """10 log10(1e-10) - 10 log10(max(1e-10, 0)) = 0 everywhere, as the oracle gives it"""
    from oracle.stft import log_mel_spectrogram
    from attention_based_tbn_amd.core.dataset import AudioSegments
    silent = torch.zeros(40001, device=DEV)
    loud = torch.from_numpy(_case(1.279)[0][0]).to(DEV)
    out = AudioSegments(1.279, spec_type="logms")([silent, loud], [[0, 70], [0, 70]])["Audio"]
    assert torch.equal(out[0], torch.zeros_like(out[0]))
    assert float(out[1].min()) < -10.0
    assert not log_mel_spectrogram(np.zeros(30696, dtype=np.float32)).any()


def test_log_mel_many_segments_match_single_launches():
    """config-4 volume (96 segments, one workgroup each) against the same segments launched one at a time"""
    from attention_based_tbn_amd.core.dataset import Spectrogram
    L = 30696
    wave = 0.1 * torch.randn(96, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    wave[7] *= 1e-3
    wave[40, 1000:] = 0
    spec = Spectrogram(spec_type="logms")
    full = spec(wave)
    assert full.shape == (96, 128, 256) and torch.isfinite(full).all()
    for i in range(96):
        assert torch.equal(spec(wave[i:i + 1])[0], full[i]), i


LOUD_CASES = [(256, 256, 1.279, 8), (128, 256, 1.279, 8), (256, 420, 2.1, 13)]


@pytest.mark.parametrize("F,W,audio_length,T", LOUD_CASES)
def test_loud_prior_bit_equal_to_host(F, W, audio_length, T):
    from attention_based_tbn_amd.core.dataset import AudioSegments, attention_prior
    layer = AudioSegments(audio_length, prior_type="loud")
    assert layer.num_weights == T
    nblk = W // T
    g = torch.Generator().manual_seed(F + W)
    base = torch.rand(F, W, generator=g) * 10 - 14            # distinct background values, all below the planted ones
    specs = []
    for b in range(nblk):                                      # a unique maximum in each full block in turn
        s = base.clone()
        s[(37 * b + 5) % F, b * T + (3 * b) % T] = 5.0
        specs.append(s)
    if W % T:                                                  # the partial last block is louder still and must be ignored
        for b in (0, T // 2, nblk - 1):
            s = specs[b].clone()
            s[F // 2, nblk * T + (W % T) // 2] = 9.0
            specs.append(s)
    specs = torch.stack(specs)
    got = layer.prior(specs.to(DEV))
    assert got.shape == (len(specs), T, 1) and got.dtype == torch.float32
    seen = set()
    for i in range(len(specs)):
        want = attention_prior(specs[i].numpy(), audio_length, "loud")
        assert torch.equal(got[i].cpu(), want), (i, got[i].flatten().tolist(), want.flatten().tolist())
        seen.add(tuple(want.flatten().tolist()))
    assert len(seen) > 3                                       # rolled, floored and plain Gaussians all occurred


def test_loud_prior_tie_takes_the_highest_block():
    """equal block maxima: the device takes the highest block index (what NumPy's stable small-array sort gives for up to
    16 blocks).  The expectation is the host function on a copy whose highest tied block is made strictly the loudest, so
    the test does not lean on NumPy's order among exact ties."""
    from attention_based_tbn_amd.core.dataset import AudioSegments, attention_prior
    layer = AudioSegments(1.279, prior_type="loud")
    spec = torch.full((64, 8 * 12 + 3), -3.0)
    spec[5, 8 * 1 + 2] = spec[60, 8 * 7 + 7] = spec[9, 8 * 7] = 2.0     # blocks 1 and 7 tie
    untied = spec.clone()
    untied[60, 8 * 7 + 7] = 2.5
    want = attention_prior(untied.numpy(), 1.279, "loud")
    assert not torch.equal(want, attention_prior(None, 1.279, "gaussian").float())    # block 7 of T = 8: rolled
    assert torch.equal(layer.prior(spec[None].to(DEV))[0].cpu(), want)
    flat = torch.full((64, 8 * 12 + 3), -3.0)                  # every block equal: block 11 > T, the plain Gaussian
    assert torch.equal(layer.prior(flat[None].to(DEV))[0].cpu(), attention_prior(None, 1.279, "gaussian").float())


@pytest.mark.parametrize("prior_type", ["gaussian", "uniform", "loud"])
def test_layer_weights_equal_host_prior(prior_type):
    from attention_based_tbn_amd.core.dataset import AudioSegments, attention_prior
    host, dev, frames = _case(1.279)
    out = AudioSegments(1.279, prior_type=prior_type)(dev, frames)
    assert torch.equal(out["Audio"], _layer_out(1.279, "stft"))
    assert out["weights"].shape == (4, 4, 8, 1) and out["weights"].dtype == torch.float32 and out["weights"].is_contiguous()
    spec = out["Audio"].cpu().numpy()
    for b in range(len(host)):
        for j in range(4):
            assert torch.equal(out["weights"][b, j].cpu(), attention_prior(spec[b, j, 0], 1.279, prior_type)), (b, j)


def _families(L):
    fam = {}
    name = C.create_string_buffer(160)
    for i in range(L.tbn_profile_num_entries()):
        cnt, ms, fl = C.c_long(), C.c_double(), C.c_double()
        L.tbn_profile_entry(i, name, 160, C.byref(cnt), C.byref(ms), C.byref(fl))
        f_ = name.value.decode().split("<")[0]
        fam[f_] = fam.get(f_, 0) + cnt.value
    L.tbn_profile_reset()
    return fam


def test_launch_counts():
    from attention_based_tbn_amd._lib import lib
    from attention_based_tbn_amd.core.dataset import AudioSegments
    host, dev, frames = _case(1.279)
    L = lib()
    want = {("stft", None): {"stft_logpower_kernel": 1},
            ("logms", None): {"stft_logpower_kernel": 1, "mel_db_kernel": 1},
            ("stft", "loud"): {"stft_logpower_kernel": 1, "attn_prior_loud_kernel": 1},
            ("logms", "loud"): {"stft_logpower_kernel": 1, "mel_db_kernel": 1, "attn_prior_loud_kernel": 1},
            ("stft", "gaussian"): {"stft_logpower_kernel": 1}}
    for (spec_type, prior_type), fam_want in want.items():
        layer = AudioSegments(1.279, spec_type=spec_type, prior_type=prior_type)
        layer(dev, frames)                       # first use: twiddles, mel basis and the Gaussian go up
        torch.cuda.synchronize()
        L.tbn_profile_reset()
        L.tbn_profile_enable(1)
        layer(dev, frames)
        torch.cuda.synchronize()
        L.tbn_profile_enable(0)
        fam = _families(L)
        assert fam == fam_want, (spec_type, prior_type, fam)
        spec_launches = sum(v for k, v in fam.items() if k != "attn_prior_loud_kernel")
        assert spec_launches <= (1 if spec_type == "stft" else 3) and fam.get("attn_prior_loud_kernel", 0) <= 1


def test_layer_feeds_the_model():
    """the fixed-attention golden configuration (RGB + audio, 2 clips x 3 segments, T = 8): logits from the layer's
    "Audio" and "weights" equal those from the same spectrograms and priors built by the per-segment calls"""
    from attention_based_tbn_amd.core.dataset import AudioSegments, Spectrogram, attention_prior
    from tests.util import load_case
    from tests.test_model_gpu import build_product, to_dev
    cfg, modality, meta, data, inp, target = load_case("fixed_attn")
    assert cfg.model.attention.use_fixed and cfg.data.audio.audio_length == 1.279
    host, dev, frames = _case(1.279)
    host, dev, frames = host[:2], dev[:2], frames[:2, 1:]
    from attention_based_tbn_amd.config import load_config
    layer = AudioSegments.from_config(load_config(meta["overrides"] + ["model.attention.prior_type=loud"]))
    assert layer.prior_type == "loud" and layer.audio_length == 1.279
    new = layer(dev, frames)
    assert new["Audio"].shape == (2, 3, 1, 256, 256) and new["weights"].shape == (2, 3, 8, 1)
    spec = Spectrogram()(torch.from_numpy(np.stack(_old_waves(host, frames, 1.279))).to(DEV))
    old = {"Audio": spec.view(2, 3, 1, 256, 256),
           "weights": torch.stack([attention_prior(s, 1.279, "loud") for s in spec.cpu().numpy()]).view(2, 3, 8, 1).to(DEV)}
    model, _ = build_product(cfg, modality, meta)
    model.eval()
    rgb = inp["RGB"].to(DEV)
    with torch.no_grad():
        model({"RGB": rgb, **old})              # first use of this geometry: the engine's autotune
        out_old = {k: v.clone() for k, v in model({"RGB": rgb, **old}).items()}
        out_new = model({"RGB": rgb, **new})
    assert set(out_new) == set(out_old) and len(out_new) >= 2
    for k in out_old:
        assert torch.isfinite(out_new[k]).all() and torch.equal(out_new[k], out_old[k]), k

