"""Times the general STFT kernel (tbn_stft_rate_windows, `Spectrogram(sampling_rate=...)`) at config-4 volume, 96 windows of
1.279 s, at 16, 24 (forced through the general kernel), 44.1 and 48 kHz and at 22.05 kHz (hop 110: the narrow-read path),
and writes profiles/stft_rates.md (`--out` names another file): us per call, TFLOP/s on the algorithmic 4 * 256 * win FLOP
per frame against the 157.3 TF/s fp32 MFMA peak, bytes in and out.

Like scripts/stft_profile.py the figures are warm ones, taken behind about 30 ms of the same launches: under MFMA load the
shader clock takes ~10 ms to settle, and a short burst after an idle GPU measures low.  At 24 kHz the kernel written for
(240, 120) and the general one run alternated in one process on the same input, several rounds each; the medians and their
ratio are reported.  The accuracy figures of tests/test_stft_rates_gpu.py (maximum distance from oracle/stft.py over its
inputs) go into the same file.  Under `rocprofv3 --kernel-trace --stats -- python3 scripts/stft_rates_profile.py` the same
launches appear per kernel."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from attention_based_tbn_amd.core.dataset import Spectrogram  # noqa: E402

PEAK_TF = 157.3
NSEG, SECONDS = 96, 1.279


class General(Spectrogram):
    _force_general = True


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def warm_us(fn):
    cold = timed(fn, 3, 20)
    return timed(fn, int(30e3 / cold) + 1, 200)


def lds_bytes(win, hop):
    """what the launcher asks for (csrc/stft.hip: stft_rate_launch_as)"""
    kg = (win + 7) // 8
    pad = 4 if hop % 4 == 0 and (hop // 4) % 2 == 0 else 0
    span = 63 * hop + 8 * kg
    return 4 * ((span + pad * ((span - 1) // hop) + 3) // 4 * 4)


def speed_rows():
    rows = []
    for rate, cls in ((16000, Spectrogram), (24000, General), (44100, Spectrogram), (48000, Spectrogram), (22050, Spectrogram)):
        spec = cls(sampling_rate=rate)
        L = int(SECONDS * rate)
        wave = 0.1 * torch.randn(NSEG, L, device="cuda")
        out = spec(wave)
        us = warm_us(lambda: spec(wave))
        W = out.shape[2]
        flops = 4.0 * 256 * spec.win_length * W * NSEG
        units = (spec.win_length + 7) // 8 * ((W + 63) // 64)          # tap groups x 64-frame blocks: a workgroup's work
        rows.append((rate, spec.win_length, spec.hop_length, "16-B reads" if spec.hop_length % 4 == 0 else "4-B reads",
                     lds_bytes(spec.win_length, spec.hop_length), L, W, us, flops / us / 1e6, wave.numel() * 4, out.numel() * 4,
                     1e3 * us / units))
    return rows


def ab_24khz(rounds=9):
    """the two kernels alternated on one input: medians over `rounds` warm measurements each"""
    special, general = Spectrogram(), General()
    wave = 0.1 * torch.randn(NSEG, int(SECONDS * 24000), device="cuda")
    assert torch.isfinite(general(wave)).all() and special(wave).shape == general(wave).shape
    warm_us(lambda: special(wave))
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(lambda: special(wave), 20, 100))
        b.append(timed(lambda: general(wave), 20, 100))
    return statistics.median(a), min(a), statistics.median(b), min(b)


def accuracy():
    """the inputs, references and bounds of tests/test_stft_rates_gpu.py"""
    from oracle.stft import log_mel_spectrogram, log_power_spectrogram
    from tests.stft_rates_util import RATES, lengths, log_mel_fp32, log_power_fp32, mel_signals, three_signals
    stft, mel = [], []
    for rate in RATES:
        spec = Spectrogram(sampling_rate=rate)
        worst = restated = 0.0
        for L in lengths(rate):
            waves = three_signals(rate, L)
            got = spec(torch.tensor(waves).cuda()).cpu().numpy()
            for i in range(3):
                ref = log_power_spectrogram(waves[i], sampling_rate=rate)
                worst = max(worst, float(np.abs(got[i] - ref).max()))
                restated = max(restated, float(np.abs(log_power_fp32(waves[i], rate) - ref).max()))
        stft.append((rate, spec.win_length, spec.hop_length, worst, restated))
    for rate in (16000, 48000):
        waves = mel_signals(rate)
        got = Spectrogram(sampling_rate=rate, spec_type="logms")(torch.tensor(waves).cuda()).cpu().numpy()
        refs = [log_mel_spectrogram(w, sampling_rate=rate) for w in waves]
        mel.append((rate, max(float(np.abs(got[i] - refs[i]).max()) for i in range(3)),
                    max(float(np.abs(log_mel_fp32(waves[i], rate) - refs[i]).max()) for i in range(3))))
    return stft, mel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_rates.md"))
    args = ap.parse_args()
    rows = speed_rows()
    s_med, s_min, g_med, g_min = ab_24khz()
    stft, mel = accuracy()
    md = ["# STFT at any sampling rate: the general kernel (scripts/stft_rates_profile.py)", "",
          f"{NSEG} windows of {SECONDS} s per call, warm figures (behind ~30 ms of the same launches), "
          f"one MI355X.  FLOP = 4 * 256 * win per frame; peak = {PEAK_TF} TF/s (fp32 MFMA).  The last column divides the time by "
          "ceil(win / 8) tap groups x ceil(W / 64) frame blocks, the work a workgroup really does: where it is level, what a "
          "rate loses against another is its rounding (W = 257 runs a fifth 64-frame block for one frame; win = 441 runs 448 "
          "taps), not its read path.", "",
          "| rate (Hz) | win | hop | frame reads | LDS per workgroup (B) | samples | W | us per call | TFLOP/s | % of peak | bytes in | bytes out | ns per tap group x frame block |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for rate, win, hop, path, lds, L, W, us, tf, bi, bo, unit in rows:
        note = " (general kernel forced)" if rate == 24000 else ""
        md.append(f"| {rate}{note} | {win} | {hop} | {path} | {lds} | {L} | {W} | {us:.1f} | {tf:.1f} | {100 * tf / PEAK_TF:.1f} | {bi} | {bo} "
                  f"| {unit:.0f} |")
    md += ["", "## 24 kHz: the kernel written for (240, 120) against the general one", "",
           "Alternated in one process on the same input, 9 rounds of 100 launches each.", "",
           "| kernel | median us | min us |", "|---|---|---|",
           f"| stft_logpower_kernel (the 24 kHz path) | {s_med:.1f} | {s_min:.1f} |",
           f"| stft_rate_kernel (forced) | {g_med:.1f} | {g_min:.1f} |", "",
           f"general / specialised = {g_med / s_med:.3f} (medians).  The specialised kernel stays the 24 kHz path.", "",
           "## Accuracy: maximum distance from oracle/stft.py on the inputs of tests/test_stft_rates_gpu.py", "",
           "Log-power STFT, all four lengths and three signals per rate; bound 2e-3.  \"fp32 NumPy\" is the restatement of "
           "tests/stft_rates_util.py (the same table and taps, groups of 8 taps) on the same inputs.", "",
           "| rate (Hz) | win | hop | kernel | fp32 NumPy |", "|---|---|---|---|---|"]
    md += [f"| {r} | {w} | {h} | {e:.3e} | {n:.3e} |" for r, w, h, e, n in stft]
    md += ["", "Log-mel (dB), 3 x 1.279 s; bound 2e-3 dB: the restatement stays below 5e-4 dB at both rates, so the bound of "
           "the 24 kHz test holds unchanged.", "", "| rate (Hz) | kernel | fp32 NumPy |", "|---|---|---|"]
    md += [f"| {r} | {e:.3e} | {n:.3e} |" for r, e, n in mel]
    text = "\n".join(md) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
