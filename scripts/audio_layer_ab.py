"""A/B of the audio data layer at config-4 volume: 32 untrimmed clips of unequal length, 3 segments each = 96 segments
of 1.279 s.  One row per representation:

  stft           parent: `trim_audio` slices -> torch.stack -> Spectrogram          new: AudioSegments (windows cut in the launch)
  logms          parent: the same staging + the torch-op log-mel (restated below)    new: AudioSegments(spec_type="logms")
  logms + loud   parent: ... + per-segment host `attention_prior(np.asarray(spec))`  new: ... + tbn_attn_prior_loud

The two arms alternate in one process (parent, new, parent, new, ...); each sample is the wall time of `--inner` calls
ending in a device synchronise.  Reported: median and range over the alternations, the outputs' agreement, and the
library's own launch count of the new arm from tbn_profile_* (the parent's STFT entry is not bracketed by the profiler; its
torch kernels are not the library's).  No gate on speed: this prints what it measured.

    python scripts/audio_layer_ab.py [--alternations 9] [--inner 20] [--out profiles/audio_layer.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from attention_based_tbn_amd import ops                                                     # noqa: E402
from attention_based_tbn_amd._lib import lib                                                # noqa: E402
from attention_based_tbn_amd.core.dataset import (AudioSegments, Spectrogram, attention_prior,   # noqa: E402
                                                  trim_audio)

AUDIO_LENGTH = 1.279


def parent_log_mel(stft0, spec_obj, wave):
    """`Spectrogram(spec_type="logms")` as the parent commit computed it: STFT kernel with eps = 0, exp, permuted copy,
    the mel projection as a Linear, amax / log10 / clamp / maximum in torch"""
    nseg = wave.shape[0]
    spec = stft0(wave)
    W = spec.shape[2]
    power = torch.exp(spec)
    rows = power.permute(0, 2, 1).reshape(nseg * W, 256)
    mel = ops.linear(rows, spec_obj._melbasis(wave.device), None).reshape(nseg, W, 128).permute(0, 2, 1)
    amin = 1e-10
    ref = mel.amax(dim=(1, 2), keepdim=True)
    db = 10.0 * torch.log10(torch.clamp(mel, min=amin)) - 10.0 * torch.log10(torch.clamp(ref, min=amin))
    return torch.maximum(db, db.amax(dim=(1, 2), keepdim=True) - 80.0).contiguous()


def library_launches(fn):
    L = lib()
    torch.cuda.synchronize()
    L.tbn_profile_reset()
    L.tbn_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    L.tbn_profile_enable(0)
    fam, name = {}, C.create_string_buffer(160)
    for i in range(L.tbn_profile_num_entries()):
        cnt, ms, fl = C.c_long(), C.c_double(), C.c_double()
        L.tbn_profile_entry(i, name, 160, C.byref(cnt), C.byref(ms), C.byref(fl))
        fam[name.value.decode()] = cnt.value
    L.tbn_profile_reset()
    return fam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("audio_layer_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    lengths = [36001 + 2731 * i + (i * i) % 97 for i in range(32)]            # 1.5 s ... 5 s, unequal, mostly odd
    clips = [(0.1 * torch.randn(n, generator=g)).to(dev) for n in lengths]
    frames = np.array([[int(n / 24000 * 60 * q) for q in (0.05, 0.5, 0.97)] for n in lengths])
    stft_old, mel_obj = Spectrogram(), Spectrogram(spec_type="logms")
    stft0 = Spectrogram(eps=0.0)

    def staged():
        return torch.stack([trim_audio(c, int(f), AUDIO_LENGTH) for c, fr in zip(clips, frames) for f in fr])

    def host_prior(spec):
        return torch.stack([attention_prior(s, AUDIO_LENGTH, "loud") for s in spec.cpu().numpy()]).to(dev)

    new_stft = AudioSegments(AUDIO_LENGTH)
    new_mel = AudioSegments(AUDIO_LENGTH, spec_type="logms")
    new_mel_loud = AudioSegments(AUDIO_LENGTH, spec_type="logms", prior_type="loud")

    def parent_mel_loud():
        s = parent_log_mel(stft0, mel_obj, staged())
        return s, host_prior(s)

    def new_mel_loud_fn():
        o = new_mel_loud(clips, frames)
        return o["Audio"], o["weights"]

    rows = [("stft", lambda: stft_old(staged()), lambda: new_stft(clips, frames)["Audio"]),
            ("logms", lambda: parent_log_mel(stft0, mel_obj, staged()), lambda: new_mel(clips, frames)["Audio"]),
            ("logms + loud prior", parent_mel_loud, new_mel_loud_fn)]
    lines = ["# Audio data layer: parent path vs `AudioSegments`", "",
             f"`scripts/audio_layer_ab.py --alternations {args.alternations} --inner {args.inner}` on {torch.cuda.get_device_name(0)}: "
             "32 clips of unequal length, 96 segments of 1.279 s; arms alternated in one process, each sample = wall time of "
             f"{args.inner} calls ending in a device synchronise, divided by {args.inner}.", "",
             "| row | parent ms / call: median (min - max) | new ms / call: median (min - max) | new / parent | outputs | library launches of the new arm |",
             "|---|---|---|---|---|---|"]
    for label, parent, new in rows:
        a, b = parent(), new()                            # warm-up of both arms (tables, twiddles, code objects) + agreement
        a0, b0 = (a[0], b[0]) if isinstance(a, tuple) else (a, b)
        b0 = b0.reshape(a0.shape)
        agree = "bit-identical" if torch.equal(a0, b0) else f"max abs diff {float((a0 - b0).abs().max()):.2e}"
        if isinstance(a, tuple):
            agree += "; prior " + ("bit-identical" if torch.equal(a[1].reshape(-1), b[1].reshape(-1)) else "DIFFERS")
        for fn in (parent, new):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        tp, tn = [], []
        for _ in range(args.alternations):
            for fn, acc in ((parent, tp), (new, tn)):
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3 / args.inner)
        fam = library_launches(new)
        mp, mn = statistics.median(tp), statistics.median(tn)
        lines.append(f"| {label} | {mp:.3f} ({min(tp):.3f} - {max(tp):.3f}) | {mn:.3f} ({min(tn):.3f} - {max(tn):.3f}) | "
                     f"{mn / mp:.2f} | {agree} | {sum(fam.values())}: " + ", ".join(f"{k} x{v}" for k, v in sorted(fam.items())) + " |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
