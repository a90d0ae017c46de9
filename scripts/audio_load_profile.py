"""Measurements behind profiles/audio_load.md (needs the MI355X; no fallback).

For a synthetic ten-minute recording as the camera files hold it (48 kHz stereo s16) and its 44.1 kHz twin:
(i)   the kernel alone: `resample_pcm` on PCM bytes that are already on the device, into a preallocated output, timed with
      device events; taps/s = outputs * 2W / time;
(ii)  `load_audio` end to end: RIFF walk, file read (page cache warm: the file was just written), upload of the raw bytes,
      the launch; host clock round work that ends in a device synchronise;
(iii) the parent's path for the pre-resampled equivalent: `read_wav` of a 24 kHz mono s16 file of the same duration plus
      the upload of its float32 samples -- what `Video_Dataset._waveform` does on a cache miss today.
All arms run in one process, alternated repetition by repetition after warm-up; median and minimum - maximum are printed,
and one JSON line at the end.  librosa and resampy are not installed here: their time is NOT measured.

    python scripts/audio_load_profile.py [--minutes 10] [--reps 11] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from attention_based_tbn_amd.core.dataset import load_audio, read_wav, wav_info  # noqa: E402
from attention_based_tbn_amd.core.dataset.audio_file import bank_geometry, resample_pcm  # noqa: E402


def write_s16(path, rate, channels, seconds, seed):
    rng = np.random.RandomState(seed)
    pcm = rng.randint(-8192, 8192, size=(int(rate * seconds), channels)).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return pcm.shape[0]


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sr", type=int, default=24000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audio_load_profile: no GPU (there is no fallback: nothing is measured without one)")
    seconds = args.minutes * 60
    res = dict(minutes=args.minutes, sr=args.sr, reps=args.reps, device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for rate in (48000, 44100):
            files[rate] = os.path.join(tmp, f"cam_{rate}.wav")
            write_s16(files[rate], rate, 2, seconds, rate)
        pre = os.path.join(tmp, "pre_24000.wav")
        write_s16(pre, args.sr, 1, seconds, 1)
        arms, meta = {}, {}
        for rate, path in files.items():
            info = wav_info(path)
            raw = np.fromfile(path, dtype=np.uint8, count=info.data_bytes, offset=info.data_offset)
            pcm = torch.from_numpy(raw).cuda()
            out = torch.empty(-(-info.frames * args.sr // rate), dtype=torch.float32, device="cuda")
            taps, phases, floats = bank_geometry(rate, args.sr)
            meta[rate] = dict(frames=info.frames, bytes=info.data_bytes, outputs=out.numel(), taps=taps, phases=phases)
            arms[f"kernel_{rate}"] = (device_ms, lambda pcm=pcm, info=info, rate=rate, out=out: resample_pcm(
                pcm, info.frames, info.channels, info.format, rate, args.sr, out=out))
            arms[f"load_audio_{rate}"] = (host_ms, lambda path=path: load_audio(path, args.sr))
        arms["read_wav_upload_pre_resampled"] = (host_ms, lambda: torch.from_numpy(read_wav(pre, args.sr)).cuda())
        times = {k: [] for k in arms}
        for rep in range(args.warmup + args.reps):
            for name, (clock, fn) in arms.items():          # alternated: every arm once per repetition
                t = clock(fn)
                if rep >= args.warmup:
                    times[name].append(t)
    for name, t in times.items():
        res[name] = stats(t)
    for rate, m in meta.items():
        k = res[f"kernel_{rate}"]
        m["taps_per_s"] = m["outputs"] * m["taps"] / (k["median"] * 1e-3)
        m["pcm_gb_per_s"] = m["bytes"] / (k["median"] * 1e-3) / 1e9
        res[f"geometry_{rate}"] = m
    for name in times:
        s = res[name]
        print(f"{name:32s} median {s['median']:9.3f} ms   ({s['min']:.3f} - {s['max']:.3f})")
    for rate, m in meta.items():
        print(f"{rate} -> {args.sr}: {m['frames']} frames, {m['outputs']} outputs x {m['taps']} taps, {m['phases']} phases: "
              f"{m['taps_per_s'] / 1e12:.3f} T taps/s, {m['pcm_gb_per_s']:.1f} GB/s of PCM")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
