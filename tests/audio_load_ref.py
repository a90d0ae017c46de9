"""The float64 NumPy restatement of the audio-file arithmetic (decode, downmix, resampy's `kaiser_best` resampler with exact
positions) that tests/test_audio_load_cpu.py and tests/test_audio_load_gpu.py check the library against, plus the .wav
writers they share.  Nothing here imports the package: it is the other side of the comparison.

The resampler is written as resampy's TAP LOOP (left wing over x[n - i], right wing over x[n + 1 + i], linear interpolation
in the filter table), vectorised over the outputs of a chunk; `bank` restates the polyphase form the kernel reads."""
import math
import struct

import numpy as np

NUM_ZEROS, NUM_TABLE = 64, 512
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
NWIN = NUM_ZEROS * NUM_TABLE + 1

RATIOS = [(48000, 24000), (96000, 24000), (44100, 24000), (22050, 24000), (16000, 24000), (8000, 24000), (23999, 24000)]
GEOMETRY = {(48000, 24000): (129, 1), (96000, 24000): (257, 1), (44100, 24000): (118, 80), (22050, 24000): (65, 160),
            (16000, 24000): (65, 3), (8000, 24000): (65, 3), (23999, 24000): (65, 24000)}        # (W, L), from the issue's table

_tables = {}


def filter_table(sr_orig, sr_new):
    """-> (win, delta, scale, step): the 32769 samples of the right half of the filter, their forward differences"""
    key = (sr_orig, sr_new)
    if key not in _tables:
        n = NUM_ZEROS * NUM_TABLE
        j = np.arange(n + 1, dtype=np.float64)
        win = np.kaiser(2 * n + 1, BETA)[n:] * ROLLOFF * np.sinc(ROLLOFF * j / NUM_TABLE)
        ratio = sr_new / sr_orig
        if ratio < 1:
            win = win * ratio
        delta = np.zeros_like(win)
        delta[:-1] = win[1:] - win[:-1]
        scale = min(1.0, ratio)
        _tables[key] = (win, delta, scale, int(scale * NUM_TABLE))
    return _tables[key]


def geometry(sr_orig, sr_new):
    """-> (W, L)"""
    step = filter_table(sr_orig, sr_new)[3]
    return -(-NWIN // step), sr_new // math.gcd(sr_orig, sr_new)


def out_length(frames, sr_orig, sr_new):
    return -(-frames * sr_new // sr_orig)


def _wing(win, delta, scale, step, fr, right):
    frac = scale * fr
    if right:
        frac = scale - frac
    idx = frac * NUM_TABLE
    off = idx.astype(np.int64)
    return off, idx - off, (NWIN - off) // step


def bank(sr_orig, sr_new):
    """the polyphase bank in float64, (2W, L): tap k multiplies x[n - W + 1 + k]"""
    win, delta, scale, step = filter_table(sr_orig, sr_new)
    W, L = geometry(sr_orig, sr_new)
    out = np.zeros((2 * W, L), dtype=np.float64)
    r = np.arange(L, dtype=np.int64)
    fr = ((r * sr_orig) % sr_new) / sr_new
    for right in (False, True):
        off, eta, count = _wing(win, delta, scale, step, fr, right)
        for i in range(W):
            live = i < count
            k = np.where(live, off + i * step, 0)
            w = np.where(live, win[k] + eta * delta[k], 0.0)
            out[W + i if right else W - 1 - i] = w
    return out


def resample(x, sr_orig, sr_new, chunk=1 << 15):
    """x: 1-D mono samples -> (y, mass), both float64 of ceil(len(x) * sr_new / sr_orig) samples: y the resampled signal
    (the padded tail sample 0), mass[t] = sum_k |w_k| |x_k| over the taps of output t (what a float32 error bound scales by)"""
    x = np.asarray(x, dtype=np.float64)
    frames = len(x)
    n_len = out_length(frames, sr_orig, sr_new)
    if sr_orig == sr_new:
        return x.copy(), np.abs(x)
    win, delta, scale, step = filter_table(sr_orig, sr_new)
    W = geometry(sr_orig, sr_new)[0]
    n_out = frames * sr_new // sr_orig
    y, mass = np.zeros(n_len), np.zeros(n_len)
    for a in range(0, n_out, chunk):
        t = np.arange(a, min(a + chunk, n_out), dtype=np.int64)
        pos = t * sr_orig
        n, fr = pos // sr_new, (pos % sr_new) / sr_new
        acc, absacc = np.zeros(len(t)), np.zeros(len(t))
        for right in (False, True):
            off, eta, count = _wing(win, delta, scale, step, fr, right)
            for i in range(W):
                src = n + 1 + i if right else n - i
                live = (i < count) & (src >= 0) & (src < frames)
                if not live.any():
                    continue
                k = np.where(live, off + i * step, 0)
                term = np.where(live, (win[k] + eta * delta[k]) * x[np.clip(src, 0, frames - 1)], 0.0)
                acc += term
                absacc += np.abs(term)
        y[t], mass[t] = acc, absacc
    return y, mass


def error_bound(mass, W):
    """|y - y_ref| <= (2W + 3) 2^-24 sum_k |w_k| |x_k| + 2^-126 for a float32 sum of 2W products of float32-rounded weights, in
    any order, with or without fused multiply-adds (2W - 1 additions, one product and one weight rounding per term,
    first-order terms bounded by (2W + 1) u, the rest covers the second order)"""
    return (2 * W + 3) * 2.0 ** -24 * mass + 2.0 ** -126


# ------------------------------------------------------------------------------------------------- samples and .wav files
WIDTH = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4}


def random_samples(fmt, frames, channels, seed):
    """uniform noise over the whole range of the format: integers (frames, channels) int64, or float32 in [-1, 1)"""
    rng = np.random.RandomState(seed)
    if fmt == "f32":
        return (rng.rand(frames, channels) * 2 - 1).astype(np.float32)
    bits = 8 * WIDTH[fmt]
    v = rng.randint(-(1 << (bits - 1)), 1 << (bits - 1), size=(frames, channels), dtype=np.int64)
    return v + 128 if fmt == "u8" else v           # u8 is stored offset: 0..255


def to_bytes(fmt, samples):
    s = np.asarray(samples)
    if fmt == "f32":
        return s.astype("<f4").tobytes()
    if fmt == "u8":
        return s.astype(np.uint8).tobytes()
    if fmt == "s24":
        b = s.astype("<i4").reshape(-1, 1).view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b).tobytes()
    return s.astype({"s16": "<i2", "s32": "<i4"}[fmt]).tobytes()


def decode(fmt, samples):
    """the float32 samples libsndfile hands out, (frames, channels)"""
    s = np.asarray(samples)
    if fmt == "f32":
        return s.astype(np.float32)
    if fmt == "u8":
        return ((s - 128) / 128.0).astype(np.float32)
    return (s / float(1 << (8 * WIDTH[fmt] - 1))).astype(np.float32)


def mono32(fmt, samples):
    """decode + the float32 downmix: the sum of the channels in channel order, divided by their number"""
    d = decode(fmt, samples)
    acc = d[:, 0].copy()
    for c in range(1, d.shape[1]):
        acc = (acc + d[:, c]).astype(np.float32)
    return acc if d.shape[1] == 1 else (acc / np.float32(d.shape[1])).astype(np.float32)


def write_wav(path, fmt, samples, rate, extensible=False, chunks_before_data=(), data_size=None, cut=None):
    """a RIFF / WAVE file written with `struct`: `chunks_before_data` = [(name, body bytes)] (odd bodies are padded),
    `data_size` overrides the declared size of the data chunk, `cut` truncates the finished file to that many bytes"""
    s = np.asarray(samples)
    channels, width = s.shape[1], WIDTH[fmt]
    tag = 3 if fmt == "f32" else 1
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels * width, channels * width,
                       8 * width)
    if extensible:
        guid_tail = bytes.fromhex("000000001000800000aa00389b71")
        body += struct.pack("<HHIH", 22, 8 * width, 0, tag) + guid_tail
    out = b"fmt " + struct.pack("<I", len(body)) + body
    for name, blob in chunks_before_data:
        out += name + struct.pack("<I", len(blob)) + blob + (b"\0" if len(blob) & 1 else b"")
    data = to_bytes(fmt, s)
    out += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    out = b"RIFF" + struct.pack("<I", 4 + len(out)) + b"WAVE" + out
    with open(path, "wb") as f:
        f.write(out if cut is None else out[:cut])
    return len(out) - len(data)          # the data offset
