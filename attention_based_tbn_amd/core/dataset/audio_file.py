"""Audio files at any rate and sample format -> the mono float32 waveform at the target rate, on the device: what the
reference reads with `librosa.load(path, sr=data.audio.sampling_rate, mono=True)` (`core/dataset/dataset.py:401-414`,
`preprocessing/create_audio_pickle.py:47-49`).

  wav_info    a RIFF / WAVE chunk walker (PCM, IEEE float, WAVE_FORMAT_EXTENSIBLE), host only;
  load_audio  the data chunk's raw bytes go to the device as they are (2 to 4 times fewer bytes than decoded stereo
              float32) and ONE launch of `tbn_audio_load` decodes, downmixes and resamples them (csrc/audio_load.hip holds
              the arithmetic: resampy's `kaiser_best` restated as a polyphase bank, exact positions).

`read_wav` (dataset.py) stays what it was: 16-bit PCM at the target rate, read on the host.  This module is the opt-in
`Video_Dataset(audio_load="device")` path and the `preprocessing.create_audio_pickle` tool.
"""
import ctypes as C
import os
import struct
import threading
from collections import namedtuple

import numpy as np
import torch

from ..._lib import TbnHipError, call, lib, ptr, stream_ptr

U8, S16, S24, S32, F32 = range(5)       # include/tbn_hip.h TBN_AUDIO_*
FORMAT_NAMES = ("u8", "s16", "s24", "s32", "f32")
SAMPLE_WIDTH = (1, 2, 3, 4, 4)
MAX_CHANNELS = 8

WavInfo = namedtuple("WavInfo", "format channels rate frames data_offset data_bytes")

_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def wav_info(path):
    """-> WavInfo(format, channels, rate, frames, data_offset, data_bytes): `format` is one of U8 / S16 / S24 / S32 / F32,
    `data_offset` the file position of the first sample, `data_bytes` = frames * channels * width (a trailing partial frame
    is dropped).  Reads `fmt ` with tag 1 (PCM), 3 (IEEE float) or 0xFFFE (the tag is then the first two bytes of the
    sub-format), skips every other chunk (odd sizes are padded to even), and takes `data` clamped to the end of the file; a
    declared data size of 0 or 0xFFFFFFFF (a streamed writer that never patched the header) means "to the end of the
    file".  Anything else raises ValueError naming the path -- on the host, before any GPU use."""
    path = os.fspath(path)

    def bad(why):
        return ValueError(f"{path}: {why}")

    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise bad("not a RIFF / WAVE file")
        fmt, pos = None, 12
        while True:
            f.seek(pos)
            ck = f.read(8)
            if len(ck) < 8:
                raise bad("truncated: the file ends before its " + ("data" if fmt is not None else "fmt") + " chunk")
            name, ck_size = ck[:4], struct.unpack("<I", ck[4:])[0]
            body = pos + 8
            if name == b"fmt ":
                raw = f.read(min(ck_size, 40))
                if ck_size < 16 or len(raw) < 16:
                    raise bad("truncated fmt chunk")
                tag, channels, rate, _, block_align, bits = struct.unpack("<HHIIHH", raw[:16])
                if tag == _EXTENSIBLE:
                    if len(raw) < 26:
                        raise bad("truncated WAVE_FORMAT_EXTENSIBLE fmt chunk")
                    tag = struct.unpack("<H", raw[24:26])[0]
                fmt = (tag, channels, rate, block_align, bits)
            elif name == b"data":
                if fmt is None:
                    raise bad("data chunk before the fmt chunk")
                if ck_size in (0, 0xFFFFFFFF) or body + ck_size > size:
                    ck_size = size - body
                break
            pos = body + ck_size + (ck_size & 1)
    tag, channels, rate, block_align, bits = fmt
    if tag == _PCM and bits in (8, 16, 24, 32):
        code = {8: U8, 16: S16, 24: S24, 32: S32}[bits]
    elif tag == _FLOAT and bits == 32:
        code = F32
    elif tag == _FLOAT and bits == 64:
        raise bad("64-bit float samples are not read")
    else:
        raise bad(f"format tag {tag:#x} with {bits}-bit samples is not read (PCM 8 / 16 / 24 / 32 and 32-bit float are)")
    if not 1 <= channels <= MAX_CHANNELS:
        raise bad(f"{channels} channels, 1..{MAX_CHANNELS} are read")
    if rate < 1:
        raise bad(f"sampling rate {rate}")
    frame_bytes = channels * SAMPLE_WIDTH[code]
    if block_align != frame_bytes:
        raise bad(f"block_align {block_align}, but {channels} channels of {SAMPLE_WIDTH[code]} bytes are {frame_bytes}")
    frames = ck_size // frame_bytes
    return WavInfo(code, channels, rate, frames, body, frames * frame_bytes)


def output_tile():
    """the outputs one workgroup of the resampling kernel makes: its seams lie at the multiples (tests place sizes there)"""
    return int(lib().tbn_audio_tile())


def bank_geometry(sr_orig, sr_new):
    """-> (taps, phases, floats) of the polyphase bank; (0, 0, 0) at equal rates.  Host only."""
    taps, phases, floats = C.c_int(), C.c_int(), C.c_size_t()
    call("tbn_audio_bank_geometry", int(sr_orig), int(sr_new), C.byref(taps), C.byref(phases), C.byref(floats))
    return taps.value, phases.value, floats.value


def make_bank(sr_orig, sr_new):
    """the bank as a host float32 array (taps, phases); float64 arithmetic rounded once.  Host only."""
    taps, phases, floats = bank_geometry(sr_orig, sr_new)
    if floats == 0:
        raise ValueError(f"make_bank: {sr_orig} -> {sr_new} Hz needs no bank")
    bank = np.empty((taps, phases), dtype=np.float32)
    call("tbn_audio_make_bank", int(sr_orig), int(sr_new), bank.ctypes.data, floats)
    return bank


_banks, _banks_lock = {}, threading.Lock()


def _device_bank(sr_orig, sr_new, device):
    key = (int(sr_orig), int(sr_new), device)
    with _banks_lock:
        if key not in _banks:
            _banks[key] = torch.from_numpy(make_bank(sr_orig, sr_new)).to(device)     # a synchronous copy: usable on any stream
        return _banks[key]


def resample_pcm(pcm, frames, channels, fmt, sr_orig, sr_new, *, out=None):
    """`pcm`: a contiguous uint8 device tensor of frames * channels * width bytes of interleaved little-endian samples ->
    the 1-D float32 waveform of ceil(frames * sr_new / sr_orig) samples, one launch on the current stream.  `out`: write
    into this contiguous float32 tensor of exactly that length on the same device instead of a new one."""
    if not getattr(pcm, "is_cuda", False):
        raise TbnHipError("resample_pcm: the samples are not on the GPU (decode and resampling are HIP kernels, no CPU fallback)")
    if pcm.dtype != torch.uint8 or pcm.dim() != 1 or not pcm.is_contiguous():
        raise TbnHipError(f"resample_pcm: pcm must be a contiguous 1-D uint8 tensor (got {pcm.dtype}, shape {tuple(pcm.shape)})")
    frames, sr_orig, sr_new = int(frames), int(sr_orig), int(sr_new)
    if sr_orig < 1 or sr_new < 1:
        raise ValueError(f"resample_pcm: sampling rates {sr_orig} -> {sr_new}")
    out_len = -(-frames * sr_new // sr_orig)
    if out is not None and (out.device != pcm.device or out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous()
                            or out.numel() != out_len):
        raise TbnHipError(f"resample_pcm: out must be a contiguous 1-D float32 tensor of {out_len} samples on {pcm.device} "
                          f"(got {out.dtype}, shape {tuple(out.shape)}, {out.device})")
    with torch.cuda.device(pcm.device):
        if out is None:
            out = torch.empty(out_len, dtype=torch.float32, device=pcm.device)
        if frames > 0:
            bank = _device_bank(sr_orig, sr_new, pcm.device) if sr_orig != sr_new else None
            call("tbn_audio_load", ptr(pcm), pcm.numel(), frames, int(channels), int(fmt), sr_orig, sr_new, ptr(bank), ptr(out),
                 out_len, stream_ptr())
    return out


def load_audio(path, sr=24000, *, device="cuda", out=None):
    """`librosa.load(path, sr=sr, mono=True)[0]` as a 1-D float32 tensor on `device`, for a .wav file of any PCM width or
    32-bit float, 1..8 channels, any rate.  Launches on the current stream; the bank of a ratio is built once and cached
    per (file rate, sr, device).  `out`: see `resample_pcm`."""
    device = torch.device(device)
    if device.type != "cuda":
        raise TbnHipError(f"load_audio: device {device} -- decode and resampling are HIP kernels, there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if int(sr) != sr or sr < 1:
        raise ValueError(f"load_audio: sr={sr!r} is not a positive integer rate")
    info = wav_info(path)
    raw = np.fromfile(path, dtype=np.uint8, count=info.data_bytes, offset=info.data_offset)
    if raw.size != info.data_bytes:
        raise ValueError(f"{os.fspath(path)}: read {raw.size} of {info.data_bytes} data bytes")
    if info.frames == 0:
        raw = raw[:0]
    return resample_pcm(torch.from_numpy(raw).to(device), info.frames, info.channels, info.format, info.rate, int(sr), out=out)
