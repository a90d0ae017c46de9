"""tbn_frames_to_tensor_batch (csrc/frames.hip) at the C-ABI: a batch of clips, each with its own geometry, in one launch.
The expectation is tbn_frames_to_tensor -- the pinned single-geometry entry -- called once per clip with that clip's row
of the table; the result must be bit-identical (`torch.equal`).  `out` and the device table are followed by 256 guard
bytes that must survive, `out` is pre-filled with a NaN bit pattern and rows no clip names must keep it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256
GUARD_VALUE = 0xCD
NAN_BITS = 0x7FC00ABC          # a quiet NaN with a payload: compared as int32, bit for bit


def _frames(rng, n, h, w, c):
    return torch.from_numpy(rng.randint(0, 256, (n, h, w, c)).astype(np.uint8)).cuda()


def _stats(n_stat):
    if n_stat == 0:
        return None, None
    mean = torch.tensor([0.408, 0.459, 0.502, 0.3][:n_stat], dtype=torch.float32).cuda()
    std = torch.tensor([0.9, 1.1, 0.75, 1.3][:n_stat], dtype=torch.float32).cuda()
    return mean, std


class _Out(object):
    """`out_rows` rows of (co, oh, ow) floats, NaN pattern, followed by guard bytes"""

    def __init__(self, out_rows, co, oh, ow):
        self.shape = (out_rows, co, oh, ow)
        self.floats = out_rows * co * oh * ow
        self.buf = torch.full((self.floats * 4 + GUARD_BYTES,), GUARD_VALUE, dtype=torch.uint8, device="cuda")
        self.bits()[:] = NAN_BITS

    def bits(self):
        return self.buf[:self.floats * 4].view(torch.int32).view(self.shape)

    def values(self):
        return self.buf[:self.floats * 4].view(torch.float32).view(self.shape)

    def guard_intact(self):
        return bool((self.buf[self.floats * 4:] == GUARD_VALUE).all())

    def untouched(self):
        return bool((self.bits() == NAN_BITS).all())


def _table(rows):
    """rows: dicts of tbn_frames_clip fields -> (host ctypes array, device bytes followed by guard bytes)"""
    from attention_based_tbn_amd._lib import FramesClip
    host = (FramesClip * max(1, len(rows)))()
    for i, r in enumerate(rows):
        host[i] = FramesClip(r["first_img"], r["box"][0], r["box"][1], r["box"][2], r["box"][3], r["resized"][0],
                             r["resized"][1], r["crop"][0], r["crop"][1], r["flip"], r["out_row"], 0)
    raw = np.frombuffer(bytes(host), dtype=np.uint8)[:len(rows) * C.sizeof(FramesClip)]
    dev = torch.full((raw.size + GUARD_BYTES,), GUARD_VALUE, dtype=torch.uint8, device="cuda")
    dev[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return host, dev, raw


def _batch(frames, rows, per_clip, ow, oh, stack, n_stat, out):
    """-> rc of tbn_frames_to_tensor_batch; asserts the guard bytes behind `out` and the table afterwards"""
    from attention_based_tbn_amd import _lib
    mean, std = _stats(n_stat)
    host, dev, raw = _table(rows)
    n, h, w, c = frames.shape
    rc = _lib.lib().tbn_frames_to_tensor_batch(_lib.ptr(frames), n, h, w, c, host, _lib.ptr(dev), len(rows), per_clip, ow,
                                               oh, stack, _lib.ptr(mean), _lib.ptr(std), n_stat, 1, _lib.ptr(out.buf),
                                               out.shape[0], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert out.guard_intact(), "write behind out"
    assert bool((dev[raw.size:] == GUARD_VALUE).all()) and np.array_equal(dev[:raw.size].cpu().numpy(), raw), "table changed"
    return rc


def _single(frames, r, per_clip, ow, oh, stack, n_stat):
    """the pinned entry for one clip's images and its row of the table -> (per_clip / stack, C * stack, oh, ow)"""
    from attention_based_tbn_amd import _lib
    mean, std = _stats(n_stat)
    _, h, w, c = frames.shape
    imgs = frames[r["first_img"]:r["first_img"] + per_clip].contiguous()
    want = torch.empty((per_clip // stack, c * stack, oh, ow), dtype=torch.float32, device="cuda")
    _lib.call("tbn_frames_to_tensor", _lib.ptr(imgs), per_clip, h, w, c, r["box"][0], r["box"][1], r["box"][2], r["box"][3],
              r["resized"][0], r["resized"][1], r["crop"][0], r["crop"][1], ow, oh, r["flip"], stack, _lib.ptr(mean),
              _lib.ptr(std), n_stat, 1, _lib.ptr(want), _lib.stream_ptr())
    return want


def _check_rows(out, frames, rows, per_clip, ow, oh, stack, n_stat):
    n = per_clip // stack
    for i, r in enumerate(rows):
        want = _single(frames, r, per_clip, ow, oh, stack, n_stat)
        got = out.values()[r["out_row"]:r["out_row"] + n]
        assert not bool(torch.isnan(want).any())
        assert torch.equal(got, want), (i, int((got != want).sum()))


def _row(first_img, box, resized, crop, flip, out_row):
    return dict(first_img=first_img, box=box, resized=resized, crop=crop, flip=flip, out_row=out_row)


def test_a_downscale_plain_copy_and_flipped_upscale_in_one_launch():
    rng = np.random.RandomState(0)
    frames = _frames(rng, 6, 37, 53, 3)
    rows = [_row(0, (5, 3, 30, 20), (24, 18), (4, 1), 0, 0),          # downscaled, window inside the resized box
            _row(2, (20, 11, 16, 16), (16, 16), (0, 0), 0, 2),        # a 16x16 box: no resize, beside resizing clips
            _row(4, (31, 17, 9, 11), (16, 16), (0, 0), 1, 4)]         # 9x11 -> 16x16, upscaled and flipped
    out = _Out(6, 3, 16, 16)
    assert _batch(frames, rows, 2, 16, 16, 1, 3, out) == 0
    _check_rows(out, frames, rows, 2, 16, 16, 1, 3)
    assert not bool(torch.isnan(out.values()).any())


def test_b_stacked_gray_two_row_tiles_reversed_rows_repeated_stats():
    rng = np.random.RandomState(1)
    frames = _frames(rng, 24, 61, 47, 1)
    rows = [_row(0, (3, 2, 40, 55), (30, 44), (5, 3), 1, 4),          # out rows in reversed order
            _row(8, (0, 0, 47, 61), (24, 40), (0, 0), 0, 2),
            _row(16, (10, 9, 24, 40), (24, 40), (0, 0), 1, 0)]
    out = _Out(6, 4, 40, 24)                                          # 40 rows: two row tiles per plane
    assert _batch(frames, rows, 8, 24, 40, 4, 2, out) == 0            # 2 statistics repeat over the 4 channels
    _check_rows(out, frames, rows, 8, 24, 40, 4, 2)
    assert not bool(torch.isnan(out.values()).any())


def test_c_rows_no_clip_names_are_not_touched_second_launch_fills_them():
    rng = np.random.RandomState(2)
    big, small = _frames(rng, 6, 40, 56, 3), _frames(rng, 6, 35, 50, 3)
    first = [_row(0, (7, 5, 35, 30), (16, 16), (0, 0), 1, 3),         # batch clips 1 and 3 of a 4-clip output
             _row(3, (0, 0, 56, 40), (28, 20), (6, 2), 0, 9)]
    out = _Out(12, 3, 16, 16)
    assert _batch(big, first, 3, 16, 16, 1, 3, out) == 0
    bits = out.bits()
    assert bool((bits[0:3] == NAN_BITS).all()) and bool((bits[6:9] == NAN_BITS).all())
    _check_rows(out, big, first, 3, 16, 16, 1, 3)
    second = [_row(3, (10, 0, 26, 35), (16, 16), (0, 0), 0, 0),       # clips 0 and 2, from frames of another size
              _row(0, (0, 9, 26, 26), (18, 18), (1, 2), 1, 6)]
    assert _batch(small, second, 3, 16, 16, 1, 3, out) == 0
    _check_rows(out, small, second, 3, 16, 16, 1, 3)
    _check_rows(out, big, first, 3, 16, 16, 1, 3)                     # ... and the first launch's rows are still there
    assert not bool(torch.isnan(out.values()).any())


def test_d_more_than_256_columns():
    rng = np.random.RandomState(3)
    frames = _frames(rng, 1, 10, 400, 2)
    for row in (_row(0, (20, 1, 360, 9), (300, 8), (0, 0), 1, 0), _row(0, (50, 2, 300, 8), (300, 8), (0, 0), 0, 0)):
        out = _Out(1, 2, 8, 300)
        assert _batch(frames, [row], 1, 300, 8, 1, 0, out) == 0
        _check_rows(out, frames, [row], 1, 300, 8, 1, 0)


def test_e_no_clips_launches_nothing():
    frames = _frames(np.random.RandomState(4), 2, 8, 8, 1)
    out = _Out(2, 1, 8, 8)
    assert _batch(frames, [], 1, 8, 8, 1, 0, out) == 0
    assert out.untouched()


def test_refusals_name_the_clip_and_write_nothing():
    from attention_based_tbn_amd import _lib
    rng = np.random.RandomState(5)
    frames = _frames(rng, 6, 37, 53, 1)
    good = [_row(0, (5, 3, 30, 20), (24, 18), (4, 1), 0, 0), _row(2, (0, 0, 16, 16), (16, 16), (0, 0), 1, 1),
            _row(4, (1, 1, 9, 11), (16, 16), (0, 0), 0, 2)]

    def refused(rows, needle, clip, per_clip=2, stack=2, out_rows=3):
        out = _Out(out_rows, stack, 16, 16)
        assert _batch(frames, rows, per_clip, 16, 16, stack, 1, out) < 0
        msg = _lib.lib().tbn_last_error().decode()
        assert needle in msg and "clip %d" % clip in msg, msg
        assert out.untouched()

    out = _Out(3, 2, 16, 16)
    assert _batch(frames, good, 2, 16, 16, 2, 1, out) == 0 and not out.untouched()
    refused([good[0], good[1], dict(good[2], first_img=5)], "outside the 6 frames", 2)
    refused([good[0], dict(good[1], box=(40, 0, 16, 16)), good[2]], "outside the 53x37 frame", 1)
    refused([good[0], good[1], dict(good[2], crop=(1, 0))], "outside the resized 16x16 box", 2)
    refused([good[0], dict(good[1], out_row=3), good[2]], "outside the 3 rows", 1)
    refused([dict(good[0], out_row=-1), good[1], good[2]], "outside the 3 rows", 0)
    refused([good[0], dict(good[1], out_row=2), good[2]], "overlapping output rows", 1)
    refused([dict(good[0], first_img=0), dict(good[1], first_img=3)], "multiple of the stack", 0, per_clip=3, stack=2)
    # a null table / frames pointer
    out = _Out(3, 2, 16, 16)
    host, dev, _ = _table(good)
    rc = _lib.lib().tbn_frames_to_tensor_batch(_lib.ptr(frames), 6, 37, 53, 1, host, None, 3, 2, 16, 16, 2, None, None, 0, 1,
                                               _lib.ptr(out.buf), 3, _lib.stream_ptr())
    assert rc < 0 and "null" in _lib.lib().tbn_last_error().decode() and out.untouched()
