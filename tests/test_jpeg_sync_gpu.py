"""Huffman decoding on the device (csrc/jpeg_entropy.hip through tbn_jpeg_entropy_decode_dev) and the opt-in Python surface
on top of it (decode_jpegs / FrameReader with entropy="device"), against the host stage's coefficients and libjpeg-turbo's
pixels.  Integer results: equality, no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref as R
from tests import jpeg_sync_util as U

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256
GUARD_VALUE = 0xCD
NO_RECORD = 0xFFFFFFFF
# single-byte changes in big_256x456_420's scan, chosen on the CPU with scripts/jpeg_sync_check.cpp --pick (both passed
# its sanitizer run with exact-size buffers): (file offset, new value)
ACCEPTED_CHANGE = (14261, 250)         # the host stage still decodes the file
REFUSED_CHANGE = (14809, 63)           # the host stage: "invalid Huffman code in the scan data (MCU 458 of 464 ...)"

_host = {}


def _want(name, data=None):
    """the host stage's (geo, coef, quant) of a case, computed once"""
    if name not in _host:
        data = U.blob(name) if data is None else data
        rc, geo, msg = R.parse(data)
        assert rc == 0, msg
        rc, coef, quant, msg = R.entropy_decode(data, geo)
        assert rc == 0, (name, msg)
        _host[name] = (geo, coef, quant)
    return _host[name]


def _guarded(nbytes, dev):
    return torch.full((nbytes + GUARD_BYTES,), GUARD_VALUE, dtype=torch.uint8, device=dev)


def _device_decode(blobs, geo, subseq_bits, skip=()):
    """pack on the host, tbn_jpeg_entropy_decode_dev on the current stream; coef, status, info and the workspace are
    followed by guard bytes -> (coef (n, coef_count) int16, status (n,), info (n, 2), quant (n, comps, 64))"""
    from attention_based_tbn_amd import _lib
    n = len(blobs)
    records, offsets, quants, total = [], [], [], 0
    for i, data in enumerate(blobs):
        rc, record, _, quant, msg = U.pack(data, geo)
        assert rc == 0 and len(record) > 0, msg
        quants.append(quant)
        if i in skip:
            offsets.append(NO_RECORD)
            continue
        offsets.append(total)
        records.append(record)
        total += len(record)
    dev = torch.device("cuda")
    packed = torch.from_numpy(np.concatenate(records) if records else np.zeros(16, np.uint8)).to(dev)
    offsets_d = torch.from_numpy(np.array(offsets, np.uint32).view(np.int32)).to(dev)
    coef_bytes = 2 * int(geo.coef_count)
    ws_bytes = int(_lib.lib().tbn_jpeg_entropy_workspace_bytes(C.byref(geo), n))
    assert ws_bytes == 16 * n
    coef, status, info, ws = (_guarded(b, dev) for b in (n * coef_bytes, 4 * n, 8 * n, ws_bytes))
    _lib.call("tbn_jpeg_entropy_decode_dev", _lib.ptr(packed), max(total, 16), _lib.ptr(offsets_d), n, C.byref(geo), subseq_bits,
              _lib.ptr(coef), _lib.ptr(status), _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
    torch.cuda.current_stream().synchronize()
    for name, buf, used in (("coef", coef, n * coef_bytes), ("status", status, 4 * n), ("info", info, 8 * n), ("workspace", ws, ws_bytes)):
        assert bool((buf[used:] == GUARD_VALUE).all()), "write behind " + name
    return (coef[:n * coef_bytes].cpu().numpy().view(np.int16).reshape(n, -1), status[:4 * n].cpu().numpy().view(np.int32),
            info[:8 * n].cpu().numpy().view(np.int32).reshape(n, 2), np.stack(quants))


def _check_one(name, subseq_bits):
    """-> (None or what is wrong with the decode of one case, lanes, rounds)"""
    geo, want, _ = _want(name)
    coef, status, info, _ = _device_decode([U.blob(name)], geo, subseq_bits)
    lanes, rounds = int(info[0, 0]), int(info[0, 1])
    print(name, "S", subseq_bits, "status", int(status[0]), "lanes", lanes, "rounds", rounds)
    problem = None
    if status[0] != 0:
        problem = (name, subseq_bits, "status", int(status[0]))
    elif not 1 <= rounds <= lanes <= U.MAX_INTERVALS:
        problem = (name, subseq_bits, "rounds", rounds, "lanes", lanes)
    elif not np.array_equal(coef[0], want):
        problem = (name, subseq_bits, "coefficients differ", int((coef[0] != want).sum()))
    return problem, lanes, rounds


def test_every_case_of_the_first_fixture_equals_the_host_stage():
    """1x1 up to 40x56 and the two frame-sized files; 4:4:4 / 4:2:2 / 4:2:0 / gray; restart intervals 0, 1, 2, 3 and 228"""
    bad = []
    for name in R.color_names() + R.gray_names():
        for subseq_bits in (0, 64):
            bad.append(_check_one(name, subseq_bits)[0])
    bad = [b for b in bad if b]
    assert not bad, bad


@pytest.mark.parametrize("name", ["camera_256x456_420_q90opt", "camera_256x456_gray_q60", "uniform_256x456_gray_q75",
                                  "ri8_264x264_gray_q75", "plain_264x264_gray_q75"])
@pytest.mark.parametrize("subseq_bits", [0, 64, 96])
def test_the_second_fixture_equals_the_host_stage(name, subseq_bits):
    problem, lanes, rounds = _check_one(name, subseq_bits)
    assert problem is None
    bits = 8 * len(b"".join(U.unstuff(U.blob(name))))
    if name == "camera_256x456_420_q90opt":
        assert lanes > 64                                   # several wavefronts
        assert bits > 64 * U.MAX_INTERVALS                  # at S = 64 the lanes do not fit: S grows
        if subseq_bits == 0:
            assert lanes == -(-bits // 1024)
    if name == "uniform_256x456_gray_q75" and subseq_bits == 0:
        assert rounds == lanes == -(-bits // 1024) and lanes > 1      # nothing synchronises except through the chain


def test_seven_table_sets_in_one_launch_on_a_side_stream():
    names = [n for n in R.color_names() if n.startswith("batch")]
    assert len(names) == 7
    geo = _want(names[0])[0]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        coef, status, info, quant = _device_decode([U.blob(n) for n in names], geo, 0)
        alone = _check_one("camera_256x456_420_q90opt", 0)[0]  # tables of its own (optimize=True)
    assert alone is None
    assert not status.any() and (info[:, 1] >= 1).all() and (info[:, 1] <= info[:, 0]).all()
    for i, name in enumerate(names):
        assert np.array_equal(coef[i], _want(name)[1]), name
        assert np.array_equal(quant[i], _want(name)[2]), name


def test_an_image_without_a_record_is_skipped_and_bad_arguments_are_refused():
    from attention_based_tbn_amd import _lib
    names = ["batch_40x56_420_q20", "batch_40x56_420_q55", "batch_40x56_420_q98"]
    geo = _want(names[0])[0]
    coef, status, info, _ = _device_decode([U.blob(n) for n in names], geo, 0, skip=(1,))
    assert status.tolist() == [0, 64, 0] and info[1].tolist() == [0, 0] and not coef[1].any()
    for i in (0, 2):
        assert np.array_equal(coef[i], _want(names[i])[1])
    dev = torch.device("cuda")
    packed, offsets, st, inf, ws = (torch.zeros(4096, dtype=torch.uint8, device=dev) for _ in range(5))
    big = torch.zeros(2 * int(geo.coef_count), dtype=torch.uint8, device=dev)
    args = lambda g, s: (_lib.ptr(packed), 4096, _lib.ptr(offsets), 1, C.byref(g), s, _lib.ptr(big), _lib.ptr(st), _lib.ptr(inf),
                         _lib.ptr(ws), 0)
    for s in (32, 48, 100, -64):
        with pytest.raises(_lib.TbnHipError, match="subseq_bits"):
            _lib.call("tbn_jpeg_entropy_decode_dev", *args(geo, s))
    wrong = _lib.JpegGeometry.from_buffer_copy(geo)
    wrong.blocks_w[1] = 7
    with pytest.raises(_lib.TbnHipError, match="block extents"):
        _lib.call("tbn_jpeg_entropy_decode_dev", *args(wrong, 0))
    # a record that is not one (zeros): a status, nothing else
    torch.cuda.synchronize()
    _lib.call("tbn_jpeg_entropy_decode_dev", *args(geo, 0))
    torch.cuda.synchronize()
    assert int(st[:4].view(torch.int32)[0]) == 32 and not big.any()


def test_decode_jpegs_on_the_device_gives_libjpeg_pixels():
    from attention_based_tbn_amd.core.dataset import decode_jpegs
    color, gray = R.blob("big_256x456_420"), R.blob("big_256x456_gray")
    got = decode_jpegs([color, color, color], entropy="device")
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 256, 456, 3)
    for i in range(3):
        assert np.array_equal(got[i].cpu().numpy(), R.golden("big_256x456_420", "bgr"))
    got = decode_jpegs([color], gray=True, threads=1, entropy="device")
    assert tuple(got.shape) == (1, 256, 456, 1) and np.array_equal(got[0].cpu().numpy(), R.golden("big_256x456_420", "gray"))
    got = decode_jpegs([gray] * 5, gray=True, threads=64, entropy="device")
    assert tuple(got.shape) == (5, 256, 456, 1)
    assert all(np.array_equal(got[i].cpu().numpy(), R.golden("big_256x456_gray", "gray")) for i in range(5))
    got = decode_jpegs([gray], entropy="device")
    assert np.array_equal(got[0].cpu().numpy(), R.golden("big_256x456_gray", "bgr"))


def test_host_routed_and_mixed_batches_equal_the_host_mode():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset import decode_jpegs
    routed = U.blob("ri1_264x264_gray_q75")                 # 1089 intervals: more than the lanes
    want = decode_jpegs([routed], gray=True, entropy="host")
    got = decode_jpegs([routed], gray=True, entropy="device")
    assert torch.equal(got, want)
    names = ["plain_264x264_gray_q75", "ri1_264x264_gray_q75", "ri8_264x264_gray_q75", "ri1_264x264_gray_q75",
             "plain_264x264_gray_q75"]
    blobs = [U.blob(n) for n in names]
    for gray in (True, False):
        got = decode_jpegs(blobs, gray=gray, threads=3, entropy="device")
        want = decode_jpegs(blobs, gray=gray, entropy="host")
        for i in range(len(names)):
            assert torch.equal(got[i], want[i]), (gray, i, names[i])
    assert torch.equal(want[0], want[1]) and torch.equal(want[0], want[2])   # the same pixels, three encodings
    with pytest.raises(TbnHipError, match="progressive"):
        decode_jpegs([R.blob("refuse_progressive")], entropy="device")
    with pytest.raises(TbnHipError, match="image 1.*ends early"):
        decode_jpegs([blobs[0], blobs[0][:len(blobs[0]) // 2]], entropy="device")


def test_frame_reader_with_device_entropy_over_the_reference_layout(tmp_path):
    from attention_based_tbn_amd.core.dataset import FrameReader
    vid = "P01_01"
    os.makedirs(tmp_path / "rgb" / vid)
    os.makedirs(tmp_path / "flow" / vid)
    rgb_names = ["batch_40x56_420_q20", "batch_40x56_420_q55", "batch_40x56_420_q98"]
    for idx, name in zip((3, 4, 17), rgb_names):
        (tmp_path / "rgb" / vid / "img_{:010d}.jpg".format(idx)).write_bytes(R.blob(name))
    flow_names = ["batch_40x56_420_q%d" % q for q in (20, 40, 55, 70, 80, 92)]
    for k, idx in enumerate((5, 6, 9)):
        (tmp_path / "flow" / vid / "x_{:010d}.jpg".format(idx)).write_bytes(R.blob(flow_names[2 * k]))
        (tmp_path / "flow" / vid / "y_{:010d}.jpg".format(idx)).write_bytes(R.blob(flow_names[2 * k + 1]))
    reader = FrameReader(str(tmp_path), "rgb", "flow", "jpg", entropy="device")
    got = reader.read_rgb(vid, np.array([3, 4, 17]))
    assert tuple(got.shape) == (3, 40, 56, 3)
    for i, name in enumerate(rgb_names):
        assert np.array_equal(got[i].cpu().numpy(), R.golden(name, "bgr"))
    got = reader.read_flow(vid, [5, 6, 9])
    assert tuple(got.shape) == (6, 40, 56, 1)
    for i, name in enumerate(flow_names):                                   # x, y, x, y, x, y
        assert np.array_equal(got[i].cpu().numpy(), R.golden(name, "gray")), (i, name)
    missing = os.path.join(str(tmp_path), "flow", vid, "y_{:010d}.jpg".format(7))
    (tmp_path / "flow" / vid / "x_{:010d}.jpg".format(7)).write_bytes(R.blob(flow_names[0]))
    with pytest.raises(Exception) as e:
        reader.read_flow(vid, [5, 7])
    assert missing in str(e.value)
    with pytest.raises(Exception) as e:
        reader.read_rgb(vid, [3, 5])
    assert os.path.join(str(tmp_path), "rgb", vid, "img_{:010d}.jpg".format(5)) in str(e.value)


def _changed(data, change):
    b = bytearray(data)
    assert b[change[0]] != change[1]
    b[change[0]] = change[1]
    return bytes(b)


def test_a_damaged_scan_the_host_stage_accepts_gives_the_same_pixels_on_both_paths():
    from attention_based_tbn_amd.core.dataset import decode_jpegs
    good = R.blob("big_256x456_420")
    bad = _changed(good, ACCEPTED_CHANGE)
    geo, want, _ = _want("big_256x456_420 accepted change", bad)
    coef, status, _, _ = _device_decode([bad], geo, 0)
    assert status[0] == 0 and np.array_equal(coef[0], want) and not np.array_equal(want, _want("big_256x456_420")[1])
    for gray in (False, True):
        got = decode_jpegs([good, bad], gray=gray, entropy="device")
        want_px = decode_jpegs([good, bad], gray=gray, entropy="host")
        assert torch.equal(got, want_px)
    assert not torch.equal(got[0], got[1])


def test_a_damaged_scan_the_host_stage_refuses_raises_its_message():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset import decode_jpegs
    good = R.blob("big_256x456_420")
    bad = _changed(good, REFUSED_CHANGE)
    rc, geo, _ = R.parse(bad)
    rc, _, _, msg = R.entropy_decode(bad, geo)
    assert rc == -1 and "invalid Huffman code" in msg
    _, status, _, _ = _device_decode([good, bad], geo, 0)
    assert status[0] == 0 and status[1] != 0
    with pytest.raises(TbnHipError, match=r"image 1: jpeg: invalid Huffman code") as e:
        decode_jpegs([good, bad], entropy="device")
    assert msg in str(e.value)
    with pytest.raises(TbnHipError, match=r"image 1: jpeg: invalid Huffman code"):
        decode_jpegs([good, bad], entropy="host")
