"""Device stage of the JPEG decoder (csrc/jpeg.hip: dequantisation + ISLOW IDCT, fancy upsampling + YCbCr -> BGR) and
the Python surface on top of it (core/dataset/frames.py), against libjpeg-turbo's pixels in tests/golden/jpeg_cases.npz.
Integer arithmetic: equality, no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref as R

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256
GUARD_VALUE = 0xCD


def _host(names):
    """entropy-decode `names` (one geometry) -> (geo, coef (n, coef_count) int16, quant (n, comps, 64) uint16)"""
    coefs, quants, geo = [], [], None
    for name in names:
        data = R.blob(name)
        if geo is None:
            rc, geo, msg = R.parse(data)
            assert rc == 0, msg
        rc, coef, quant, msg = R.entropy_decode(data, geo)
        assert rc == 0, (name, msg)
        coefs.append(coef)
        quants.append(quant)
    return geo, np.stack(coefs), np.stack(quants)


def _reconstruct(names, out_channels):
    """tbn_jpeg_reconstruct on the current stream, frames and workspace followed by guard bytes -> (n, H, W, C) uint8"""
    from attention_based_tbn_amd import _lib
    geo, coef, quant = _host(names)
    n = len(names)
    dev = torch.device("cuda")
    coef_d = torch.from_numpy(coef).to(dev)
    quant_d = torch.from_numpy(quant.view(np.int16)).to(dev)
    ws_bytes = int(_lib.lib().tbn_jpeg_workspace_bytes(C.byref(geo), n))
    assert ws_bytes == n * int(geo.coef_count)
    frame_bytes = n * geo.height * geo.width * out_channels
    frames = torch.full((frame_bytes + GUARD_BYTES,), GUARD_VALUE, dtype=torch.uint8, device=dev)
    ws = torch.full((ws_bytes + GUARD_BYTES,), GUARD_VALUE, dtype=torch.uint8, device=dev)
    _lib.call("tbn_jpeg_reconstruct", _lib.ptr(coef_d), _lib.ptr(quant_d), n, C.byref(geo), out_channels, _lib.ptr(frames),
              _lib.ptr(ws), _lib.stream_ptr())
    torch.cuda.current_stream().synchronize()
    assert bool((frames[frame_bytes:] == GUARD_VALUE).all()), "write behind the frames"
    assert bool((ws[ws_bytes:] == GUARD_VALUE).all()), "write behind the workspace"
    return frames[:frame_bytes].view(n, geo.height, geo.width, out_channels).cpu().numpy()


def test_reconstruct_equals_libjpeg_for_every_case_and_output_mode():
    bad = []
    for name in R.color_names() + R.gray_names():
        for mode, channels in (("bgr", 3), ("gray", 1)):       # colour | gray -> 3 channels, luma only | gray
            got = _reconstruct([name], channels)[0]
            want = R.golden(name, mode)
            if got.shape != want.shape or not np.array_equal(got, want):
                bad.append((name, mode, got.shape, int((got != want).sum()) if got.shape == want.shape else -1))
    assert not bad, bad


def test_seven_qualities_in_one_launch_on_a_side_stream():
    names = [n for n in R.color_names() if n.startswith("batch")]
    assert len(names) == 7
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got3 = _reconstruct(names, 3)
        got1 = _reconstruct(names, 1)
    for i, name in enumerate(names):
        assert np.array_equal(got3[i], R.golden(name, "bgr")), name
        assert np.array_equal(got1[i], R.golden(name, "gray")), name


def test_reconstruct_refuses_bad_arguments():
    from attention_based_tbn_amd import _lib
    geo, coef, quant = _host(["c_16x16_420_q90"])
    dev = torch.device("cuda")
    coef_d, quant_d = torch.from_numpy(coef).to(dev), torch.from_numpy(quant.view(np.int16)).to(dev)
    out = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(geo.coef_count), dtype=torch.uint8, device=dev)
    args = lambda g, ch, c=coef_d: (_lib.ptr(c), _lib.ptr(quant_d), 1, C.byref(g), ch, _lib.ptr(out), _lib.ptr(ws), 0)
    with pytest.raises(_lib.TbnHipError, match="out_channels"):
        _lib.call("tbn_jpeg_reconstruct", *args(geo, 2))
    bad = _lib.JpegGeometry.from_buffer_copy(geo)
    bad.blocks_w[1] = 7
    with pytest.raises(_lib.TbnHipError, match="block extents"):
        _lib.call("tbn_jpeg_reconstruct", *args(bad, 3))
    bad = _lib.JpegGeometry.from_buffer_copy(geo)
    bad.hsamp[0] = 4
    with pytest.raises(_lib.TbnHipError, match="sampling"):
        _lib.call("tbn_jpeg_reconstruct", *args(bad, 3))
    with pytest.raises(_lib.TbnHipError, match="aligned"):
        _lib.call("tbn_jpeg_reconstruct", *args(geo, 3, coef_d.view(-1)[1:]))
    torch.cuda.synchronize()


def test_decode_jpegs_on_the_frame_sized_files():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset import decode_jpegs
    color, gray = R.blob("big_256x456_420"), R.blob("big_256x456_gray")
    got = decode_jpegs([color, color, color])
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 256, 456, 3)
    for i in range(3):
        assert np.array_equal(got[i].cpu().numpy(), R.golden("big_256x456_420", "bgr"))
    got = decode_jpegs([color], gray=True, threads=1)
    assert tuple(got.shape) == (1, 256, 456, 1) and np.array_equal(got[0].cpu().numpy(), R.golden("big_256x456_420", "gray"))
    got = decode_jpegs([gray] * 5, gray=True, threads=64)
    assert tuple(got.shape) == (5, 256, 456, 1)
    assert all(np.array_equal(got[i].cpu().numpy(), R.golden("big_256x456_gray", "gray")) for i in range(5))
    got = decode_jpegs([gray])
    assert np.array_equal(got[0].cpu().numpy(), R.golden("big_256x456_gray", "bgr"))
    with pytest.raises(TbnHipError, match=r"mixed geometries.*56x40.*50x35"):
        decode_jpegs([R.blob("c_40x56_420_q90"), R.blob("c_35x50_420_q90")])
    with pytest.raises(TbnHipError, match="progressive"):
        decode_jpegs([R.blob("refuse_progressive")])
    with pytest.raises(TbnHipError, match="image 1.*ends early"):
        decode_jpegs([color, color[:len(color) // 2]])


def test_device_pipeline_takes_decoded_frames():
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import decode_jpegs, get_transforms
    tfs = get_transforms(load_config([]), ["RGB", "Flow"], "train")
    rgb = [R.blob("big_256x456_420")] * 3
    want_frames = torch.from_numpy(np.stack([R.golden("big_256x456_420", "bgr")] * 3))
    np.random.seed(3)
    a = tfs["RGB"](decode_jpegs(rgb))
    np.random.seed(3)
    b = tfs["RGB"](want_frames)
    assert a.shape[1] == 3 and torch.equal(a, b)
    flow = [R.blob("big_256x456_gray")] * 10
    want_frames = torch.from_numpy(np.stack([R.golden("big_256x456_gray", "gray")] * 10))
    np.random.seed(4)
    a = tfs["Flow"](decode_jpegs(flow, gray=True))
    np.random.seed(4)
    b = tfs["Flow"](want_frames)
    assert a.shape[1] == 10 and torch.equal(a, b)


def test_frame_reader_over_the_reference_layout(tmp_path):
    from attention_based_tbn_amd.core.dataset import FrameReader
    vid = "P01_01"
    os.makedirs(tmp_path / "rgb" / vid)
    os.makedirs(tmp_path / "flow" / vid)
    rgb_names = ["batch_40x56_420_q20", "batch_40x56_420_q55", "batch_40x56_420_q98"]
    for idx, name in zip((3, 4, 17), rgb_names):
        (tmp_path / "rgb" / vid / "img_{:010d}.jpg".format(idx)).write_bytes(R.blob(name))
    # distinct x and y images per index: six 4:2:0 colour files read as gray give six different luma planes
    flow_names = ["batch_40x56_420_q%d" % q for q in (20, 40, 55, 70, 80, 92)]
    for k, idx in enumerate((5, 6, 9)):
        (tmp_path / "flow" / vid / "x_{:010d}.jpg".format(idx)).write_bytes(R.blob(flow_names[2 * k]))
        (tmp_path / "flow" / vid / "y_{:010d}.jpg".format(idx)).write_bytes(R.blob(flow_names[2 * k + 1]))
    reader = FrameReader(str(tmp_path), "rgb", "flow", "jpg")
    got = reader.read_rgb(vid, np.array([3, 4, 17]))
    assert tuple(got.shape) == (3, 40, 56, 3)
    for i, name in enumerate(rgb_names):
        assert np.array_equal(got[i].cpu().numpy(), R.golden(name, "bgr"))
    got = reader.read_flow(vid, [5, 6, 9])
    assert tuple(got.shape) == (6, 40, 56, 1)
    for i, name in enumerate(flow_names):                                   # x, y, x, y, x, y
        assert np.array_equal(got[i].cpu().numpy(), R.golden(name, "gray")), (i, name)
    assert not np.array_equal(R.golden(flow_names[0], "gray"), R.golden(flow_names[1], "gray"))
    missing = os.path.join(str(tmp_path), "flow", vid, "y_{:010d}.jpg".format(7))
    (tmp_path / "flow" / vid / "x_{:010d}.jpg".format(7)).write_bytes(R.blob(flow_names[0]))
    with pytest.raises(Exception) as e:
        reader.read_flow(vid, [5, 7])
    assert missing in str(e.value)
    with pytest.raises(Exception) as e:
        reader.read_rgb(vid, [3, 5])
    assert os.path.join(str(tmp_path), "rgb", vid, "img_{:010d}.jpg".format(5)) in str(e.value)
