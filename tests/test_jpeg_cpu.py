"""Host stage of the JPEG decoder (csrc/tbn_jpeg_host.h through tbn_jpeg_parse / tbn_jpeg_entropy_decode), no GPU:
its coefficients, pushed through the numpy restatement of the reconstruction arithmetic (tests/jpeg_ref.py), must equal
libjpeg-turbo's pixels (tests/golden/jpeg_cases.npz) byte for byte; everything it does not support, and every damaged
stream, must come back as an error that names its cause, with the guard words round the output buffers intact
(jpeg_ref.entropy_decode checks them after every call)."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = R.color_names() + R.gray_names()


def _decode(name):
    data = R.blob(name)
    rc, geo, msg = R.parse(data)
    assert rc == 0, (name, msg)
    rc, coef, quant, msg = R.entropy_decode(data, geo)
    assert rc == 0, (name, msg)
    return geo, coef, quant


def _refused(data, *words, geo=None):
    """both entries refuse `data` and the message names the cause (every word of `words`, case-insensitive)"""
    rc, g, msg = R.parse(data)
    if geo is None and rc == 0:
        geo = g
    if rc != 0:
        assert rc < 0 and msg.startswith("jpeg:") and all(w.lower() in msg.lower() for w in words), (rc, msg)
    if geo is None:
        ok_rc, geo, _ = R.parse(R.blob("c_16x16_420_q90"))
        assert ok_rc == 0
    rc2, _, _, msg2 = R.entropy_decode(data, geo)
    assert rc2 < 0 and msg2.startswith("jpeg:") and all(w.lower() in msg2.lower() for w in words), (rc2, msg2)
    return msg2


def _segments(data):
    """[(offset of the 0xFF, marker code)] up to and including SOS, then the scan start and the EOI offset"""
    segs, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        segs.append((pos, m))
        pos += 2 + (data[pos + 2] << 8 | data[pos + 3])
        if m == 0xDA:
            break
    return segs, pos, data.rindex(b"\xff\xd9")


def _patch_sof(data, fn):
    segs, _, _ = _segments(data)
    off = [o for o, m in segs if m == 0xC0][0]
    b = bytearray(data)
    fn(b, off)
    return bytes(b)


def _drop_segment(data, marker, index=0):
    segs, _, _ = _segments(data)
    off = [o for o, m in segs if m == marker][index]
    ln = 2 + (data[off + 2] << 8 | data[off + 3])
    return data[:off] + data[off + ln:]


def test_header_signatures_and_version_are_unchanged():
    from attention_based_tbn_amd import _lib
    handle = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tbn_hip.h")).read()
    declared = set(re.findall(r"\b(tbn_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES)
    for name in ("tbn_jpeg_parse", "tbn_jpeg_entropy_decode", "tbn_jpeg_workspace_bytes", "tbn_jpeg_reconstruct"):
        assert name in declared and getattr(handle, name) is not None
    assert "tbn_jpeg_geometry" not in declared            # the struct shares its name with no function
    assert handle.tbn_capabilities() == 255 and (handle.tbn_version() & 0xFFFF) == 102
    assert len(re.findall(r"^#define TBN_CAP_", header, re.M)) == 8
    host = open(os.path.join(ROOT, "attention_based_tbn_amd", "csrc", "tbn_jpeg_host.h")).read()
    assert "hip" not in "".join(re.findall(r"^#include.*$", host, re.M)).lower()     # the host stage includes nothing from HIP


@pytest.mark.parametrize("name", ALL)
def test_parse_returns_the_geometry(name):
    rc, geo, msg = R.parse(R.blob(name))
    assert rc == 0, msg
    h, w = R.golden(name, "gray").shape[:2]
    color = name in R.color_names()
    assert (geo.width, geo.height, geo.components) == (w, h, 3 if color else 1)
    hs, vs = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[name.split("_")[2]] if color else (1, 1)
    assert (geo.hsamp[0], geo.vsamp[0]) == (hs, vs)
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    assert (geo.blocks_w[0], geo.blocks_h[0]) == (mx * hs, my * vs)
    total = 64 * mx * hs * my * vs
    if color:
        assert [geo.hsamp[1], geo.vsamp[1], geo.hsamp[2], geo.vsamp[2]] == [1, 1, 1, 1]
        assert [geo.blocks_w[1], geo.blocks_h[1], geo.blocks_w[2], geo.blocks_h[2]] == [mx, my, mx, my]
        total += 2 * 64 * mx * my
    assert geo.coef_count == total
    want_ri = {"q35r3opt": 3, "q100r1": 1, "q85r2": 2}.get(name.split("_")[-1], None)
    if want_ri is not None:
        assert geo.restart_interval == want_ri
    elif name.endswith("q90") or name.startswith("batch"):
        assert geo.restart_interval == 0


@pytest.mark.parametrize("name", ALL)
def test_entropy_decode_then_numpy_reconstruction_equals_libjpeg(name):
    geo, coef, quant = _decode(name)
    assert np.array_equal(R.reconstruct(coef, quant, geo, 3), R.golden(name, "bgr"))     # colour, or gray -> 3 channels
    assert np.array_equal(R.reconstruct(coef, quant, geo, 1), R.golden(name, "gray"))    # luma only, or gray


def test_sixteen_threads_decode_the_same_batch_identically():
    names = [n for n in R.color_names() if n.startswith("batch")] + ["big_256x456_420"]
    want = {n: _decode(n) for n in names}

    def work(_):
        return [(n,) + _decode(n)[1:] for n in names]

    with ThreadPoolExecutor(max_workers=16) as ex:
        results = list(ex.map(work, range(16)))
    for res in results:
        for n, coef, quant in res:
            assert np.array_equal(coef, want[n][1]) and np.array_equal(quant, want[n][2])


def test_fixture_pixels_are_what_pillow_decodes():
    Image = pytest.importorskip("PIL.Image")
    import io
    for name in R.color_names():
        im = Image.open(io.BytesIO(R.blob(name)))
        assert np.array_equal(np.asarray(im)[:, :, ::-1], R.golden(name, "bgr")), name
        im = Image.open(io.BytesIO(R.blob(name)))
        im.draft("L", im.size)
        assert np.array_equal(np.asarray(im)[:, :, None], R.golden(name, "gray")), name
    for name in R.gray_names():
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(R.blob(name))))[:, :, None], R.golden(name, "gray")), name


def test_fill_bytes_in_front_of_markers_are_skipped():
    name = "c_33x47_420_q35r3opt"
    data = R.blob(name)
    segs, scan, eoi = _segments(data)
    rsts = [scan + m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", data[scan:eoi])]    # a data 0xFF is followed by 0x00
    assert len(rsts) >= 2
    cuts = [o for o, _ in segs] + rsts + [eoi]
    out, last = b"", 0
    for c in cuts:
        out += data[last:c] + b"\xff\xff"
        last = c
    out += data[last:]
    geo, coef, quant = _decode(name)
    rc, geo2, msg = R.parse(out)
    assert rc == 0, msg
    rc, coef2, quant2, msg = R.entropy_decode(out, geo2)
    assert rc == 0, msg
    assert np.array_equal(coef, coef2) and np.array_equal(quant, quant2)


# ---------------------------------------------------------------- refusals ---------------------------------------------
def test_progressive_is_refused():
    _refused(R.blob("refuse_progressive"), "progressive")


def test_other_frame_types_and_arithmetic_coding_are_refused():
    base = R.blob("c_16x16_420_q90")
    _refused(_patch_sof(base, lambda b, o: b.__setitem__(o + 1, 0xC9)), "arithmetic")
    _refused(_patch_sof(base, lambda b, o: b.__setitem__(o + 1, 0xC1)), "SOF1", "not supported")
    _refused(_patch_sof(base, lambda b, o: b.__setitem__(o + 1, 0xC3)), "SOF3", "not supported")


def test_twelve_bit_precision_is_refused():
    _refused(_patch_sof(R.blob("c_16x16_420_q90"), lambda b, o: b.__setitem__(o + 4, 12)), "12-bit")


def test_four_components_are_refused():
    _refused(R.blob("refuse_cmyk"), "4 components")


def test_other_sampling_is_refused():
    base = R.blob("c_16x16_420_q90")
    for byte_off, value in ((11, 0x41), (11, 0x12), (14, 0x21), (11, 0x44)):       # luma 4x1, 1x2, chroma 2x1, luma 4x4
        _refused(_patch_sof(base, lambda b, o: b.__setitem__(o + byte_off, value)), "sampling")


def test_more_than_one_scan_is_refused():
    data = R.blob("g_16x16_q85r2")
    _, _, eoi = _segments(data)
    _refused(data[:eoi] + b"\xff\xda" + data[eoi + 2:] + b"\x00\x08\x01\x01\x00\x00\x3f\x00\xff\xd9", "more than one scan")
    # a colour file whose first scan carries one component only (non-interleaved)
    data = R.blob("c_16x16_444_q90")
    segs, scan, _ = _segments(data)
    sos = [o for o, m in segs if m == 0xDA][0]
    one = data[:sos] + b"\xff\xda\x00\x08\x01" + data[sos + 5:sos + 7] + data[scan - 3:]
    _refused(one, "more than one scan")


def test_a_missing_table_is_refused():
    base = R.blob("c_16x16_420_q90")
    n_dht = sum(1 for _, m in _segments(base)[0] if m == 0xC4)
    for i in range(n_dht):
        _refused(_drop_segment(base, 0xC4, i), "missing", "Huffman table")
    n_dqt = sum(1 for _, m in _segments(base)[0] if m == 0xDB)
    for i in range(n_dqt):
        _refused(_drop_segment(base, 0xDB, i), "missing quantisation table")


def _dc_ramp_stream(blocks):
    """a hand-made gray file of `blocks` 8x8 blocks in a row: one-code Huffman tables (DC: category 11, AC: EOB), every
    block adds +2047 to the DC prediction"""
    bits = ("0" + "1" * 11 + "0") * blocks
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    w = 8 * blocks
    return (b"\xff\xd8" + b"\xff\xdb\x00\x43\x00" + bytes([1] * 64) +
            b"\xff\xc0\x00\x0b\x08\x00\x08" + bytes([w >> 8, w & 255]) + b"\x01\x01\x11\x00" +
            b"\xff\xc4\x00\x14\x00" + bytes([1] + [0] * 15) + b"\x0b" +
            b"\xff\xc4\x00\x14\x10" + bytes([1] + [0] * 15) + b"\x00" +
            b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + scan + b"\xff\xd9")


def test_a_coefficient_that_leaves_int16_is_refused():
    data = _dc_ramp_stream(16)                    # 16 * 2047 = 32752 still fits
    rc, geo, msg = R.parse(data)
    assert rc == 0 and (geo.width, geo.height, geo.coef_count) == (128, 8, 16 * 64), msg
    rc, coef, quant, msg = R.entropy_decode(data, geo)
    assert rc == 0, msg
    assert coef.reshape(16, 64)[:, 0].tolist() == [2047 * (i + 1) for i in range(16)] and not coef.reshape(16, 64)[:, 1:].any()
    _refused(_dc_ramp_stream(17), "int16")        # 17 * 2047 = 34799


def test_geometry_mismatch_is_refused_and_names_both_sizes():
    rc, geo, _ = R.parse(R.blob("c_33x47_420_q90"))
    assert rc == 0
    msg = _refused(R.blob("c_35x50_420_q90"), "geometry mismatch", geo=geo)
    assert "50x35" in msg and "47x33" in msg
    rc, geo, _ = R.parse(R.blob("c_16x16_420_q90"))
    _refused(R.blob("c_16x16_422_q90"), "geometry mismatch", geo=geo)        # same size, other sampling
    _refused(R.blob("g_16x16_q85r2"), "geometry mismatch", geo=geo)          # same size, other component count


def test_a_marker_inside_the_scan_data_is_refused():
    data = R.blob("c_33x47_444_q90")                                          # no restart interval: no marker belongs there
    _, scan, eoi = _segments(data)
    mid = (scan + eoi) // 2
    _refused(data[:mid] + b"\xff\xd0" + data[mid:], "marker")
    _refused(data[:mid] + b"\xff\xd9", "marker")
    # a restart file whose markers come in the wrong order
    data = R.blob("c_33x47_444_q100r1")
    _, scan, _ = _segments(data)
    first = data.index(b"\xff\xd0", scan)
    _refused(data[:first] + b"\xff\xd3" + data[first + 2:], "RST0")


@pytest.mark.parametrize("name", ["c_33x47_420_q35r3opt", "c_17x31_422_q90", "g_35x50_q85r2", "c_8x8_444_q100r1"])
def test_truncated_streams_are_refused(name):
    data = R.blob(name)
    rc, geo, _ = R.parse(data)
    assert rc == 0
    segs, scan, eoi = _segments(data)
    cuts = {0, 1, 2, scan, eoi, eoi + 1} | {o for o, _ in segs} | {o + 2 for o, _ in segs}
    cuts |= {scan + m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", data[scan:eoi])}
    rng = np.random.default_rng(11)
    cuts |= set(int(v) for v in rng.integers(0, len(data), 200))
    for cut in sorted(cuts):
        rc, _, _, msg = R.entropy_decode(data[:cut], geo)
        assert rc < 0 and msg.startswith("jpeg:"), (cut, rc, msg)
        assert "ends early" in msg or "no SOI" in msg, (cut, msg)
        rc, _, pmsg = R.parse(data[:cut])
        assert (rc == 0) == (cut >= scan) and (rc == 0 or "ends early" in pmsg or "no SOI" in pmsg), (cut, pmsg)


@pytest.mark.parametrize("name", ["c_33x47_420_q35r3opt", "c_40x56_422_q90", "g_35x50_q85r2"])
def test_corrupted_scan_bytes_decode_or_fail_but_return(name):
    data = R.blob(name)
    rc, geo, _ = R.parse(data)
    assert rc == 0
    _, scan, eoi = _segments(data)
    rng = np.random.default_rng(12)
    failed = 0
    for _ in range(200):
        b = bytearray(data)
        b[int(rng.integers(scan, eoi))] = int(rng.integers(0, 256))
        rc, _, _, msg = R.entropy_decode(bytes(b), geo)              # the guard words are checked inside
        assert rc == 0 or (rc < 0 and msg.startswith("jpeg:") and len(msg) > 10), (rc, msg)
        failed += rc != 0
    assert failed > 0                                                # some of them must have been noticed


def test_null_arguments_are_refused():
    from attention_based_tbn_amd import _lib
    import ctypes as C
    data = R.blob("c_8x8_444_q90")
    assert _lib.lib().tbn_jpeg_parse(data, len(data), None) < 0
    geo = _lib.JpegGeometry()
    assert _lib.lib().tbn_jpeg_parse(None, 10, C.byref(geo)) < 0
    assert _lib.lib().tbn_jpeg_entropy_decode(data, len(data), None, None, None) < 0
    assert _lib.lib().tbn_jpeg_workspace_bytes(None, 1) == 0


def test_python_surface_fails_loudly_without_a_gpu(monkeypatch, tmp_path):
    import torch
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset import FrameReader, decode_jpegs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        decode_jpegs([R.blob("c_8x8_444_q90")])
    os.makedirs(tmp_path / "rgb" / "v")
    (tmp_path / "rgb" / "v" / "img_{:010d}.jpg".format(1)).write_bytes(R.blob("c_8x8_444_q90"))
    reader = FrameReader(str(tmp_path), "rgb", "flow", "jpg")
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        reader.read_rgb("v", [1])
    with pytest.raises(Exception, match="Problem reading file .*x_0000000002.jpg"):      # the missing file comes first
        reader.read_flow("v", [2])
