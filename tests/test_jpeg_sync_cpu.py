"""Host side of the device entropy decoder, no GPU: the pack stage (csrc/tbn_jpeg_sync.h through tbn_jpeg_scan_pack) against
a Python unstuffing written here, its refusals against the host stage's, and the new interface.  The decoder core
itself is checked against the host stage on the CPU by scripts/jpeg_sync_check.cpp (a sanitizer build), and on the
device by tests/test_jpeg_sync_gpu.py."""
import os
import re

import numpy as np
import pytest

from tests import jpeg_ref as R
from tests import jpeg_sync_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tbn_jpeg_scan_pack", "tbn_jpeg_scan_pack_bytes", "tbn_jpeg_entropy_workspace_bytes",
               "tbn_jpeg_entropy_decode_dev")


@pytest.mark.parametrize("name", U.decodable_names())
def test_pack_output_equals_a_python_unstuffing(name):
    data = U.blob(name)
    rc, geo, msg = R.parse(data)
    assert rc == 0, msg
    want_n = U.expected_intervals(geo)
    rc, record, count, quant, msg = U.pack(data, geo, max_intervals=2048)      # guard words are checked inside
    assert rc == 0, msg
    assert count == want_n
    h, iv, scan = U.split_record(record)
    assert h["magic"] == U.MAGIC and h["n_intervals"] == want_n and h["record_bytes"] == len(record)
    assert h["restart_interval"] == geo.restart_interval
    assert h["intervals_off"] == 32 + U.TABLES_BYTES and h["scan_off"] % 16 == 0
    parts = U.unstuff(data)
    assert len(parts) == want_n
    assert scan == b"".join(parts)
    starts = np.cumsum([0] + [len(p) for p in parts[:-1]])
    assert iv[:, 0].tolist() == [8 * int(s) for s in starts] and iv[:, 1].tolist() == [8 * len(p) for p in parts]
    assert not record[h["scan_off"] + h["scan_bytes"]:].any()                  # the padding reads as zeros
    rc, _, want_quant, msg = R.entropy_decode(data, geo)
    assert rc == 0 and np.array_equal(quant, want_quant)


def test_an_image_of_more_intervals_than_lanes_is_left_unpacked():
    data = U.blob("ri1_264x264_gray_q75")
    rc, geo, _ = R.parse(data)
    assert rc == 0 and U.expected_intervals(geo) == 1089
    rc, record, count, _, msg = U.pack(data, geo, max_intervals=U.MAX_INTERVALS, n_intervals=1)
    assert rc == 0 and count == 1089 and len(record) == 0, msg


def test_the_tables_are_the_image_s_own():
    """the optimize=True file carries tables of its own: its record differs from the standard-table file's"""
    tables = []
    for name in ("camera_256x456_420_q90opt", "big_256x456_420"):
        data = U.blob(name)
        rc, geo, _ = R.parse(data)
        rc, record, _, _, msg = U.pack(data, geo)
        assert rc == 0, msg
        tables.append(record[32:32 + U.TABLES_BYTES].tobytes())
    assert tables[0] != tables[1]
    slots = np.frombuffer(tables[0][-32:], np.int32)
    assert slots[:6].tolist() == [0, 2, 2, 1, 3, 3]      # luma DC, chroma DC x 2; luma AC, chroma AC x 2: four tables


def _pack_rc(data, geo):
    rc, record, _, _, msg = U.pack(data, geo, n_intervals=max(1, min(U.expected_intervals(geo), U.MAX_INTERVALS)))
    assert rc == 0 or (len(record) == 0 and msg.startswith("jpeg:"))
    return rc, msg


def test_pack_refusals_carry_the_host_stage_s_codes():
    rc, small, _ = R.parse(R.blob("c_16x16_420_q90"))
    assert rc == 0
    # a file cut before EOI: at the marker, inside the scan, inside the header
    data = R.blob("c_33x47_420_q35r3opt")
    rc, geo, _ = R.parse(data)
    for cut in (len(data) - 2, len(data) - 1, len(data) - 40, len(data) // 2, 30, 2, 0):
        want_rc, _, _, want_msg = R.entropy_decode(data[:cut], geo)
        got_rc, msg = _pack_rc(data[:cut], geo)
        assert got_rc == want_rc == -1 and ("ends early" in msg or "no SOI" in msg), (cut, got_rc, msg, want_msg)
    for name, word in (("refuse_progressive", "progressive"), ("refuse_cmyk", "4 components")):
        want_rc, _, _, want_msg = R.entropy_decode(R.blob(name), small)
        got_rc, msg = _pack_rc(R.blob(name), small)
        assert got_rc == want_rc == -3 and msg == want_msg and word in msg
    # a restart file whose markers come in the wrong order
    data = R.blob("c_33x47_444_q100r1")
    rc, geo, _ = R.parse(data)
    first = data.index(b"\xff\xd0", data.index(b"\xff\xda"))
    bad = data[:first] + b"\xff\xd3" + data[first + 2:]
    want_rc, _, _, want_msg = R.entropy_decode(bad, geo)
    got_rc, msg = _pack_rc(bad, geo)
    assert got_rc == want_rc == -1 and "RST0 expected" in msg and "RST0" in want_msg
    # a marker where none belongs, a geometry mismatch
    data = R.blob("c_33x47_444_q90")
    rc, geo, _ = R.parse(data)
    mid = (data.index(b"\xff\xda") + len(data)) // 2
    got_rc, msg = _pack_rc(data[:mid] + b"\xff\xd0" + data[mid:], geo)
    assert got_rc == -1 and "marker" in msg
    got_rc, msg = _pack_rc(R.blob("c_35x50_420_q90"), geo)
    assert got_rc == -1 and "geometry mismatch" in msg


def test_the_new_symbols_are_declared_and_bound():
    from attention_based_tbn_amd import _lib
    handle = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tbn_hip.h")).read()
    declared = set(re.findall(r"\b(tbn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and getattr(handle, name) is not None
    sync = open(os.path.join(ROOT, "attention_based_tbn_amd", "csrc", "tbn_jpeg_sync.h")).read()
    assert "hip" not in "".join(re.findall(r"^#include.*$", sync, re.M)).lower()     # the shared core includes nothing from HIP
    assert handle.tbn_jpeg_scan_pack_bytes(1000, 3) == 32 + U.TABLES_BYTES + 32 + 1008
    assert handle.tbn_jpeg_entropy_workspace_bytes(None, 1) == 0
    data = R.blob("c_8x8_444_q90")
    assert handle.tbn_jpeg_scan_pack(data, len(data), None, None, 0, 1, None, None, None) < 0


def test_the_entropy_keyword_is_checked_before_any_gpu_use(monkeypatch):
    import torch
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset import FrameReader, decode_jpegs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("GPU use")))
    with pytest.raises(ValueError, match="bogus"):
        decode_jpegs([R.blob("c_8x8_444_q90")], entropy="bogus")
    with pytest.raises(ValueError, match="bogus"):
        FrameReader("/nonexistent", "rgb", "flow", entropy="bogus")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for mode in ("host", "device"):
        with pytest.raises(TbnHipError, match="no CPU fallback"):
            decode_jpegs([R.blob("c_8x8_444_q90")], entropy=mode)
