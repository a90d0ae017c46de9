"""Helpers the tests of the device entropy decoder share (tests/test_jpeg_sync_cpu.py, tests/test_jpeg_sync_gpu.py): the
second fixture, the pack stage called through ctypes with guard words round its output buffers, the record layout of
csrc/tbn_jpeg_sync.h, and a short Python unstuffing of a scan."""
import ctypes as C
import os

import numpy as np

from tests import jpeg_ref as R
from tests.util import GOLDEN

FIXTURE = os.path.join(GOLDEN, "jpeg_sync_cases.npz")
MAX_INTERVALS = 1024
GUARD = 64                # guard bytes / elements on each side of a buffer
RECORD_GUARD = 0x5A
QUANT_GUARD = 0xA5A5
HEADER_WORDS = 8          # magic, n_intervals, scan_bytes, intervals_off, scan_off, record_bytes, restart_interval, reserved
TABLES_BYTES = 5728
MAGIC = 0x4A4E4254

_cases = None


def cases():
    global _cases
    if _cases is None:
        with np.load(FIXTURE) as z:
            _cases = {k[:-4]: z[k].tobytes() for k in z.files}
    return _cases


def blob(name):
    """a case of either fixture"""
    return cases()[name] if name in cases() else R.blob(name)


def decodable_names():
    """every case of both fixtures that the host stage decodes"""
    return R.color_names() + R.gray_names() + sorted(cases())


def mcus(geo):
    return (geo.blocks_w[0] // geo.hsamp[0]) * (geo.blocks_h[0] // geo.vsamp[0])


def expected_intervals(geo):
    return -(-mcus(geo) // geo.restart_interval) if geo.restart_interval else 1


def unstuff(data):
    """the entropy-coded segment of a well-formed file -> one bytes object per interval: cut at RSTn, FF 00 -> FF"""
    pos = 2
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        pos += 2 + (data[pos + 2] << 8 | data[pos + 3])
        if m == 0xDA:
            break
    parts, cur = [], bytearray()
    while True:
        c = data[pos]
        if c != 0xFF:
            cur.append(c)
            pos += 1
            continue
        q = pos + 1
        while data[q] == 0xFF:
            q += 1
        if data[q] == 0:
            cur.append(0xFF)
        elif 0xD0 <= data[q] <= 0xD7:
            parts.append(bytes(cur))
            cur = bytearray()
        else:
            assert data[q] == 0xD9
            parts.append(bytes(cur))
            return parts
        pos = q + 1


def pack(data, geo, max_intervals=MAX_INTERVALS, n_intervals=None):
    """tbn_jpeg_scan_pack into a record of exactly the declared capacity -> (rc, record bytes used, interval count,
    quant (components, 64), message); asserts the guard words on both sides of both buffers"""
    from attention_based_tbn_amd import _lib
    L = _lib.lib()
    if n_intervals is None:
        n_intervals = min(expected_intervals(geo), max_intervals)
    cap = int(L.tbn_jpeg_scan_pack_bytes(len(data), n_intervals))
    assert cap % 16 == 0 and cap >= 32 + TABLES_BYTES + 8 * n_intervals + len(data)
    nq = geo.components * 64
    raw = np.full(cap + 2 * GUARD + 16, RECORD_GUARD, np.uint8)
    lead = GUARD + (-(raw.ctypes.data + GUARD) % 16)                     # the record must be 16-byte aligned
    quant = np.full(nq + 2 * GUARD, QUANT_GUARD, np.uint16)
    count, used = C.c_int(-1), C.c_size_t(1 << 40)
    rc = L.tbn_jpeg_scan_pack(data, len(data), C.byref(geo), raw.ctypes.data + lead, cap, max_intervals,
                              quant.ctypes.data + 2 * GUARD, C.byref(count), C.byref(used))
    msg = (L.tbn_last_error() or b"").decode() if rc else ""
    assert (raw[:lead] == RECORD_GUARD).all() and (raw[lead + cap:] == RECORD_GUARD).all(), "write outside the record"
    assert (quant[:GUARD] == QUANT_GUARD).all() and (quant[GUARD + nq:] == QUANT_GUARD).all(), "write outside quant"
    assert used.value <= cap and used.value % 16 == 0
    return rc, raw[lead:lead + used.value].copy(), count.value, quant[GUARD:GUARD + nq].reshape(geo.components, 64).copy(), msg


def split_record(record):
    """record bytes (uint8 array) -> (header dict, intervals (n, 2) uint32, scan bytes)"""
    words = record[:4 * HEADER_WORDS].view(np.uint32)
    keys = ("magic", "n_intervals", "scan_bytes", "intervals_off", "scan_off", "record_bytes", "restart_interval", "reserved")
    h = dict(zip(keys, (int(w) for w in words)))
    n = h["n_intervals"]
    iv = record[h["intervals_off"]:h["intervals_off"] + 8 * n].view(np.uint32).reshape(n, 2)
    return h, iv, record[h["scan_off"]:h["scan_off"] + h["scan_bytes"]].tobytes()
