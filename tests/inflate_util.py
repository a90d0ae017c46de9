"""What the inflate tests share: the fixture tests/golden/inflate_cases.npz (scripts/make_inflate_golden.py), zlib's output
of every good case computed once, and the member table of tbn_inflate_batch / tbn_inflate_host."""
import ctypes as C
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_cases.npz")

# include/tbn_hip.h
OK, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, SYMBOL, NO_EOB, DISTANCE, INPUT, OUTPUT_FULL, OUTPUT_SHORT, CRC, SKIPPED, ROW = range(13)

# what each refused stream of the fixture is refused with
BAD_STATUS = {
    "bad_block_type": BLOCK_TYPE,
    "bad_stored_len": STORED_LEN,
    "bad_oversubscribed_code_lengths": CODE_LENGTHS,
    "bad_incomplete_code_lengths": CODE_LENGTHS,
    "bad_oversubscribed_literals": CODE_LENGTHS,
    "bad_incomplete_literals": CODE_LENGTHS,
    "bad_repeat_without_previous": CODE_LENGTHS,
    "bad_repeat_past_the_end": CODE_LENGTHS,
    "bad_literal_length_symbol_286": SYMBOL,
    "bad_distance_symbol_30": SYMBOL,
    "bad_no_end_of_block": NO_EOB,
    "bad_distance_too_far_back": DISTANCE,
}

_cache = {}


def _load():
    if not _cache:
        with np.load(GOLDEN) as z:
            _cache["streams"] = {k: z[k].tobytes() for k in z.files if k != "structure"}
            _cache["structure"] = json.loads(z["structure"].tobytes().decode())
        _cache["want"] = {k: zlib.decompress(v, -15) for k, v in _cache["streams"].items() if not k.startswith("bad_")}
    return _cache


def stream(name):
    return _load()["streams"][name]


def want(name):
    """zlib's output of a good case (computed once)"""
    return _load()["want"][name]


def structure(name):
    return _load()["structure"][name]


def good_names():
    return sorted(_load()["want"])


def bad_names():
    return sorted(k for k in _load()["streams"] if k.startswith("bad_"))


class Member(object):
    """one member of a table: its compressed bytes and what the directory would say about it"""

    def __init__(self, data, size, crc, method=8, skip=False):
        self.data, self.size, self.crc, self.method, self.skip = data, size, crc, method, skip


def member(name, **kw):
    return Member(stream(name), len(want(name)), zlib.crc32(want(name)), **kw)


def pack(members, out_gap=0):
    """-> (packed input uint8 array, table (_lib.InflateMember * n), out_bytes): inputs at 16-byte aligned offsets, outputs
    one after the other with `out_gap` spare bytes between them"""
    from attention_based_tbn_amd._lib import InflateMember
    table = (InflateMember * len(members))()
    chunks, at, out_at = [], 0, 0
    for row, m in zip(table, members):
        row.in_off, row.in_len, row.out_off, row.out_len = at, len(m.data), out_at, m.size
        row.crc, row.method, row.skip = m.crc, m.method, int(m.skip)
        padded = -(-len(m.data) // 16) * 16
        chunks.append(np.frombuffer(m.data + bytes(padded - len(m.data)), np.uint8))
        at += padded
        out_at += m.size + out_gap
    packed = np.concatenate(chunks) if at else np.zeros(0, np.uint8)
    return packed, table, out_at


def run_host(members, out_gap=0):
    """tbn_inflate_host over the members -> (outputs as bytes per member, statuses, infos, the whole out array)"""
    from attention_based_tbn_amd import _lib
    packed, table, out_bytes = pack(members, out_gap)
    n = len(members)
    packed = np.ascontiguousarray(np.concatenate([packed, np.zeros(16, np.uint8)]))       # never a null pointer
    out = np.full(out_bytes + 16, 0xCD, np.uint8)
    status = np.full(n, -1, np.int32)
    info = np.full(n, -1, np.int32)
    _lib.call("tbn_inflate_host", packed.ctypes.data, packed.size - 16, C.addressof(table), n, out.ctypes.data, out_bytes,
              status.ctypes.data, info.ctypes.data)
    assert (out[out_bytes:] == 0xCD).all()
    outs = [out[row.out_off:row.out_off + row.out_len].tobytes() for row in table]
    return outs, status.tolist(), info.tolist(), out
