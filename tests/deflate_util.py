"""Shared by tests/test_deflate_cpu.py and tests/test_deflate_gpu.py: the cases of tests/golden/deflate_cases.npz, the member
table both entry points get (guard gaps between the out slots, a skipped row, a row one byte short of the bound) and the
host twin's answer to it, computed once."""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_cases.npz")
OK, CAPACITY, ROW, SKIPPED = 0, 1, 2, 3
GUARD = 0xCD
GAP = 7

Batch = namedtuple("Batch", "raw table rows out_bytes")
Row = namedtuple("Row", "name in_off in_len out_off out_cap skip")
Result = namedtuple("Result", "out out_len crc status")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in _golden()["names"]]


def raw(name):
    return _golden()["raw_" + name].tobytes()


def zlib_size(name, level):
    return int(_golden()["zlib%d" % level][names().index(name)])


def lib():
    from attention_based_tbn_amd import _lib
    return _lib.lib()


def chunk():
    return int(lib().tbn_deflate_chunk())


def bound(n):
    return int(lib().tbn_deflate_bound(n))


@functools.lru_cache(maxsize=None)
def batch():
    """every case once, then `flow_stack` again as a skipped row and `skewed` again with out_cap = bound - 1; the raw bytes
    packed at multiples of 4, the out slots GAP bytes apart (and GAP bytes behind the last)"""
    from attention_based_tbn_amd._lib import DeflateMember
    plan = [(n, False, 0) for n in names()]
    plan.insert(4, ("flow_stack", True, 0))
    plan.insert(7, ("skewed", False, -1))
    table = (DeflateMember * len(plan))()
    rows, parts, in_at, out_at = [], [], 0, 0
    for i, (name, skip, short) in enumerate(plan):
        data = raw(name)
        cap = bound(len(data)) + short
        rows.append(Row(name, in_at, len(data), out_at, cap, skip))
        r = table[i]
        r.in_off, r.in_len, r.out_off, r.out_cap, r.skip = in_at, len(data), out_at, cap, int(skip)
        padded = -(-len(data) // 4) * 4
        parts.append(np.frombuffer(data + b"\0" * (padded - len(data)), np.uint8))
        in_at += padded
        out_at += cap + GAP
    return Batch(np.concatenate(parts), table, rows, out_at)


def plain_index(name):
    """the row of case `name` that is neither skipped nor short"""
    return [i for i, r in enumerate(batch().rows) if r.name == name and expected_status(r) == OK][0]


def expected_status(row):
    return SKIPPED if row.skip else CAPACITY if row.out_cap < bound(row.in_len) else OK


@functools.lru_cache(maxsize=None)
def host_result():
    """tbn_deflate_host over batch(): the reference of the device test, computed once and never changed"""
    b = batch()
    n = len(b.rows)
    out = np.full(b.out_bytes, GUARD, np.uint8)
    out_len, crc, status = np.full(n, 0xCDCDCDCD, np.uint32), np.full(n, 0xCDCDCDCD, np.uint32), np.full(n, -1, np.int32)
    rc = lib().tbn_deflate_host(b.raw.ctypes.data, b.raw.size, C.addressof(b.table), n, out.ctypes.data, out.size,
                                out_len.ctypes.data, crc.ctypes.data, status.ctypes.data)
    assert rc == 0, rc
    for a in (out, out_len, crc, status):
        a.setflags(write=False)
    return Result(out, out_len, crc, status)


def stream(result, i):
    row = batch().rows[i]
    return result.out[row.out_off:row.out_off + int(result.out_len[i])].tobytes()


def check_layout(result):
    """what holds for any correct answer to batch(): statuses, nothing written for a refused row, the gaps untouched"""
    b = batch()
    for i, row in enumerate(b.rows):
        want = expected_status(row)
        assert int(result.status[i]) == want, (i, row.name, int(result.status[i]))
        used = int(result.out_len[i])
        if want != OK:
            assert used == 0 and int(result.crc[i]) == 0
        assert used <= row.out_cap
        assert (result.out[row.out_off + used:row.out_off + row.out_cap + GAP] == GUARD).all(), (i, row.name)
