"""Shared by tests/test_npz_chunks_cpu.py and tests/test_npz_chunks_gpu.py: the small member set of the chunk-index tests,
its streams and chunk index from the host twin tbn_deflate_host_indexed (computed once, never changed), and the tables
tbn_inflate_chunks / tbn_inflate_chunks_host get (outputs GAP guard bytes apart)."""
import ctypes as C
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import deflate_util as D

GUARD = 0xCD
GAP = 7
OK, DISTANCE, CRC, SKIPPED, ROW, SEGMENT = 0, 6, 10, 11, 12, 13

Case = namedtuple("Case", "name raw stream crc ends")
Tables = namedtuple("Tables", "packed members chunks begin n_chunks out_bytes")
Result = namedtuple("Result", "out status info chunk_status")


def lib():
    return D.lib()


def chunk():
    return D.chunk()


def _smooth(rng, n):
    """compressible, JPEG-like: a slow wave plus a little noise"""
    x = np.arange(n)
    return (128 + 60 * np.sin(x / 37.0) + 20 * np.sin(x / 5.3) + rng.randint(-2, 3, n)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def raws():
    """name -> raw bytes: sizes 0, 1, chunk - 1, chunk, chunk + 1, 2 chunks, 3 chunks + 5; smooth, seeded random (a
    stored chunk) and all zeros (dist < len matches); a random chunk between compressible ones; the fixture's flow_stack
    behind its .npy header (two chunks)"""
    from attention_based_tbn_amd.core.dataset.npz_file import npy_header
    rng = np.random.RandomState(11)
    c = chunk()
    out = [("empty", np.zeros(0, np.uint8)),
           ("one_byte", _smooth(rng, 1)),
           ("smooth_chunk_minus_1", _smooth(rng, c - 1)),
           ("random_chunk", rng.randint(0, 256, c).astype(np.uint8)),
           ("zeros_chunk_plus_1", np.zeros(c + 1, np.uint8)),
           ("smooth_two_chunks", _smooth(rng, 2 * c)),
           ("smooth_three_chunks_5", _smooth(rng, 3 * c + 5)),
           ("zeros_three_chunks_5", np.zeros(3 * c + 5, np.uint8)),
           ("random_between_smooth", np.concatenate([_smooth(rng, c), rng.randint(0, 256, c).astype(np.uint8), _smooth(rng, c + 5)])),
           ("flow_stack_npy", np.concatenate([np.frombuffer(npy_header((64, 96, 10)), np.uint8),
                                              np.frombuffer(D.raw("flow_stack"), np.uint8)]))]
    return {k: v.tobytes() for k, v in out}


def n_chunks_of(size):
    return max(1, -(-size // chunk()))


def deflate_host(datas, indexed):
    """tbn_deflate_host(_indexed) over the raw byte strings -> (streams, crcs, statuses, ends per member or None)"""
    from attention_based_tbn_amd._lib import DeflateMember
    n = len(datas)
    table = (DeflateMember * n)()
    parts, in_at, out_at = [], 0, 0
    for row, data in zip(table, datas):
        cap = D.bound(len(data))
        row.in_off, row.in_len, row.out_off, row.out_cap = in_at, len(data), out_at, cap
        padded = -(-len(data) // 4) * 4
        parts.append(np.frombuffer(data + bytes(padded - len(data)), np.uint8))
        in_at += padded
        out_at += cap
    raw = np.concatenate(parts + [np.zeros(4, np.uint8)])
    out = np.zeros(out_at, np.uint8)
    out_len, crc, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(n, -1, np.int32)
    counts = [n_chunks_of(len(d)) for d in datas]
    ends = np.full(sum(counts), 0xCDCDCDCD, np.uint32)
    args = [raw.ctypes.data, in_at, C.addressof(table), n, out.ctypes.data, out.size, out_len.ctypes.data, crc.ctypes.data,
            status.ctypes.data]
    if indexed:
        rc = lib().tbn_deflate_host_indexed(*args, ends.ctypes.data)
    else:
        rc = lib().tbn_deflate_host(*args)
    assert rc == 0, rc
    streams = [out[r.out_off:r.out_off + int(l)].tobytes() for r, l in zip(table, out_len)]
    split = np.split(ends, np.cumsum(counts)[:-1]) if indexed else [None] * n
    return streams, crc.tolist(), status.tolist(), [None if e is None else e.tolist() for e in split]


@functools.lru_cache(maxsize=None)
def cases():
    """the member set compressed by the host twin with its index: the reference of both suites"""
    names = list(raws())
    streams, crcs, statuses, ends = deflate_host([raws()[k] for k in names], True)
    assert not any(statuses), statuses
    return tuple(Case(k, raws()[k], s, c, tuple(e)) for k, s, c, e in zip(names, streams, crcs, ends))


def tables(members, skip=()):
    """`members`: (stream, raw size, crc, ends) each -> the Tables of tbn_inflate_chunks: streams at 16-byte aligned offsets,
    the outputs GAP guard bytes apart (and GAP behind the last), a chunk row per index entry; rows in `skip` carry the marker"""
    from attention_based_tbn_amd._lib import InflateChunk, InflateMember
    n = len(members)
    mt = (InflateMember * n)()
    total = sum(len(m[3]) for m in members)
    ct = (InflateChunk * max(total, 1))()
    begin = np.zeros(n + 1, np.uint32)
    parts, at, out_at, c = [], 0, 0, 0
    for i, (stream, size, crc, ends) in enumerate(members):
        row = mt[i]
        row.in_off, row.in_len, row.out_off, row.out_len, row.crc, row.method, row.skip = at, len(stream), out_at, size, crc, 8, int(i in skip)
        prev = 0
        for k, end in enumerate(ends):
            r = ct[c]
            r.in_off, r.in_len, r.out_off = at + prev, max(0, end - prev), out_at + k * chunk()
            r.out_len, r.member, r.last = max(0, min(chunk(), size - k * chunk())), i, int(k + 1 == len(ends))
            prev, c = end, c + 1
        begin[i + 1] = c
        padded = -(-len(stream) // 16) * 16
        parts.append(np.frombuffer(stream + bytes(padded - len(stream)), np.uint8))
        at += padded
        out_at += size + GAP
    return Tables(np.concatenate(parts), mt, ct, begin, total, out_at)


def fresh(t):
    n = len(t.members)
    return Result(np.full(t.out_bytes, GUARD, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32),
                  np.full(2 * max(t.n_chunks, 1), -1, np.int32))


def run_host(t):
    """tbn_inflate_chunks_host over the tables -> Result"""
    r = fresh(t)
    packed = np.ascontiguousarray(t.packed)
    rc = lib().tbn_inflate_chunks_host(packed.ctypes.data, packed.size, C.addressof(t.members), len(t.members),
                                       C.addressof(t.chunks), t.begin.ctypes.data, t.n_chunks, r.out.ctypes.data, r.out.size,
                                       r.status.ctypes.data, r.info.ctypes.data, r.chunk_status.ctypes.data)
    assert rc == 0, rc
    return r


def member_bytes(t, result, i):
    row = t.members[i]
    return result.out[row.out_off:row.out_off + row.out_len].tobytes()


def check_guards(t, result):
    for row in t.members:
        end = row.out_off + row.out_len
        assert (result.out[end:end + GAP] == GUARD).all(), row.out_off


def case_members():
    return [(c.stream, len(c.raw), c.crc, c.ends) for c in cases()]


@functools.lru_cache(maxsize=None)
def host_result():
    """the host chunk reader over the whole set as one batch, computed once"""
    t = tables(case_members())
    r = run_host(t)
    for a in r:
        a.setflags(write=False)
    return t, r


def crc32(data):
    return zlib.crc32(data) & 0xFFFFFFFF
