"""The deflate encoder core (csrc/tbn_deflate.h) through its host twin tbn_deflate_host: every case of
tests/golden/deflate_cases.npz is read back by zlib and by the project's own decoder, the size conditions that prove LZ77
matching, dynamic codes and the stored fallback, and the .npz container around a stream.  No GPU."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

from tests import deflate_util as U

# The realistic 64 x 96 x 10 flow stack (61 440 bytes): this encoder writes 27 775 bytes, zlib level 1 -- the standard
# single-probe greedy setting, the class this match finder belongs to -- 30 061, zlib level 6 27 203 (both recorded in the
# fixture).  Measured ratio to level 1: 0.924 (to level 6: 1.021); the bound is that rounded up to the next 0.05.  The
# encoder is deterministic: the margin only leaves room for later harmless tuning.
FLOW_STACK_RATIO_TO_ZLIB1 = 0.95


def test_the_fixture_holds_the_cases_the_chunk_size_asks_for():
    c = U.chunk()
    sizes = {n: len(U.raw(n)) for n in U.names()}
    assert sizes == {"empty": 0, "one_byte": 1, "chunk_minus_1": c - 1, "chunk": c, "chunk_plus_1": c + 1,
                     "two_chunks_17": 2 * c + 17, "zeros_1mib": 1 << 20, "period_10": 3 * c, "uniform_random": 2 * c,
                     "skewed": 2 * c, "flow_stack": 64 * 96 * 10}
    assert U.raw("period_10")[:10] * (3 * c // 10) == U.raw("period_10")[:3 * c // 10 * 10]
    assert all(0 < U.zlib_size(n, 6) <= U.zlib_size(n, 1) for n in U.names())


def test_the_bound_is_the_closed_form():
    c = U.chunk()
    for n in (0, 1, c - 1, c, c + 1, 10 * c, 10 * c + 1, (1 << 31) - 1):
        assert U.bound(n) == n + 5 * max(1, -(-n // c))


@pytest.mark.parametrize("name", U.names())
def test_each_case_is_read_back_by_zlib_and_by_the_projects_decoder(name):
    from tests import inflate_util as I
    res, raw = U.host_result(), U.raw(name)
    i = U.plain_index(name)
    assert int(res.status[i]) == U.OK
    stream = U.stream(res, i)
    d = zlib.decompressobj(-15)
    assert d.decompress(stream) == raw and d.eof and d.unused_data == b""
    assert len(stream) <= U.bound(len(raw))
    assert int(res.crc[i]) == zlib.crc32(raw)
    outs, status, info, _ = I.run_host([I.Member(stream, len(raw), zlib.crc32(raw), method=8)])
    assert status == [I.OK] and info == [len(raw)] and outs[0] == raw


def test_one_table_guards_skipped_row_and_short_row():
    res = U.host_result()
    U.check_layout(res)
    rows = U.batch().rows
    assert [U.expected_status(r) for r in rows].count(U.SKIPPED) == 1
    assert [U.expected_status(r) for r in rows].count(U.CAPACITY) == 1
    # the neighbours of the refused rows are what they are alone
    for i, r in enumerate(rows):
        if U.expected_status(r) == U.OK:
            assert zlib.decompress(U.stream(res, i), -15) == U.raw(r.name)


def _size(name):
    res = U.host_result()
    return int(res.out_len[U.plain_index(name)])


def test_sizes_prove_long_matches_dynamic_codes_and_the_stored_fallback():
    n = 1 << 20
    assert _size("zeros_1mib") < n // 100            # only length-258 matches reach this: the fixed code's best is n / 158
    n = len(U.raw("period_10"))
    assert _size("period_10") < n // 100             # distance-10 matches are found
    n = len(U.raw("skewed"))
    assert _size("skewed") < 0.9 * n                 # no structure, 2 bits of entropy: the fixed code cannot do this
    n = len(U.raw("uniform_random"))
    assert _size("uniform_random") <= n + 5 * -(-n // 65535) + 16       # the stored fallback is taken


def test_ratio_on_the_realistic_stack_against_zlib_level_1():
    ours, z1, z6 = _size("flow_stack"), U.zlib_size("flow_stack", 1), U.zlib_size("flow_stack", 6)
    print(f"flow_stack: {ours} bytes, zlib level 1 {z1} (ratio {ours / z1:.3f}), level 6 {z6} (ratio {ours / z6:.3f})")
    assert ours <= FLOW_STACK_RATIO_TO_ZLIB1 * z1


def test_inconsistent_rows_are_refused_and_write_nothing():
    from attention_based_tbn_amd._lib import DeflateMember
    data = np.frombuffer(U.raw("flow_stack"), np.uint8)
    n = data.size
    cap = U.bound(n)
    bad = [dict(in_off=4, in_len=n), dict(in_off=2, in_len=16), dict(in_len=1 << 31), dict(out_off=8, out_cap=cap),
           dict(out_off=cap + 1, out_cap=0)]
    table = (DeflateMember * (len(bad) + 1))()
    for r in table:
        r.in_off, r.in_len, r.out_off, r.out_cap = 0, n, 0, cap
    for r, change in zip(table, bad):
        for k, v in change.items():
            setattr(r, k, v)
    out = np.full(cap, U.GUARD, np.uint8)
    out_len, crc, status = np.zeros(len(table), np.uint32), np.zeros(len(table), np.uint32), np.zeros(len(table), np.int32)
    # the good row last: whatever the refused rows wrote would be overwritten otherwise
    rc = U.lib().tbn_deflate_host(data.ctypes.data, n, C.addressof(table), len(bad), out.ctypes.data, cap, out_len.ctypes.data,
                                  crc.ctypes.data, status.ctypes.data)
    assert rc == 0 and status[:len(bad)].tolist() == [U.ROW] * len(bad) and (out == U.GUARD).all() and not out_len.any()
    rc = U.lib().tbn_deflate_host(data.ctypes.data, n, C.addressof(table), len(table), out.ctypes.data, cap, out_len.ctypes.data,
                                  crc.ctypes.data, status.ctypes.data)
    assert rc == 0 and status[-1] == U.OK and zlib.decompress(out[:out_len[-1]].tobytes(), -15) == data.tobytes()


def test_workspace_bytes_counts_one_slot_per_chunk():
    b = U.batch()
    L = U.lib()
    one = int(L.tbn_deflate_workspace_bytes(C.addressof(b.table), 1))          # the empty member: one slot
    slots = sum(max(1, -(-r.in_len // U.chunk())) for r in b.rows if not r.skip)
    assert one > U.chunk() and int(L.tbn_deflate_workspace_bytes(C.addressof(b.table), len(b.rows))) == slots * one


@pytest.mark.parametrize("shape", [(40, 56, 10), (256, 456, 10), (1, 1, 1)])
def test_npy_header_is_what_np_save_writes(shape):
    from attention_based_tbn_amd.core.dataset.npz_file import npy_header
    buf = io.BytesIO()
    a = np.zeros(shape, np.uint8)
    np.save(buf, a)
    assert npy_header(shape) == buf.getvalue()[:len(buf.getvalue()) - a.size]


def test_a_container_around_a_host_stream_is_read_by_np_load_and_npz_member():
    from attention_based_tbn_amd._lib import DeflateMember
    from attention_based_tbn_amd.core.dataset.npz_file import npy_header, npz_container, npz_member
    arr = np.frombuffer(U.raw("flow_stack"), np.uint8).reshape(64, 96, 10)
    member = np.frombuffer(npy_header(arr.shape) + arr.tobytes(), np.uint8)
    cap = U.bound(member.size)
    table = (DeflateMember * 1)()
    table[0].in_len, table[0].out_cap = member.size, cap
    out, out_len, crc, status = np.zeros(cap, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.ones(1, np.int32)
    rc = U.lib().tbn_deflate_host(member.ctypes.data, member.size, C.addressof(table), 1, out.ctypes.data, cap,
                                  out_len.ctypes.data, crc.ctypes.data, status.ctypes.data)
    assert rc == 0 and status[0] == 0
    blob = npz_container("flow", out[:out_len[0]].tobytes(), int(crc[0]), member.size)
    with np.load(io.BytesIO(blob)) as z:
        assert z.files == ["flow"] and np.array_equal(z["flow"], arr)
    rec = npz_member(blob)
    assert rec.host is False and rec.shape == (64, 96, 10) and rec.method == 8 and rec.crc == zlib.crc32(member.tobytes())
    assert rec.size == member.size and rec.data_length == int(out_len[0])
