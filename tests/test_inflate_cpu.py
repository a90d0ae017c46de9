"""The inflate decoder core (csrc/tbn_inflate.h) through its host twin tbn_inflate_host: every case of
tests/golden/inflate_cases.npz against zlib, byte for byte, and one stream per refusal.  No GPU."""
import zlib

import pytest

from tests import inflate_util as U


def test_the_fixture_has_the_structure_each_case_is_for():
    """the counts the generator's block walker stored beside the bytes"""
    s = U.structure
    assert s("stored_two_blocks")["stored"] == 2 and s("incompressible_level6")["stored"] >= 1
    assert s("fixed_with_matches")["fixed"] == 1 and s("fixed_with_matches")["overlapping"] >= 1
    assert s("zeros_distance_1")["max_dist"] == 1 and s("zeros_distance_1")["max_len"] == 258
    assert s("rle")["overlapping"] >= 10 and s("huffman_only")["matches"] == 0
    assert s("dynamic_blocks_deep_window")["dynamic"] >= 2 and s("dynamic_blocks_deep_window")["cross_block"] >= 100
    assert s("dynamic_blocks_deep_window")["max_dist"] >= 32000
    assert s("flow_like")["dynamic"] >= 2 and s("flow_like")["cross_block"] >= 10
    assert s("flow_like_sync_flush")["empty_stored"] == 1 and s("flow_like_full_flush")["empty_stored"] == 1
    assert s("hand_far_distances")["max_dist"] == 32768 and s("hand_far_distances")["output_bytes"] == 33487
    assert s("hand_repeat_into_distances")["repeat_into_dist"] == 1
    assert U.want("empty") == b"" and len(U.stream("empty")) == 2
    assert set(U.bad_names()) == set(U.BAD_STATUS)


@pytest.mark.parametrize("name", U.good_names())
def test_each_case_alone_equals_zlib(name):
    outs, status, info, _ = U.run_host([U.member(name)])
    assert status == [U.OK] and info == [len(U.want(name))]
    assert outs[0] == U.want(name)


def test_all_cases_in_one_table_with_a_stored_member_and_a_skipped_slot():
    names = U.good_names()
    raw = U.want("flow_like")
    members = [U.member(n) for n in names]
    members.insert(3, U.Member(raw, len(raw), zlib.crc32(raw), method=0))
    members.insert(5, U.member("rle", skip=True))
    outs, status, info, out = U.run_host(members, out_gap=7)
    expect = [U.want(n) for n in names]
    expect.insert(3, raw)
    expect.insert(5, None)
    for i, e in enumerate(expect):
        if e is None:
            assert status[i] == U.SKIPPED and info[i] == 0 and outs[i] == b"\xcd" * len(outs[i])
        else:
            assert status[i] == U.OK and info[i] == len(e) and outs[i] == e, i
    # the gaps between the outputs are untouched
    at = 0
    for m in members:
        at += m.size
        assert (out[at:at + 7] == 0xCD).all()
        at += 7


@pytest.mark.parametrize("name", U.bad_names())
def test_each_refusal_has_a_stream_that_produces_its_code(name):
    with pytest.raises(zlib.error):
        zlib.decompress(U.stream(name), -15)
    for size in (3, 64, 70000):                      # whatever the directory declares: the stream's own fault comes first
        _, status, info, _ = U.run_host([U.Member(U.stream(name), size, 0)])
        assert status == [U.BAD_STATUS[name]], (name, size)
        assert 0 <= info[0] <= size


def test_exhausted_input_declared_size_and_crc():
    for name in ("flow_like", "zeros_distance_1", "stored_two_blocks", "fixed_with_matches", "empty"):
        good = U.member(name)
        data, n = good.data, good.size
        cut = U.Member(data[:len(data) - 1], n, good.crc)
        mid = U.Member(data[:len(data) // 2], n, good.crc)
        long_ = U.Member(data, n + 1, good.crc)
        wrong = U.Member(data, n, good.crc ^ 0x80000000)
        members = [good, cut, mid, long_, wrong, good]
        expect = [U.OK, U.INPUT, U.INPUT, U.OUTPUT_SHORT, U.CRC, U.OK]
        if n > 0:
            members.append(U.Member(data, n - 1, good.crc))
            expect.append(U.OUTPUT_FULL)
        outs, status, info, _ = U.run_host(members, out_gap=5)
        assert status == expect, name
        assert outs[0] == outs[5] == U.want(name) and info[0] == info[3] == info[4] == n
        assert outs[4] == U.want(name)               # a CRC mismatch: the bytes are all there


def test_a_stored_member_is_a_copy_with_its_own_checks():
    raw = bytes(range(256)) * 5 + b"tail"
    crc = zlib.crc32(raw)
    members = [U.Member(raw, len(raw), crc, method=0), U.Member(raw, len(raw) + 1, crc, method=0),
               U.Member(raw, len(raw) - 1, crc, method=0), U.Member(raw, len(raw), crc + 1, method=0),
               U.Member(b"", 0, 0, method=0), U.Member(raw, len(raw), crc, method=12)]
    outs, status, info, _ = U.run_host(members)
    assert status == [U.OK, U.OUTPUT_SHORT, U.OUTPUT_FULL, U.CRC, U.OK, U.ROW]
    assert outs[0] == raw and info[0] == len(raw)


def test_rows_outside_the_buffers_are_refused_not_followed():
    import ctypes as C

    import numpy as np

    from attention_based_tbn_amd import _lib
    packed, table, out_bytes = U.pack([U.member("rle"), U.member("rle"), U.member("rle"), U.member("rle")])
    table[0].in_len = packed.size + 1                   # past the input
    table[1].out_off = out_bytes                        # past the output
    table[2].in_off = table[2].in_off + 2               # misaligned
    out = np.full(out_bytes, 0xCD, np.uint8)
    status, info = np.zeros(4, np.int32), np.zeros(4, np.int32)
    _lib.call("tbn_inflate_host", packed.ctypes.data, packed.size, C.addressof(table), 4, out.ctypes.data, out_bytes,
              status.ctypes.data, info.ctypes.data)
    assert status.tolist() == [U.ROW, U.ROW, U.ROW, U.OK]
    assert out[table[3].out_off:].tobytes() == U.want("rle") and (out[:table[3].out_off] == 0xCD).all()
    with pytest.raises(_lib.TbnHipError, match="null"):
        _lib.call("tbn_inflate_host", 0, 0, C.addressof(table), 4, out.ctypes.data, out_bytes, status.ctypes.data, info.ctypes.data)
    _lib.call("tbn_inflate_host", 0, 0, 0, 0, 0, 0, 0, 0)            # nothing to do
