"""Chunk-indexed flow pickles without a GPU: the index tbn_deflate_host_indexed writes, the zip extra field that carries it
(core/dataset/npz_file.py) and the chunk reader's host twin tbn_inflate_chunks_host (the decoder core in segment mode,
csrc/tbn_inflate.h), over the member set of tests/npz_chunks_util.py."""
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest

from tests import npz_chunks_util as U

from attention_based_tbn_amd.core.dataset.npz_file import (npy_header, npz_chunk_index, npz_container, npz_member,
                                                           save_npz_arrays)


def _slices(case):
    prev = 0
    for k, end in enumerate(case.ends):
        yield k, case.stream[prev:end], case.raw[k * U.chunk():(k + 1) * U.chunk()]
        prev = end


def test_member_set_meets_its_conditions():
    """what the set was chosen for, from the host twin's index: chunk start offsets of all four residues mod 4, non-last
    chunks with and without the empty stored block behind them, a stored chunk"""
    t, _ = U.host_result()
    residues, with_block, without_block, stored = set(), 0, 0, 0
    for i, case in enumerate(U.cases()):
        assert len(case.ends) == U.n_chunks_of(len(case.raw)) and case.ends[-1] == len(case.stream)
        for k, data, raw in _slices(case):
            residues.add((t.members[i].in_off + case.ends[k - 1] if k else t.members[i].in_off) % 4)
            is_stored = len(data) == len(raw) + 5 and data[5:] == raw
            stored += is_stored
            if k + 1 < len(case.ends) and not is_stored:
                # the empty stored block's last four bytes are 00 00 FF FF: without them the chunk is still whole
                d = zlib.decompressobj(-15)
                ends_with_block = data[-4:] == b"\x00\x00\xff\xff" and d.decompress(data[:-4]) == raw
                with_block += ends_with_block
                without_block += not ends_with_block
    assert residues == {0, 1, 2, 3}
    assert with_block >= 1 and without_block >= 1 and stored >= 1


def test_indexed_deflate_equals_plain_deflate():
    names = [c.name for c in U.cases()]
    streams, crcs, statuses, _ = U.deflate_host([U.raws()[k] for k in names], False)
    assert not any(statuses)
    for case, s, c in zip(U.cases(), streams, crcs):
        assert case.stream == s and case.crc == c == U.crc32(case.raw), case.name
        assert zlib.decompress(case.stream, -15) == case.raw
        for k, data, raw in _slices(case):
            d = zlib.decompressobj(-15)
            assert d.decompress(data) == raw, (case.name, k)
            assert d.unused_data == b""
            assert d.eof == (k + 1 == len(case.ends)), (case.name, k)


def test_refused_rows_have_zero_entries():
    """a row one byte short of the bound, a skipped row and a good one: the index has entries for all three"""
    import ctypes as C
    from attention_based_tbn_amd._lib import DeflateMember
    data = U.raws()["smooth_two_chunks"]
    raw = np.frombuffer(data, np.uint8)
    cap = U.D.bound(len(data))
    table = (DeflateMember * 3)()
    for i, (c, skip) in enumerate([(cap - 1, 0), (cap, 1), (cap, 0)]):
        table[i].in_off, table[i].in_len, table[i].out_off, table[i].out_cap, table[i].skip = 0, len(data), i * cap, c, skip
    out = np.zeros(3 * cap, np.uint8)
    out_len, crc, status = np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.int32)
    ends = np.full(6, 0xCDCDCDCD, np.uint32)
    rc = U.lib().tbn_deflate_host_indexed(raw.ctypes.data, raw.size, C.addressof(table), 3, out.ctypes.data, out.size,
                                          out_len.ctypes.data, crc.ctypes.data, status.ctypes.data, ends.ctypes.data)
    assert rc == 0 and status.tolist() == [1, 3, 0]
    want = U.cases()[[c.name for c in U.cases()].index("smooth_two_chunks")].ends
    assert ends.tolist() == [0, 0, 0, 0] + list(want)


def test_host_chunk_reader_and_guards():
    t, r = U.host_result()
    assert r.status.tolist() == [0] * len(U.cases())
    for i, case in enumerate(U.cases()):
        assert U.member_bytes(t, r, i) == case.raw, case.name
        assert int(r.info[i]) == len(case.raw)
    assert r.chunk_status[:t.n_chunks].tolist() == [0] * t.n_chunks
    U.check_guards(t, r)


def test_host_chunk_reader_skip():
    t = U.tables(U.case_members(), skip={5})
    r = U.run_host(t)
    assert r.status.tolist() == [U.SKIPPED if i == 5 else 0 for i in range(len(U.cases()))]
    row = t.members[5]
    assert (r.out[row.out_off:row.out_off + row.out_len] == U.GUARD).all() and int(r.info[5]) == 0
    U.check_guards(t, r)


def _flow_case():
    return U.cases()[[c.name for c in U.cases()].index("flow_stack_npy")]


def test_container_round_trip():
    case = _flow_case()
    plain = npz_container("flow", case.stream, case.crc, len(case.raw))
    blob = npz_container("flow", case.stream, case.crc, len(case.raw), chunk_ends=case.ends)
    with np.load(io.BytesIO(blob)) as z:
        assert z.files == ["flow"]
        assert z["flow"].tobytes() == U.D.raw("flow_stack") and z["flow"].shape == (64, 96, 10)
    assert zipfile.ZipFile(io.BytesIO(blob)).testzip() is None
    assert npz_chunk_index(blob) == list(case.ends)
    assert npz_chunk_index(plain) is None
    assert npz_member(blob) == npz_member(plain)
    # everything in front of the central directory is the same; so is the end record's directory offset
    cd = plain.index(b"PK\x01\x02")
    assert blob[:cd] == plain[:cd]
    assert struct.unpack_from("<I", blob, len(blob) - 6) == struct.unpack_from("<I", plain, len(plain) - 6)
    # without chunk_ends: today's bytes (local header, stream, the 46-byte entry + name, the end record)
    fname = b"flow.npy"
    fields = (20, 0, 8, 0, 33, case.crc, len(case.stream), len(case.raw), len(fname), 0)
    local = struct.pack("<4sHHHHHIIIHH", b"PK\x03\x04", *fields) + fname
    central = struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\x01\x02", 20, *fields, 0, 0, 0, 0, 0) + fname
    end = struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, 1, 1, len(central), len(local) + len(case.stream), 0)
    assert plain == local + case.stream + central + end


def test_an_index_too_long_for_an_extra_field_is_left_out():
    ends = list(range(1, 20000))
    blob = npz_container("flow", b"\x03\x00", 0, 0, chunk_ends=ends)
    assert blob == npz_container("flow", b"\x03\x00", 0, 0)


def test_chunk_index_with_host_deflate_is_refused():
    import torch
    with pytest.raises(ValueError):
        save_npz_arrays(torch.zeros((1, 2, 2, 2), dtype=torch.uint8), deflate="host", chunk_index=True)


def _with_field(case, payload):
    """the container of `case` with `payload` as the whole 0x4354 field (header included)"""
    blob = npz_container("flow", case.stream, case.crc, len(case.raw), chunk_ends=case.ends)
    cd = blob.index(b"PK\x01\x02")
    entry_end = cd + 46 + 8
    old_extra, = struct.unpack_from("<H", blob, cd + 30)
    head = bytearray(blob[cd:entry_end])
    struct.pack_into("<H", head, 30, len(payload))
    central = bytes(head) + payload
    end = bytearray(blob[entry_end + old_extra:])
    struct.pack_into("<I", end, 12, len(central))
    return blob[:cd] + central + bytes(end)


def _field(version, chunk, n, ends, size=None):
    body = struct.pack("<HHII", version, 0, chunk, n) + np.asarray(ends, "<u4").tobytes()
    return struct.pack("<HH", 0x4354, len(body) if size is None else size) + body


def test_malformed_index_means_no_index():
    case = _flow_case()
    a, b = case.ends
    c = U.chunk()
    good = _with_field(case, _field(1, c, 2, [a, b]))
    assert npz_chunk_index(good) == [a, b]
    bad = {
        "version": _field(2, c, 2, [a, b]),
        "chunk size": _field(1, c // 2, 2, [a, b]),
        "count": _field(1, c, 3, [a, b - 1, b]),
        "non-monotone": _field(1, c, 2, [b, b]),
        "last end": _field(1, c, 2, [a, b - 1]),
        "cut short": _field(1, c, 2, [a, b])[:-3],
        "size field too long": _field(1, c, 2, [a, b], size=64),
    }
    for what, payload in bad.items():
        blob = _with_field(case, payload)
        assert npz_chunk_index(blob) is None, what
        if what != "cut short" and what != "size field too long":
            with np.load(io.BytesIO(blob)) as z:                 # still a file np.load reads
                assert z["flow"].shape == (64, 96, 10)
    assert npz_chunk_index(b"not a zip file") is None
    assert npz_chunk_index(good, name="other") is None


def _others_fine(t, r, odd):
    for i, case in enumerate(U.cases()):
        if i != odd:
            assert int(r.status[i]) == 0 and U.member_bytes(t, r, i) == case.raw, case.name
    U.check_guards(t, r)


@pytest.mark.parametrize("delta", [1, -1])
@pytest.mark.parametrize("name", ["smooth_three_chunks_5", "random_between_smooth", "zeros_three_chunks_5"])
def test_wrong_index_right_stream(name, delta):
    members = U.case_members()
    odd = [c.name for c in U.cases()].index(name)
    stream, size, crc, ends = members[odd]
    moved = list(ends)
    moved[1] += delta
    members[odd] = (stream, size, crc, tuple(moved))
    t = U.tables(members)
    r = U.run_host(t)
    assert int(r.status[odd]) != 0
    _others_fine(t, r, odd)


def test_invented_index_on_a_zlib_stream():
    raw = U.raws()["smooth_three_chunks_5"]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = co.compress(raw) + co.flush()
    n = U.n_chunks_of(len(raw))
    ends = tuple(len(stream) * (k + 1) // n for k in range(n))
    members = U.case_members()
    odd = 6
    members[odd] = (stream, len(raw), U.crc32(raw), ends)
    t = U.tables(members)
    r = U.run_host(t)
    assert int(r.status[odd]) != 0
    _others_fine(t, r, odd)


def test_inconsistent_chunk_rows_cost_status_12():
    """a chunk range that does not tile the member: one chunk too few, an out_off that leaves the member's slot"""
    members = U.case_members()
    t = U.tables(members)
    t.chunks[int(t.begin[6]) + 1].out_off += 1
    r = U.run_host(t)
    assert int(r.status[6]) == U.ROW
    _others_fine(t, r, 6)
    t = U.tables(members)
    t.begin[len(members)] -= 1                                  # the last member loses its last chunk
    r = U.run_host(t)
    assert int(r.status[len(members) - 1]) == U.ROW
    _others_fine(t, r, len(members) - 1)


def test_header_bytes_of_the_fixture_member():
    assert _flow_case().raw[:128] == npy_header((64, 96, 10))
