"""tbn_inflate_batch (csrc/inflate.hip) on every case of tests/golden/inflate_cases.npz: the bytes zlib gives, status 0, and
guard bytes behind every buffer that must stay untouched.  Byte results: equality, no tolerance."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests import inflate_util as U

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256
GUARD_VALUE = 0xCD
# single-byte changes, chosen on the CPU with scripts/inflate_check.cpp --pick (both passed its sanitizer run with
# exact-size buffers): (case, stream offset, new value)
REFUSED_CHANGE = ("flow_like", 9490, 12)          # "distance too far back" after 11 212 of 61 440 bytes
CRC_CHANGE = ("flow_like", 27669, 60)             # inflates to 61 440 bytes, other bytes: only the CRC notices


def _guarded(nbytes, dev):
    return torch.full((nbytes + GUARD_BYTES,), GUARD_VALUE, dtype=torch.uint8, device=dev)


def _device_inflate(members, out_gap=0):
    """tbn_inflate_batch on the current stream; input, table, output, status and info are followed by guard bytes
    -> (outputs as bytes per member, statuses, infos, the whole out array)"""
    from attention_based_tbn_amd import _lib
    packed, table, out_bytes = U.pack(members, out_gap)
    n = len(members)
    dev = torch.device("cuda")
    in_bytes = int(packed.size)
    inp = _guarded(in_bytes, dev)
    if in_bytes:
        inp[:in_bytes] = torch.from_numpy(packed).to(dev)
    table_bytes = C.sizeof(table)
    tab = _guarded(table_bytes, dev)
    tab[:table_bytes] = torch.from_numpy(np.frombuffer(table, np.uint8).copy()).to(dev)
    out, status, info = _guarded(out_bytes, dev), _guarded(4 * n, dev), _guarded(4 * n, dev)
    _lib.call("tbn_inflate_batch", _lib.ptr(inp), in_bytes, _lib.ptr(tab), n, _lib.ptr(out), out_bytes, _lib.ptr(status),
              _lib.ptr(info), _lib.stream_ptr())
    torch.cuda.current_stream().synchronize()
    for name, buf, used in (("out", out, out_bytes), ("status", status, 4 * n), ("info", info, 4 * n), ("in", inp, in_bytes),
                            ("table", tab, table_bytes)):
        assert bool((buf[used:] == GUARD_VALUE).all()), "write behind " + name
    host = out[:out_bytes].cpu().numpy()
    outs = [host[row.out_off:row.out_off + row.out_len].tobytes() for row in table]
    return (outs, status[:4 * n].cpu().numpy().view(np.int32).tolist(), info[:4 * n].cpu().numpy().view(np.int32).tolist(),
            host)


def _changed(name, change):
    assert change[0] == name
    b = bytearray(U.stream(name))
    assert b[change[1]] != change[2]
    b[change[1]] = change[2]
    return bytes(b)


@pytest.mark.parametrize("name", U.good_names())
def test_each_case_alone_equals_zlib(name):
    outs, status, info, _ = _device_inflate([U.member(name)])
    print(name, "status", status, "info", info)
    assert status == [U.OK] and info == [len(U.want(name))]
    assert outs[0] == U.want(name)


def test_all_cases_as_one_batch_with_a_stored_member_and_a_skipped_slot():
    names = U.good_names()
    raw = U.want("flow_like")
    members = [U.member(n) for n in names]
    members.insert(3, U.Member(raw, len(raw), zlib.crc32(raw), method=0))
    members.insert(5, U.member("rle", skip=True))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        outs, status, info, out = _device_inflate(members, out_gap=7)
    expect = [U.want(n) for n in names]
    expect.insert(3, raw)
    expect.insert(5, None)
    for i, e in enumerate(expect):
        if e is None:
            assert status[i] == U.SKIPPED and info[i] == 0 and outs[i] == bytes([GUARD_VALUE]) * len(outs[i])
        else:
            assert status[i] == U.OK and info[i] == len(e), (i, status[i], info[i])
            assert outs[i] == e, i
    at = 0
    for m in members:                                 # the gaps between the outputs are untouched
        at += m.size
        assert (out[at:at + 7] == GUARD_VALUE).all()
        at += 7
    # the host twin gives the same statuses, infos and bytes over the same table
    h_outs, h_status, h_info, _ = U.run_host(members, out_gap=7)
    assert h_status == status and h_info == info and all(a == b for a, b in zip(h_outs, outs) if a != b"\xcd" * len(a))


def test_a_stream_refused_mid_stream_and_one_only_the_crc_notices():
    good = U.member("flow_like")
    refused = U.Member(_changed("flow_like", REFUSED_CHANGE), good.size, good.crc)
    crc = U.Member(_changed("flow_like", CRC_CHANGE), good.size, good.crc)
    with pytest.raises(zlib.error, match="too far back"):
        zlib.decompress(refused.data, -15)
    other = zlib.decompress(crc.data, -15)
    assert len(other) == good.size and other != U.want("flow_like")
    members = [good, refused, U.member("rle"), crc, good]
    outs, status, info, out = _device_inflate(members, out_gap=9)
    assert status == [U.OK, U.DISTANCE, U.OK, U.CRC, U.OK]
    assert info == [good.size, 11212, 4000, good.size, good.size]
    assert outs[0] == outs[4] == U.want("flow_like") and outs[2] == U.want("rle")      # the neighbours are unaffected
    assert outs[3] == other                                                         # all there; the CRC is what differs
    at = 0
    for m in members:
        at += m.size
        assert (out[at:at + 9] == GUARD_VALUE).all()
        at += 9
    h_outs, h_status, h_info, _ = U.run_host(members, out_gap=9)
    assert h_status == status and h_info == info and h_outs[1][:11212] == outs[1][:11212]


def test_bad_arguments_are_refused_and_nothing_is_launched_for_no_members():
    from attention_based_tbn_amd import _lib
    dev = torch.device("cuda")
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.TbnHipError, match="null"):
        _lib.call("tbn_inflate_batch", 0, 16, _lib.ptr(buf), 1, _lib.ptr(buf), 16, _lib.ptr(buf), _lib.ptr(buf), 0)
    with pytest.raises(_lib.TbnHipError, match="aligned"):
        _lib.call("tbn_inflate_batch", _lib.ptr(buf) + 1, 16, _lib.ptr(buf), 1, _lib.ptr(buf), 16, _lib.ptr(buf), _lib.ptr(buf), 0)
    with pytest.raises(_lib.TbnHipError, match="negative"):
        _lib.call("tbn_inflate_batch", _lib.ptr(buf), 16, _lib.ptr(buf), -1, _lib.ptr(buf), 16, _lib.ptr(buf), _lib.ptr(buf), 0)
    _lib.call("tbn_inflate_batch", 0, 0, 0, 0, 0, 0, 0, 0, 0)


def test_load_npz_arrays_mixes_device_and_host_members():
    import io

    from attention_based_tbn_amd.core.dataset import npz_file as N
    rng = np.random.RandomState(5)
    arrays = [(np.add.outer(np.arange(40) * 5, np.arange(56 * 4)).reshape(40, 56, 4) + rng.randint(0, 3, (40, 56, 4))).astype(np.uint8)
              for _ in range(4)]
    blobs = []
    for i, a in enumerate(arrays):
        buf = io.BytesIO()
        if i == 2:
            np.savez_compressed(buf, flow=np.asfortranarray(a))       # the record sends it to the host
        else:
            (np.savez if i == 1 else np.savez_compressed)(buf, flow=a)
        blobs.append(buf.getvalue())
    before = N.fallback_count()
    got, statuses = N.load_npz_arrays(blobs)
    assert statuses == [0, 0, U.SKIPPED, 0] and N.fallback_count() == before + 1
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (4, 40, 56, 4)
    assert np.array_equal(got.cpu().numpy(), np.stack(arrays))
    planes, _ = N.load_npz_arrays(blobs, planes=True)
    assert tuple(planes.shape) == (16, 40, 56, 1)
    assert np.array_equal(planes.cpu().numpy()[:, :, :, 0], np.stack(arrays).transpose(0, 3, 1, 2).reshape(16, 40, 56))
