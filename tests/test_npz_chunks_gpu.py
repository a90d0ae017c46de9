"""Chunk-indexed flow pickles on the device: `tbn_inflate_chunks` (one wavefront per chunk) against its host twin over the
member set of tests/npz_chunks_util.py, the index `tbn_deflate_batch_indexed` writes, and the files through
`save_npz_arrays(chunk_index=True)` / `load_npz_arrays` / `Video_Dataset(flow_load="device")`.  Bytes: equality, no tolerance."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest
import torch

from tests import npz_chunks_util as U

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_device(t):
    """tbn_inflate_chunks over the tables -> U.Result (host arrays)"""
    from attention_based_tbn_amd._lib import call, ptr, stream_ptr
    n = len(t.members)
    f = U.fresh(t)
    packed, out = _dev(t.packed), _dev(f.out)
    members = _dev(np.frombuffer(t.members, np.uint8))
    chunks = _dev(np.frombuffer(t.chunks, np.uint8))
    begin, status, info, cs = _dev(t.begin), _dev(f.status), _dev(f.info), _dev(f.chunk_status)
    call("tbn_inflate_chunks", ptr(packed), packed.numel(), ptr(members), n, ptr(chunks), ptr(begin), t.n_chunks, ptr(out),
         out.numel(), ptr(status), ptr(info), ptr(cs), stream_ptr())
    torch.cuda.synchronize()
    return U.Result(out.cpu().numpy(), status.cpu().numpy(), info.cpu().numpy(), cs.cpu().numpy())


def _same(got, want):
    assert got.status.tolist() == want.status.tolist()
    assert got.info.tolist() == want.info.tolist()
    assert got.chunk_status.tolist() == want.chunk_status.tolist()
    assert np.array_equal(got.out, want.out)


def test_device_equals_host_twin():
    t, want = U.host_result()
    assert want.status.tolist() == [0] * len(U.cases())
    got = _run_device(t)
    _same(got, want)
    for i, case in enumerate(U.cases()):
        assert U.member_bytes(t, got, i) == case.raw, case.name
    U.check_guards(t, got)


def test_device_equals_host_twin_with_a_skipped_member():
    t = U.tables(U.case_members(), skip={6})
    want = U.run_host(t)
    got = _run_device(t)
    assert int(got.status[6]) == U.SKIPPED and int(got.info[6]) == 0
    row = t.members[6]
    assert (got.out[row.out_off:row.out_off + row.out_len] == U.GUARD).all()
    _same(got, want)
    U.check_guards(t, got)


@pytest.mark.parametrize("delta", [1, -1])
def test_device_equals_host_twin_with_a_moved_end(delta):
    """statuses and bytes produced are the host twin's for a wrong index too; what a refused chunk leaves behind the bytes
    it produced is unspecified on both sides, so the good members and the guards are compared, not the whole buffer"""
    members = U.case_members()
    odd = [c.name for c in U.cases()].index("random_between_smooth")
    stream, size, crc, ends = members[odd]
    members[odd] = (stream, size, crc, (ends[0], ends[1] + delta) + tuple(ends[2:]))
    t = U.tables(members)
    want, got = U.run_host(t), _run_device(t)
    assert int(got.status[odd]) != 0
    assert got.status.tolist() == want.status.tolist() and got.info.tolist() == want.info.tolist()
    assert got.chunk_status.tolist() == want.chunk_status.tolist()
    for i, case in enumerate(U.cases()):
        if i != odd:
            assert U.member_bytes(t, got, i) == case.raw, case.name
    U.check_guards(t, got)


def _stacks(n):
    rng = np.random.RandomState(5)
    base = np.frombuffer(U.D.raw("flow_stack"), np.uint8).reshape(64, 96, 10)
    return np.stack([np.roll(base, (3 * i, 5 * i), (0, 1)) if i % 3 else rng.randint(0, 256, base.shape).astype(np.uint8)
                     for i in range(n)])


def test_indexed_write_from_the_device():
    from attention_based_tbn_amd._lib import DeflateMember, call, lib, ptr, stream_ptr
    from attention_based_tbn_amd.core.dataset.npz_file import npy_header, npz_chunk_index, npz_member, save_npz_arrays
    stacks = _stacks(4)
    arrays = torch.from_numpy(stacks).cuda()
    plain = save_npz_arrays(arrays)
    indexed = save_npz_arrays(arrays, chunk_index=True)
    raws = [npy_header((64, 96, 10)) + s.tobytes() for s in stacks]
    _, _, statuses, host_ends = U.deflate_host(raws, True)
    assert not any(statuses)
    for a, b, stack, ends in zip(plain, indexed, stacks, host_ends):
        ra, rb = npz_member(a), npz_member(b)
        assert ra == rb
        assert a[:ra.data_offset + ra.data_length] == b[:rb.data_offset + rb.data_length]      # local header and stream
        assert npz_chunk_index(a) is None and npz_chunk_index(b) == ends and len(ends) == 2
        with np.load(io.BytesIO(b)) as z:
            assert z.files == ["flow"] and np.array_equal(z["flow"], stack)
    # the entry point itself: the ends of the host twin, zeros for a skipped row
    n = 3
    size = len(raws[0])
    stride, cap = -(-size // 16) * 16, -(-U.D.bound(size) // 16) * 16
    table = (DeflateMember * n)()
    for i in range(n):
        table[i].in_off, table[i].in_len, table[i].out_off, table[i].out_cap, table[i].skip = i * stride, size, i * cap, cap, int(i == 1)
    raw = np.zeros(n * stride, np.uint8)
    for i in range(n):
        raw[i * stride:i * stride + size] = np.frombuffer(raws[i], np.uint8)
    raw_d, table_d = _dev(raw), _dev(np.frombuffer(table, np.uint8))
    out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    meta = torch.full((3 * n + 2 * n,), -1, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib().tbn_deflate_workspace_bytes(C.addressof(table), n)), dtype=torch.uint8, device="cuda")
    call("tbn_deflate_batch_indexed", ptr(raw_d), raw.size, ptr(table_d), n, ptr(out), n * cap, ptr(meta), ptr(meta) + 4 * n,
         ptr(meta) + 8 * n, ptr(work), stream_ptr(), ptr(meta) + 12 * n)
    host = meta.cpu().numpy()
    assert host[2 * n:3 * n].tolist() == [0, 3, 0]
    assert host[3 * n:].tolist() == host_ends[0] + [0, 0] + host_ends[2]
    assert host[:n].tolist() == [host_ends[0][-1], 0, host_ends[2][-1]]


def _shift_index(blob, k, delta):
    """the file with end k of its chunk index moved by delta"""
    at = blob.rindex(struct.pack("<HH", 0x4354, 12 + 4 * 2)) + 16 + 4 * k
    end, = struct.unpack_from("<I", blob, at)
    return blob[:at] + struct.pack("<I", end + delta) + blob[at + 4:]


def test_mixed_batch_through_load_npz_arrays():
    from attention_based_tbn_amd.core.dataset import npz_file as F
    stacks = _stacks(5)
    arrays = torch.from_numpy(stacks).cuda()
    indexed = F.save_npz_arrays(arrays[[0, 4]], chunk_index=True)
    unindexed = F.save_npz_arrays(arrays[1:2])
    blobs = [indexed[0], unindexed[0]]
    for save in (np.savez_compressed, np.savez):
        buf = io.BytesIO()
        save(buf, flow=stacks[len(blobs)])
        blobs.append(buf.getvalue())
    blobs.append(_shift_index(indexed[1], 0, 1))
    assert F.npz_chunk_index(blobs[4]) is not None and F.npz_chunk_index(blobs[0]) is not None
    assert [F.npz_chunk_index(b) for b in blobs[1:4]] == [None] * 3
    for i, b in enumerate(blobs):
        with np.load(io.BytesIO(b)) as z:
            assert np.array_equal(z["flow"], stacks[i])
    before = (F.fallback_count(), F.chunked_count(), F.member_count())
    got, statuses = F.load_npz_arrays(blobs)
    assert torch.equal(got.cpu(), torch.from_numpy(stacks))
    assert [s != 0 for s in statuses] == [False, False, False, False, True]
    assert (F.fallback_count(), F.chunked_count(), F.member_count()) == (before[0] + 1, before[1] + 1, before[2] + 5)
    whole, statuses = F.load_npz_arrays(blobs, chunked=False)
    assert torch.equal(whole, got) and statuses == [0] * 5
    assert F.chunked_count() == before[1] + 1
    planes, _ = F.load_npz_arrays(blobs[:1] * 2, planes=True)          # every member indexed: the chunk reader alone
    assert torch.equal(planes.cpu(), torch.from_numpy(np.concatenate([stacks[0].transpose(2, 0, 1)[..., None]] * 2)))
    with pytest.raises(ValueError):
        F.load_npz_arrays(blobs, chunked=True)


def test_dataset_over_indexed_pickles(tmp_path):
    from tests import clip_loader_util as L
    from tests.test_flow_pickle_gpu import _cfg, _stack
    from attention_based_tbn_amd.core.dataset import npz_file as F
    cfg = _cfg(tmp_path)
    paths, flows = [], []
    for vid in L.VIDS:
        for i in range(L.N_FILES - 1):
            paths.append(os.path.join(str(tmp_path), "flow", vid, "frame_{:010d}.npz".format(i)))
            flows.append(_stack(vid, i))
    F.write_npz_files(paths, torch.from_numpy(np.stack(flows)).cuda(), chunk_index=True)
    with open(paths[0], "rb") as f:
        assert F.npz_chunk_index(f.read()) is not None
    host = L.make_dataset(cfg, ["Flow"], "train", flow_load="host")
    dev = L.make_dataset(cfg, ["Flow"], "train", flow_load="device")
    before = F.chunked_count()
    for seed in (13, 14):
        np.random.seed(seed)
        want = host.batch([0, 1, 2])[0]
        np.random.seed(seed)
        got = dev.batch([0, 1, 2])[0]
        assert tuple(got["Flow"].shape) == (3, 2, 4, 16, 16)
        assert torch.equal(got["Flow"], want["Flow"]) and torch.equal(got["indices"]["Flow"], want["indices"]["Flow"])
    assert dev.flow_fallbacks == 0 and F.chunked_count() == before + 2 * 3 * 2
