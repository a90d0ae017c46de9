"""tbn_deflate_batch (csrc/deflate.hip) against its host twin on every case of tests/golden/deflate_cases.npz: the same
bytes, lengths, CRCs and statuses, guard bytes untouched; and save_npz_arrays read back by np.load and load_npz_arrays.
Byte results: equality, no tolerance."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests import deflate_util as U

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256


def _guarded(nbytes, dev):
    return torch.full((nbytes + GUARD_BYTES,), U.GUARD, dtype=torch.uint8, device=dev)


def _device_deflate():
    """tbn_deflate_batch over U.batch() on the current stream; every buffer is followed by guard bytes -> U.Result"""
    from attention_based_tbn_amd import _lib
    b = U.batch()
    n = len(b.rows)
    dev = torch.device("cuda")
    raw = _guarded(b.raw.size, dev)
    raw[:b.raw.size] = torch.from_numpy(b.raw).to(dev)
    table_bytes = C.sizeof(b.table)
    tab = _guarded(table_bytes, dev)
    tab[:table_bytes] = torch.from_numpy(np.frombuffer(b.table, np.uint8).copy()).to(dev)
    ws_bytes = int(U.lib().tbn_deflate_workspace_bytes(C.addressof(b.table), n))
    out, ws = _guarded(b.out_bytes, dev), _guarded(ws_bytes, dev)
    out_len, crc, status = _guarded(4 * n, dev), _guarded(4 * n, dev), _guarded(4 * n, dev)
    _lib.call("tbn_deflate_batch", raw.data_ptr(), b.raw.size, tab.data_ptr(), n, out.data_ptr(), b.out_bytes, out_len.data_ptr(),
              crc.data_ptr(), status.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    for buf, used in ((raw, b.raw.size), (tab, table_bytes), (out, b.out_bytes), (ws, ws_bytes), (out_len, 4 * n), (crc, 4 * n),
                      (status, 4 * n)):
        assert bool((buf[used:] == U.GUARD).all()), "guard bytes behind a buffer were written"
    assert torch.equal(raw[:b.raw.size].cpu(), torch.from_numpy(b.raw))
    return U.Result(out[:b.out_bytes].cpu().numpy(), out_len[:4 * n].cpu().numpy().view(np.uint32),
                    crc[:4 * n].cpu().numpy().view(np.uint32), status[:4 * n].cpu().numpy().view(np.int32))


def test_one_batch_over_all_cases_equals_the_host_twin_byte_for_byte():
    host, dev = U.host_result(), _device_deflate()
    assert dev.status.tolist() == host.status.tolist()
    assert dev.out_len.tolist() == host.out_len.tolist()
    assert dev.crc.tolist() == host.crc.tolist()
    U.check_layout(dev)                              # guard gaps, the skipped and the short row
    assert np.array_equal(dev.out, host.out)         # the streams, and every byte between them


def test_the_same_call_twice_gives_identical_bytes():
    a, b = _device_deflate(), _device_deflate()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _stacks():
    g = torch.Generator().manual_seed(5)
    smooth = (128 + 20 * torch.sin(torch.arange(40 * 56 * 10) / 97.0)).to(torch.uint8).view(1, 40, 56, 10)
    stacks = torch.cat([smooth + torch.randint(0, 3, (3, 40, 56, 10), generator=g, dtype=torch.uint8),
                        torch.zeros(1, 40, 56, 10, dtype=torch.uint8),
                        torch.randint(0, 256, (1, 40, 56, 10), generator=g, dtype=torch.uint8)])
    return stacks.cuda()


@pytest.mark.parametrize("deflate", ["device", "host"])
def test_save_npz_arrays_is_read_back_by_np_load_and_by_load_npz_arrays(deflate):
    from attention_based_tbn_amd.core.dataset.npz_file import load_npz_arrays, npz_member, save_npz_arrays
    stacks = _stacks()
    blobs = save_npz_arrays(stacks, deflate=deflate)
    assert len(blobs) == 5 and all(isinstance(b, bytes) for b in blobs)
    want = stacks.cpu().numpy()
    for b, w in zip(blobs, want):
        with np.load(io.BytesIO(b)) as z:
            assert z.files == ["flow"] and z["flow"].dtype == np.uint8 and np.array_equal(z["flow"], w)
        assert npz_member(b).host is False
    back, statuses = load_npz_arrays(blobs)
    assert statuses == [0] * 5 and torch.equal(back, stacks)


def test_write_npz_files_leaves_only_the_named_files(tmp_path):
    from attention_based_tbn_amd.core.dataset.npz_file import write_npz_files
    stacks = _stacks()[:2]
    paths = [str(tmp_path / f"frame_{i:010d}.npz") for i in range(2)]
    sizes = write_npz_files(paths, stacks)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["frame_0000000000.npz", "frame_0000000001.npz"]
    for p, s, w in zip(paths, sizes, stacks.cpu().numpy()):
        assert (tmp_path / p).stat().st_size == s
        with np.load(p) as z:
            assert np.array_equal(z["flow"], w)
