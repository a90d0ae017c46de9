"""`Video_Dataset(..., flow_load="device")`: the flow pickles of a batch inflated by one `load_npz_arrays` call, against
`flow_load="host"` (np.load per pickle) under the same seed, on the synthetic dataset of tests/clip_loader_util.py.
uint8 pixels through one float table: `torch.equal`, no tolerance."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import clip_loader_util as U
from tests import jpeg_ref as R

pytestmark = pytest.mark.gpu

# a single-byte change in the fixture's `pickle_40x56x4` stream (a whole flow pickle member: header and a (40, 56, 4) array),
# chosen on the CPU with scripts/inflate_check.cpp --pick after its sanitizer run passed: (case, stream offset, new value)
PICKLE_CHANGE = ("pickle_40x56x4", 1752, 218)      # "distance too far back" after 2 040 of 9 088 bytes


def _zip_around(stream, size, crc, name=b"flow.npy"):
    """a one-member .npz around a ready-made deflate stream"""
    local = struct.pack("<4sHHHHHIIIHH", b"PK\x03\x04", 20, 0, 8, 0, 0x21, crc, len(stream), size, len(name), 0) + name
    central = struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\x01\x02", 20, 20, 0, 8, 0, 0x21, crc, len(stream), size, len(name),
                          0, 0, 0, 0, 0, 0) + name
    end = struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, 1, 1, len(central), len(local) + len(stream), 0)
    return local + stream + central + end


def _cfg(tmp_path, extra=(), **kw):
    from attention_based_tbn_amd.config import load_config
    return load_config(U.write_dataset(tmp_path, **kw) + ["data.sampling=async", "model.attention.enable=False",
                                                           "data.flow.read_flow_pickle=True"] + list(extra))


def _stack(vid, i, names=None):
    return np.concatenate([R.golden(U.flow_name(vid, axis, i + k, names), "gray") for k in range(2) for axis in ("x", "y")], 2)


def _write_pickles(root, save, small_vid=None):
    for vid in U.VIDS:
        names = U.names_35x50() if vid == small_vid else None
        for i in range(U.N_FILES - 1):
            flow = _stack(vid, i, names)
            assert flow.shape == ((35, 50, 4) if names else (40, 56, 4)) and flow.dtype == np.uint8
            save(os.path.join(str(root), "flow", vid, "frame_{:010d}.npz".format(i)), flow=flow)


def _pickle(root, vid, i):
    return os.path.join(str(root), "flow", vid, "frame_{:010d}.npz".format(i))


@pytest.mark.parametrize("save", [np.savez, np.savez_compressed], ids=["stored", "deflated"])
@pytest.mark.parametrize("small_vid", [None, "P01_02"], ids=["one_size", "two_sizes"])
def test_device_batches_equal_host_batches(tmp_path, save, small_vid):
    cfg = _cfg(tmp_path, small_vid=small_vid)
    _write_pickles(tmp_path, save, small_vid)
    host = U.make_dataset(cfg, ["Flow"], "train", flow_load="host")
    dev = U.make_dataset(cfg, ["Flow"], "train", flow_load="device")
    for seed in (13, 14):
        np.random.seed(seed)
        want = host.batch([0, 1, 2])[0]
        np.random.seed(seed)
        got = dev.batch([0, 1, 2])[0]
        assert tuple(got["Flow"].shape) == (3, 2, 4, 16, 16)
        assert torch.equal(got["Flow"], want["Flow"]) and torch.equal(got["indices"]["Flow"], want["indices"]["Flow"])
    assert dev.flow_fallbacks == 0 and host.flow_fallbacks == 0      # nothing hid behind the host path
    np.random.seed(3)
    want_item = host[1][0]["Flow"]
    np.random.seed(3)
    item = dev[1][0]["Flow"]
    assert torch.equal(item, want_item) and dev.flow_fallbacks == 0


def test_prefetching_loader_equals_the_synchronous_one(tmp_path):
    from attention_based_tbn_amd.core.utils import ClipLoader
    cfg = _cfg(tmp_path)
    _write_pickles(tmp_path, np.savez_compressed)
    dev = U.make_dataset(cfg, ["Flow"], "train", flow_load="device")
    host = U.make_dataset(cfg, ["Flow"], "train", flow_load="host")
    runs = []
    for ds, kw in ((dev, dict(prefetch=2)), (dev, dict(prefetch=0, rng="private")), (host, dict(prefetch=0, rng="private"))):
        torch.manual_seed(4)
        loader = ClipLoader(ds, 2, shuffle=True, **kw)
        runs.append([b[0]["Flow"].clone() for b in loader])
        loader.close()
    assert len(runs[0]) == 2 and [tuple(b.shape) for b in runs[0]] == [(2, 2, 4, 16, 16), (1, 2, 4, 16, 16)]
    for a, b, c in zip(*runs):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert dev.flow_fallbacks == 0


def test_create_dataloader_forwards_flow_load(tmp_path):
    import logging

    from attention_based_tbn_amd.core.utils import create_dataloader
    cfg = _cfg(tmp_path)
    _write_pickles(tmp_path, np.savez_compressed)
    loader = create_dataloader(cfg, logging.getLogger("test"), ["Flow"], mode="val", flow_load="device")
    assert loader.dataset.flow_load == "device"
    data = next(iter(loader))[0]
    assert tuple(data["Flow"].shape) == (2, 2, 4, 16, 16) and loader.dataset.flow_fallbacks == 0
    assert create_dataloader(cfg, logging.getLogger("test"), ["Flow"], mode="val").dataset.flow_load == "host"
    with pytest.raises(ValueError, match="flow_load"):
        U.make_dataset(cfg, ["Flow"], "train", flow_load="gpu")


def _batches_until(ds, what):
    with pytest.raises(Exception, match=what) as e:
        for seed in range(8):                                         # some draw reads index 3 of the second video
            np.random.seed(seed)
            ds.batch([1])
    return str(e.value)


def test_members_for_the_host_path_raise_the_host_paths_message(tmp_path):
    cfg = _cfg(tmp_path)
    _write_pickles(tmp_path, np.savez_compressed)
    flow = _stack("P01_02", 3)
    np.savez_compressed(_pickle(tmp_path, "P01_02", 3), flow=flow.astype(np.uint16))
    messages = []
    for mode in ("host", "device"):
        messages.append(_batches_until(U.make_dataset(cfg, ["Flow"], "train", flow_load=mode), "frame_0000000003.npz"))
    assert messages[0] == messages[1] and "uint16" in messages[0]
    # Fortran order: np.load reads it, so do both modes, the device mode through the host path -- and it counts it
    np.savez_compressed(_pickle(tmp_path, "P01_02", 3), flow=np.asfortranarray(flow))
    host = U.make_dataset(cfg, ["Flow"], "train", flow_load="host")
    dev = U.make_dataset(cfg, ["Flow"], "train", flow_load="device")
    seen = 0
    for seed in range(8):
        np.random.seed(seed)
        want = host.batch([1, 0])[0]
        np.random.seed(seed)
        got = dev.batch([1, 0])[0]
        assert torch.equal(got["Flow"], want["Flow"])
        seen += int((want["indices"]["Flow"][0] == 3).sum())
    assert seen > 0 and dev.flow_fallbacks == seen


def test_a_deleted_file_and_a_damaged_one_raise_the_load_message(tmp_path):
    from tests import inflate_util as I
    cfg = _cfg(tmp_path)
    _write_pickles(tmp_path, np.savez_compressed)
    path = _pickle(tmp_path, "P01_02", 3)
    name, offset, value = PICKLE_CHANGE
    member = I.want(name)
    good = _zip_around(I.stream(name), len(member), zlib.crc32(member))
    assert np.load(io.BytesIO(good))["flow"].shape == (40, 56, 4)       # the wrapper is a pickle np.load reads
    stream = bytearray(I.stream(name))
    assert stream[offset] != value
    stream[offset] = value
    with open(path, "wb") as f:
        f.write(_zip_around(bytes(stream), len(member), zlib.crc32(member)))
    with pytest.raises(Exception):
        np.load(path)["flow"]
    dev = U.make_dataset(cfg, ["Flow"], "train", flow_load="device")
    message = _batches_until(dev, "Failed to load flow file .*frame_0000000003.npz")
    assert path in message
    os.remove(path)
    message = _batches_until(U.make_dataset(cfg, ["Flow"], "train", flow_load="device"),
                             "Failed to load flow file .*frame_0000000003.npz")
    assert path in message
