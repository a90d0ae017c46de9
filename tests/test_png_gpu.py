"""PNG frames on the device: `decode_pngs` (host and device inflate) against the written pixels over the case set of
tests/png_util.py, the device kernels against their host twins, damaged images beside good ones, `decode_frames`, and
file_ext "png" through `FrameReader`, `Video_Dataset` and the flow pickle tool.  PNG is lossless: exact equality everywhere."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import clip_loader_util as CU
from tests import png_util as U

pytestmark = pytest.mark.gpu

# single-byte changes of a case's ZLIB STREAM, chosen on the CPU with scripts/png_check.cpp --pick after its sanitizer run
# passed (ASan + UBSan, every case, every truncation, seeded corruptions): (case, offset in the zlib stream, new value,
# the status tbn_png_decode_host gives)
DAMAGED = [
    ("ct0_64x64_f4_white_l6_n3", 38, 60, 8),
    ("ct0_64x64_f4_white_l6_n3", 27, 152, 20),
    ("ct2_65x67_f43210_random_l6_n1", 3, 154, 2),
    ("ct2_65x67_f43210_random_l6_n1", 12489, 60, 20),
    ("ct3_65x67_f3_levels_l9_n1", 11, 60, 6),
    ("ct3_65x67_f3_levels_l9_n1", 635, 11, 20),
]


@pytest.fixture(scope="module")
def cases():
    return U.case_set(U.limits())


@pytest.fixture(scope="module")
def by_name(cases):
    return {c.name: c for c in cases}        # a name that comes up twice: the later case, as the dump for png_check has it


def _fallbacks():
    from attention_based_tbn_amd.core.dataset.frames import png_fallback_count
    return png_fallback_count()


@pytest.mark.parametrize("inflate", ["host", "device"])
@pytest.mark.parametrize("ct", U.COLOUR_TYPES)
def test_decode_pngs_equals_the_written_pixels(cases, ct, inflate):
    from attention_based_tbn_amd.core.dataset.frames import decode_pngs
    before = _fallbacks()
    for k, c in enumerate(c for c in cases if c.colour_type == ct):
        threads = (1, 64)[k % 2]
        got = decode_pngs(c.blobs, inflate=inflate, threads=threads)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(c.blobs),) + c.size + (3,)
        assert np.array_equal(got.cpu().numpy(), c.frames()), c.name
        if ct in (0, 4):
            got = decode_pngs(c.blobs, gray=True, inflate=inflate, threads=threads)
            assert np.array_equal(got.cpu().numpy(), c.frames(gray=True)), c.name
    assert _fallbacks() == before             # tbn_png_decode took every image: no host stage


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_one_batch_of_frame_size(inflate):
    from attention_based_tbn_amd.core.dataset.frames import decode_pngs
    before = _fallbacks()
    for c in U.frame_batch(4):
        assert np.array_equal(decode_pngs(c.blobs, inflate=inflate).cpu().numpy(), c.frames()), c.name
        if c.colour_type == 0:
            assert np.array_equal(decode_pngs(c.blobs, gray=True, inflate=inflate).cpu().numpy(), c.frames(gray=True))
    assert _fallbacks() == before


def _decode_dev(blobs, gray=False, damage=None, table_edit=None):
    """tbn_png_decode over what tests/png_util.pack gathers -> (frames, statuses, info), as U.decode_host returns them"""
    from attention_based_tbn_amd._lib import PngImage, call, lib, ptr, stream_ptr
    geo, packed, table, in_bytes = U.pack(blobs, damage)
    if table_edit is not None:
        table_edit(table)
    n, ch = len(blobs), 1 if gray else 3
    rows = np.frombuffer(bytes(table), np.uint8)
    dev = torch.from_numpy(np.concatenate([packed, np.zeros(-len(packed) % 8, np.uint8), rows])).cuda()
    table_at = len(packed) + (-len(packed) % 8)
    frames = torch.zeros((n, geo.height, geo.width, ch), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(int(lib().tbn_png_workspace_bytes(C.byref(geo), n)), dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    info = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    assert C.sizeof(PngImage) == 24
    call("tbn_png_decode", ptr(dev), in_bytes, ptr(dev) + table_at, n, C.byref(geo), ch, ptr(frames), ptr(ws), ptr(status),
         ptr(info), stream_ptr())
    return frames.cpu().numpy(), status.tolist(), info.tolist()


def test_device_and_host_twins_agree_on_pixels_and_on_the_new_statuses():
    c = U.make_case(11, 0, (6, 9), (1,), "random", U.STREAMS[0], 3)
    raw = bytearray(U.filter_rows(c.pixels[2], (1,)))
    raw[2 * 10] = 5
    idx = np.array([[0, 1, 2], [2, 1, 3]], np.uint8)[:, :, None]
    pal = np.arange(9, dtype=np.uint8).reshape(3, 3)
    runs = [
        (c.blobs, dict(table_edit=lambda t: setattr(t[1], "adler", t[1].adler ^ 0x100)), [0, 20, 0]),
        ([c.blobs[0], c.blobs[1], U.png(c.pixels[2], 0, raw=bytes(raw), level=0)], {}, [0, 0, 21]),
        ([U.png(idx, 3, palette=pal), U.png(np.minimum(idx, 2), 3, palette=pal)], {}, [22, 0]),
        (c.blobs, dict(table_edit=lambda t: setattr(t[0], "in_len", t[0].in_len - 9)), [7, 0, 0]),
        (c.blobs, dict(table_edit=lambda t: setattr(t[2], "in_off", t[2].in_off + 1)), [0, 0, 12]),
    ]
    for blobs, kw, want in runs:
        hf, hs, hi = U.decode_host(blobs, **kw)
        df, ds, di = _decode_dev(blobs, **kw)
        assert hs == want and ds == want and di == hi
        good = [i for i, s in enumerate(want) if s in (0, 21, 22)]      # a status of the unfilter stage: the same bytes still
        assert np.array_equal(df[good], hf[good])
    for ct in U.COLOUR_TYPES:
        c = U.make_case(21 + ct, ct, (67, 70), (4, 3, 2, 1, 0), "random", U.STREAMS[1], 2)
        hf, hs, hi = U.decode_host(c.blobs)
        df, ds, di = _decode_dev(c.blobs)
        assert hs == ds == [0, 0] and hi == di and np.array_equal(hf, df) and np.array_equal(df, c.frames())


def test_unfilter_alone_equals_its_host_twin_on_garbage_scanlines():
    """random bytes as scanlines, filter bytes above 4 and indices past the palette among them: a status and the twin's
    bytes, at every colour type"""
    from attention_based_tbn_amd._lib import PngGeometry, call, lib, ptr, stream_ptr
    rng = np.random.RandomState(5)
    for ct in U.COLOUR_TYPES:
        h, w, n = 70, 69, 3
        bpp = U.BPP[ct]
        g = PngGeometry(w, h, ct, bpp, 0, 0, h * (1 + w * bpp), 0)
        raw = rng.randint(0, 256, (n, h, 1 + w * bpp)).astype(np.uint8)
        raw[:, :, 0] = rng.randint(0, 5, (n, h))
        raw[1, 66, 0] = 9
        pal = np.zeros((n, 1024), np.uint8)
        pal[:, :768] = rng.randint(0, 256, (n, 768))
        pal[:, 768] = 200
        pal[:, 600:768] = 0
        want = np.zeros((n, h, w, 3), np.uint8)
        status = (C.c_int * n)()
        assert lib().tbn_png_unfilter_host(raw.ctypes.data, pal.ctypes.data, n, C.byref(g), 3, want.ctypes.data, C.addressof(status)) == 0
        assert list(status) == ([22, 21, 22] if ct == 3 else [0, 21, 0])
        d_raw, d_pal = torch.from_numpy(raw).cuda(), torch.from_numpy(pal).cuda()
        got = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
        d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        call("tbn_png_unfilter", ptr(d_raw), ptr(d_pal), n, C.byref(g), 3, ptr(got), ptr(d_status), stream_ptr())
        assert d_status.tolist() == list(status) and np.array_equal(got.cpu().numpy(), want), ct


def _damaged_blob(c, offset, value):
    zs = bytearray(U.deflate(U.filter_rows(c.pixels[0], c.schedule), c.stream[0], c.stream[1]))
    assert zs[offset] != value
    zs[offset] = value
    return U.png(c.pixels[0], c.colour_type, palette=c.palettes[0], zstream=bytes(zs), idat_splits=U.SPLITS)


@pytest.mark.parametrize("name, offset, value, status", DAMAGED)
def test_a_damaged_image_beside_good_ones(by_name, name, offset, value, status):
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset.frames import decode_pngs
    c = by_name[name]
    other = U.make_case(99, c.colour_type, c.size, c.schedule, c.kind, c.stream, 2)
    bad = _damaged_blob(c, offset, value)
    blobs = [other.blobs[0], bad, other.blobs[1]]
    assert U.decode_host(blobs)[1] == [0, status, 0]
    assert _decode_dev(blobs)[1] == [0, status, 0]
    before = _fallbacks()
    with pytest.raises(TbnHipError, match=r"decode_pngs: image 1: png: ") as e:
        decode_pngs(blobs, inflate="device")
    assert "image 0" not in str(e.value) and "image 2" not in str(e.value)
    assert _fallbacks() == before + 1                         # the device stage sent it to the host stage, which refused it
    with pytest.raises(TbnHipError, match=r"decode_pngs: image 1: png: "):
        decode_pngs(blobs, inflate="host")
    good = decode_pngs([blobs[0], blobs[2]], inflate="device")
    assert np.array_equal(good.cpu().numpy(), other.frames()) and _fallbacks() == before + 1


def test_a_filter_byte_above_4_is_refused_by_both_modes_and_names_the_image():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset.frames import decode_pngs
    c = U.make_case(31, 2, (9, 6), (2,), "random", U.STREAMS[1], 2)
    raw = bytearray(U.filter_rows(c.pixels[1], (2,)))
    raw[4 * 19] = 7
    blobs = [c.blobs[0], U.png(c.pixels[1], 2, raw=bytes(raw))]
    for inflate in ("host", "device"):
        with pytest.raises(TbnHipError, match=r"image 1: png: scanline 4 has filter type 7"):
            decode_pngs(blobs, inflate=inflate)
    idx = np.array([[0, 1, 2], [2, 1, 3]], np.uint8)[:, :, None]
    pal = np.arange(9, dtype=np.uint8).reshape(3, 3)
    for inflate in ("host", "device"):
        with pytest.raises(TbnHipError, match=r"image 0: png: a palette index at or beyond the PLTE entry count"):
            decode_pngs([U.png(idx, 3, palette=pal), U.png(np.minimum(idx, 2), 3, palette=pal)], inflate=inflate)


def test_refusals_in_decode_jpegs_wording():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset.frames import decode_pngs
    a = U.make_case(1, 2, (4, 5), (0,), "random", U.STREAMS[1])
    b = U.make_case(2, 2, (4, 6), (0,), "random", U.STREAMS[1])
    g = U.make_case(3, 0, (4, 5), (0,), "random", U.STREAMS[1])
    with pytest.raises(TbnHipError, match=r"mixed geometries in one batch: image 0 is 5x4 \(colour type 2\), image 1 is 6x4"):
        decode_pngs(a.blobs + b.blobs)
    with pytest.raises(TbnHipError, match=r"mixed geometries in one batch: image 0 is 5x4 \(colour type 2\), image 1 is 5x4 \(colour type 0\)"):
        decode_pngs(a.blobs + g.blobs)
    with pytest.raises(ValueError, match="inflate='gpu' is not 'host' or 'device'"):
        decode_pngs(a.blobs, inflate="gpu")
    with pytest.raises(TbnHipError, match="expected a non-empty list"):
        decode_pngs([])
    for ct in (2, 3, 6):
        c = U.make_case(4, ct, (4, 5), (0,), "random", U.STREAMS[1])
        with pytest.raises(TbnHipError, match=f"gray=True with colour type {ct}"):
            decode_pngs(c.blobs, gray=True)
    with pytest.raises(TbnHipError, match=r"image 0: png: bit depth 16 is not supported"):
        decode_pngs([U.png(np.zeros((2, 2, 1), np.uint8), 0, bit_depth=16)])


def test_decode_frames_dispatches_by_content():
    from tests import jpeg_ref as R
    from attention_based_tbn_amd.core.dataset.frames import decode_frames, decode_jpegs
    names = [n for n in R.color_names() if "_40x56_" in n][:3]
    jpegs = [R.blob(n) for n in names]
    for gray in (False, True):
        assert torch.equal(decode_frames(jpegs, gray=gray), decode_jpegs(jpegs, gray=gray))
    assert torch.equal(decode_frames(jpegs, entropy="device"), decode_jpegs(jpegs, entropy="device"))
    c = U.make_case(41, 2, (40, 56), (4, 3, 2, 1, 0), "random", U.STREAMS[1], 2)
    mixed = [jpegs[0], c.blobs[0], jpegs[1], jpegs[2], c.blobs[1]]
    got = decode_frames(mixed, inflate="device").cpu().numpy()
    want = decode_jpegs(jpegs).cpu().numpy()
    assert np.array_equal(got[[0, 2, 3]], want) and np.array_equal(got[[1, 4]], c.frames())
    assert np.array_equal(decode_frames(c.blobs).cpu().numpy(), c.frames())
    gray_png = U.make_case(42, 0, (40, 56), (3,), "random", U.STREAMS[1], 1)
    got = decode_frames([jpegs[0]] + gray_png.blobs, gray=True).cpu().numpy()
    assert np.array_equal(got[0], decode_jpegs(jpegs[:1], gray=True).cpu().numpy()[0]) and np.array_equal(got[1:], gray_png.frames(gray=True))


# ---- file_ext "png" through the readers ------------------------------------------------------------------------------------
H, W = 40, 56


def _rgb_pixels(vid, idx):
    return np.random.RandomState(1000 * (1 + CU.VIDS.index(vid)) + idx).randint(0, 256, (H, W, 3)).astype(np.uint8)


def _flow_pixels(vid, axis, idx):
    return np.random.RandomState(5000 * (1 + CU.VIDS.index(vid)) + 2 * idx + (axis == "y")).randint(0, 256, (H, W, 1)).astype(np.uint8)



def _write_png_dataset(root):
    """the clip-loader tests' dataset (tests/clip_loader_util.py), its frames written as PNG of known pixels: RGB files
    colour type 2, flow planes colour type 0, adaptive-looking filter schedules, the stream in several IDAT chunks"""
    overrides = CU.write_dataset(root)
    for vid in CU.VIDS:
        for i in range(CU.N_FILES):
            os.remove(os.path.join(root, "rgb", vid, "img_{:010d}.jpg".format(i)))
            with open(os.path.join(root, "rgb", vid, "img_{:010d}.png".format(i)), "wb") as f:
                f.write(U.png(_rgb_pixels(vid, i), 2, (4, 3, 2, 1, 0), U.SPLITS))
            for axis in ("x", "y"):
                os.remove(os.path.join(root, "flow", vid, "{}_{:010d}.jpg".format(axis, i)))
                with open(os.path.join(root, "flow", vid, "{}_{:010d}.png".format(axis, i)), "wb") as f:
                    f.write(U.png(_flow_pixels(vid, axis, i), 0, (1, 4), (5,), ancillary=[(b"gAMA", b"\0\0\xb1\x8f")]))
    return overrides + ["data.rgb.file_ext=png", "data.flow.file_ext=png"]


def _expected_batch(cfg, mode, rows, seed):
    """`DevicePipeline.__call__` on the written pixels, clip after clip in the reference's draw order"""
    from attention_based_tbn_amd.core.dataset import frame_span, get_offsets, get_transforms
    modality = ["RGB", "Flow"]
    tfs = get_transforms(cfg, modality, mode, flow_length=2 * cfg.data.flow.win_length)
    win = cfg.data.flow.win_length
    out = {m: [] for m in modality}
    np.random.seed(seed)
    for row in rows:
        _, vid, start, stop, _, _ = CU.ROWS[row]
        first, num = frame_span(start, stop)
        idx = {}
        for m_no, m in enumerate(modality):
            if m_no > 0 and cfg.data.sampling == "sync":
                idx[m] = (idx["RGB"] / 2).astype(np.int64)
            else:
                idx[m] = get_offsets(first[m], num[m], m, mode, 2, win if m == "Flow" else 1)
            if m == "RGB":
                frames = np.stack([_rgb_pixels(vid, int(i))[:, :, ::-1] for i in idx[m]])
            else:
                frames = np.stack([_flow_pixels(vid, axis, int(i) + k) for i in idx[m] for k in range(win) for axis in ("x", "y")])
            out[m].append(tfs[m](torch.from_numpy(frames.copy())))
    return {m: torch.stack(v) for m, v in out.items()}


def test_frame_reader_reads_png(tmp_path):
    from attention_based_tbn_amd.core.dataset import FrameReader
    _write_png_dataset(str(tmp_path))
    for inflate in ("host", "device"):
        reader = FrameReader(str(tmp_path), "rgb", "flow", file_ext="png", inflate=inflate)
        got = reader.read_rgb("P01_02", [3, 0, 16]).cpu().numpy()
        assert np.array_equal(got, np.stack([_rgb_pixels("P01_02", i)[:, :, ::-1] for i in (3, 0, 16)]))
        got = reader.read_flow("P01_01", [2, 7]).cpu().numpy()
        assert np.array_equal(got, np.stack([_flow_pixels("P01_01", a, i) for i in (2, 7) for a in ("x", "y")]))
    with pytest.raises(ValueError, match="FrameReader: inflate='x' is not 'host' or 'device'"):
        FrameReader(str(tmp_path), "rgb", "flow", inflate="x")


@pytest.mark.parametrize("mode, inflate", [("train", "host"), ("test", "device")])
def test_video_dataset_with_png_frames(tmp_path, mode, inflate, monkeypatch):
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import dataset as D
    cfg = load_config(_write_png_dataset(str(tmp_path)))
    ds = CU.make_dataset(cfg, ["RGB", "Flow"], mode, inflate=inflate)
    rows = [2, 0, 1]
    want = _expected_batch(cfg, mode, rows, 7)
    np.random.seed(7)
    data = ds.batch(rows)[0]
    for m in ("RGB", "Flow"):
        assert torch.equal(data[m].cpu(), want[m].cpu()), m
    # keep=: the clips outside it cost one 33-byte header per modality, their files are not read
    reads = []
    real_read = D.FrameReader._read
    monkeypatch.setattr(D.FrameReader, "_read", staticmethod(lambda p: (reads.append(p), real_read(p))[1]))
    monkeypatch.setattr(D, "jpeg_frame_size", lambda p: pytest.fail("a PNG dataset asked for a JPEG frame header"))
    np.random.seed(7)
    part = ds.batch(rows, keep=[1])[0]
    for m in ("RGB", "Flow"):
        assert torch.equal(part[m].cpu(), want[m][1:2].cpu()), m
    assert reads and all("P01_01" in p and p.endswith(".png") for p in reads)        # row 0 alone, the kept clip
    with pytest.raises(ValueError, match="Video_Dataset: inflate='x' is not 'host' or 'device'"):
        CU.make_dataset(cfg, ["RGB"], mode, inflate="x")


def test_create_dataloader_takes_inflate(tmp_path):
    import logging
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.utils.create_dataloader import create_dataloader
    cfg = load_config(_write_png_dataset(str(tmp_path)))
    loader = create_dataloader(cfg, logging.getLogger("png"), ["RGB"], "test", inflate="device")
    assert loader.dataset.inflate == "device"
    want = _expected_batch(cfg, "test", [0, 1], 0)
    data = next(iter(loader))[0]
    assert torch.equal(data["RGB"].cpu(), want["RGB"].cpu())


def test_the_flow_pickle_tool_reads_png_planes(tmp_path):
    from attention_based_tbn_amd.preprocessing.create_epic_flow_pickle import main
    win = 3
    planes = {uv: [np.random.RandomState(10 * k + (uv == "v")).randint(0, 256, (20, 28, 1)).astype(np.uint8) for k in range(7)]
              for uv in "uv"}
    for uv in "uv":
        d = tmp_path / "flow" / "P01" / "P01_01" / uv
        d.mkdir(parents=True)
        for i in range(7):
            (d / "frame_{:010d}.png".format(i + 1)).write_bytes(U.png(planes[uv][i], 0, (4, 2), (3,)))
    csv = tmp_path / "annotations.csv"
    csv.write_text("uid,participant_id,video_id,start_frame,stop_frame\n0,P01,P01_01,2,14\n")
    written, kept = main([str(csv), str(tmp_path / "flow"), "--out-dir", str(tmp_path / "out"), "--win-len", str(win),
                          "--file-format", "frame_{:010d}.png"])
    assert len(written) >= 3 and kept == []
    for path in written:
        idx = int(os.path.basename(path)[6:16]) + 1
        want = np.concatenate([planes[uv][idx + i - 1] for i in range(win) for uv in "uv"], axis=2)
        with np.load(path) as z:
            assert z.files == ["flow"] and np.array_equal(z["flow"], want), path
