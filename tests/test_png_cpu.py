"""PNG frames, the host side: the container parser (csrc/tbn_png_host.h) with every refusal, and the host twins of the
device half (tbn_png_decode_host: decoder core, Adler-32 pieces, unfilter) against the written pixels over the whole case
set of tests/png_util.py -- exact equality, PNG is lossless.  No GPU."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest

from tests import png_util as U


def _lib():
    from attention_based_tbn_amd._lib import lib
    return lib()


def _parse(blob):
    from attention_based_tbn_amd._lib import PngGeometry
    g = PngGeometry()
    rc = _lib().tbn_png_parse(blob, len(blob), C.byref(g))
    return rc, g, (_lib().tbn_last_error() or b"").decode()


def _gather(blob):
    rc, g, msg = _parse(blob)
    assert rc == 0, msg
    z = np.zeros(int(_lib().tbn_png_gather_bytes(g.idat_bytes)), np.uint8)
    pal = np.zeros(1024, np.uint8)
    begin, end, adler = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = _lib().tbn_png_gather(blob, len(blob), C.byref(g), z.ctypes.data, pal.ctypes.data, C.byref(begin), C.byref(end), C.byref(adler))
    return rc, (_lib().tbn_last_error() or b"").decode(), z, pal, (begin.value, end.value, adler.value)


@pytest.fixture(scope="module")
def cases():
    return U.case_set(U.limits())


SMALL = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)


def test_import_surface():
    from attention_based_tbn_amd.core import dataset
    from attention_based_tbn_amd.core.dataset import frames
    for name in ("decode_pngs", "decode_frames", "png_geometry", "png_fallback_count", "decode_jpegs", "FrameReader"):
        assert callable(getattr(dataset, name))
    for name in ("png_limits", "png_frame_size", "is_png", "geometry_key"):
        assert callable(getattr(frames, name))
    assert frames.png_fallback_count() == 0


@pytest.mark.parametrize("ct", U.COLOUR_TYPES)
def test_parser_geometry(ct):
    from attention_based_tbn_amd.core.dataset.frames import geometry_key, png_frame_size, png_geometry
    c = U.make_case(3, ct, (5, 9), (4, 3, 2, 1, 0), "levels", U.STREAMS[1])
    g = png_geometry(c.blobs[0])
    bpp = U.BPP[ct]
    assert (g.width, g.height, g.colour_type, g.bpp) == (9, 5, ct, bpp)
    assert g.raw_bytes == 5 * (1 + 9 * bpp)
    zs = U.deflate(U.filter_rows(c.pixels[0], c.schedule), 6, zlib.Z_DEFAULT_STRATEGY)
    assert g.idat_bytes == len(zs)
    assert g.palette_entries == (7 if ct == 3 else 0)
    assert geometry_key(g) == (9, 5, "png", ct)
    assert png_frame_size(c.blobs[0][:33]) == (5, 9)
    rc, msg, z, pal, (begin, end, adler) = _gather(c.blobs[0])
    assert rc == 0 and begin == 4 and end == 2 + len(zs) - 4
    assert bytes(z[2:2 + len(zs)]) == zs and adler == zlib.adler32(U.filter_rows(c.pixels[0], c.schedule))
    if ct == 3:
        assert np.array_equal(pal[:21].reshape(7, 3), c.palettes[0][:, ::-1]) and not pal[21:768].any()
        assert int(pal[768]) == 7 and not pal[769:].any()


@pytest.mark.parametrize("kw, code, words", [
    (dict(bit_depth=1), -3, "bit depth 1 is not supported"),
    (dict(bit_depth=2), -3, "bit depth 2 is not supported"),
    (dict(bit_depth=4), -3, "bit depth 4 is not supported"),
    (dict(bit_depth=16), -3, "bit depth 16 is not supported"),
    (dict(interlace=1), -3, "Adam7 interlace is not supported"),
])
def test_unsupported_kinds_are_refused_by_name(kw, code, words):
    rc, _, msg = _parse(U.png(SMALL[:, :, :1], 0, **kw))
    assert rc == code and words in msg


def test_a_row_longer_than_the_kernel_keeps_is_refused():
    _, _, max_row = U.limits()
    assert max_row >= 4096 * 4
    ihdr = U.chunk(b"IHDR", struct.pack(">IIBBBBB", max_row // 4 + 1, 1, 8, 6, 0, 0, 0))
    rc, _, msg = _parse(U.SIGNATURE + ihdr + U.chunk(b"IDAT", b"\x78\x9c" + bytes(8)) + U.chunk(b"IEND", b""))
    assert rc == -3 and "scanline" in msg and str(max_row) in msg
    ok = U.chunk(b"IHDR", struct.pack(">IIBBBBB", max_row // 4, 1, 8, 6, 0, 0, 0))
    assert _parse(U.SIGNATURE + ok + U.chunk(b"IDAT", b"\x78\x9c" + bytes(8)) + U.chunk(b"IEND", b""))[0] == 0


def test_container_refusals():
    good = U.png(SMALL, 2, (1,), (3,), ancillary=[(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"k\0v")])
    assert _parse(good)[0] == 0
    rc, _, msg = _parse(b"\xff\xd8\xff\xe0" + good[4:])
    assert rc == -1 and "no PNG signature" in msg
    # critical CRCs count, ancillary ones do not
    at = good.index(b"IDAT")
    bad = bytearray(good)
    bad[at + 5] ^= 1
    rc, _, msg = _parse(bytes(bad))
    assert rc == -1 and "CRC-32 mismatch in chunk IDAT" in msg
    bad = bytearray(good)
    bad[good.index(b"IHDR") + 4 + 13] ^= 1
    assert "CRC-32 mismatch in chunk IHDR" in _parse(bytes(bad))[2]
    bad = bytearray(good)
    bad[good.index(b"gAMA") + 5] ^= 1          # payload changed, CRC now wrong: skipped unread
    assert _parse(bytes(bad))[0] == 0
    rc, _, msg = _parse(good[:-12])
    assert rc == -1 and "stream ends early" in msg and "IEND" in msg
    # IDAT, tEXt, IDAT
    zs = U.deflate(U.filter_rows(SMALL, (0,)), 6, zlib.Z_DEFAULT_STRATEGY)
    ihdr = U.chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 5, 8, 2, 0, 0, 0))
    split = U.SIGNATURE + ihdr + U.chunk(b"IDAT", zs[:5]) + U.chunk(b"tEXt", b"k\0v") + U.chunk(b"IDAT", zs[5:]) + U.chunk(b"IEND", b"")
    rc, _, msg = _parse(split)
    assert rc == -1 and "not consecutive" in msg
    rc, _, msg = _parse(U.SIGNATURE + U.chunk(b"tEXt", b"k\0v") + ihdr + U.chunk(b"IDAT", zs) + U.chunk(b"IEND", b""))
    assert rc == -1 and "not IHDR" in msg
    rc, _, msg = _parse(U.SIGNATURE + U.chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 5, 8, 2, 0, 0, 0) + b"\0") + U.chunk(b"IEND", b""))
    assert rc == -1 and "not 13" in msg
    # palette: missing, not a multiple of 3, more than 256 entries
    idx = np.zeros((5, 7, 1), np.uint8)
    rc, _, msg = _parse(U.png(idx, 3))
    assert rc == -1 and "without PLTE" in msg
    rc, _, msg = _parse(U.png(idx, 3, palette=np.zeros(257 * 3, np.uint8)))
    assert rc == -1 and "PLTE is 771 bytes long" in msg
    rc, _, msg = _parse(U.png(idx, 3, palette=np.zeros(4, np.uint8)))
    assert rc == -1 and "PLTE is 4 bytes long" in msg
    assert _parse(U.png(idx, 3, palette=np.zeros(256 * 3, np.uint8)))[1].palette_entries == 256


@pytest.mark.parametrize("header, words", [
    (b"\x79\x9c", "compression method 9"), (b"\x88\x1c", "window of 2^16"), (b"\x78\xbb", "preset dictionary"), (b"\x78\x9d", "FCHECK"),
])
def test_bad_zlib_headers(header, words):
    zs = U.deflate(U.filter_rows(SMALL, (0,)), 6, zlib.Z_DEFAULT_STRATEGY)
    rc, msg, *_ = _gather(U.png(SMALL, 2, zstream=header + zs[2:], idat_splits=(1,)))
    assert rc == -1 and words in msg


def test_every_truncation_of_a_small_file_is_an_error():
    from attention_based_tbn_amd._lib import PngGeometry
    good = U.png(SMALL, 2, (4, 3, 2, 1, 0), U.SPLITS, ancillary=[(b"tRNS", bytes(6))])
    assert _parse(good)[0] == 0
    for n in range(len(good)):
        rc, _, msg = _parse(good[:n])
        assert rc == -1 and msg.startswith("png: "), (n, rc, msg)
        g = PngGeometry()
        rc = _lib().tbn_png_parse_header(good[:n], n, C.byref(g))
        assert (rc == 0) == (n >= 33), n


def test_decode_host_equals_the_written_pixels_on_the_whole_case_set(cases):
    """the condition that lets the GPU test demand png_fallback_count() == 0"""
    seen = set()
    for c in cases + U.frame_batch():
        frames, status, info = U.decode_host(c.blobs)
        assert status == [0] * len(c.blobs), c.name
        assert np.array_equal(frames, c.frames()), c.name
        if c.colour_type in (0, 4):
            gray, status, _ = U.decode_host(c.blobs, gray=True)
            assert status == [0] * len(c.blobs) and np.array_equal(gray, c.frames(gray=True)), c.name
        seen.add((c.colour_type, c.schedule, c.kind, c.stream[0]))
    assert len(seen) == 5 * 6 * 3 * 3        # every colour type x schedule x pixel kind x stream kind came up


def test_unfilter_host_alone_and_colour_read_as_gray():
    from attention_based_tbn_amd._lib import PngGeometry
    c = U.make_case(9, 6, (3, 5), (4,), "random", U.STREAMS[1], 2)
    g = PngGeometry()
    assert _lib().tbn_png_parse(c.blobs[0], len(c.blobs[0]), C.byref(g)) == 0
    raw = np.frombuffer(b"".join(U.filter_rows(p, (4,)) for p in c.pixels), np.uint8).copy()
    frames = np.zeros((2, 3, 5, 3), np.uint8)
    status = (C.c_int * 2)()
    assert _lib().tbn_png_unfilter_host(raw.ctypes.data, None, 2, C.byref(g), 3, frames.ctypes.data, C.addressof(status)) == 0
    assert list(status) == [0, 0] and np.array_equal(frames, c.frames())
    rc = _lib().tbn_png_unfilter_host(raw.ctypes.data, None, 2, C.byref(g), 1, frames.ctypes.data, C.addressof(status))
    assert rc == -1 and b"colour read as gray" in _lib().tbn_last_error()


def test_the_three_new_statuses():
    c = U.make_case(11, 0, (6, 9), (1,), "random", U.STREAMS[0], 3)      # stored blocks: stream bytes are scanline bytes

    # a flipped Adler-32 byte
    frames, status, _ = U.decode_host(c.blobs, table_edit=lambda t: setattr(t[1], "adler", t[1].adler ^ 0x100))
    assert status == [0, 20, 0] and np.array_equal(frames[[0, 2]], c.frames()[[0, 2]])
    # a filter byte set to 5, with the Adler-32 of those bytes so that the unfilter stage is reached
    raw = bytearray(U.filter_rows(c.pixels[2], (1,)))
    raw[2 * 10] = 5
    blobs = [c.blobs[0], c.blobs[1], U.png(c.pixels[2], 0, raw=bytes(raw), level=0)]
    frames, status, _ = U.decode_host(blobs)
    assert status == [0, 0, 21] and np.array_equal(frames[:2], c.frames()[:2])
    # an index past the palette
    idx = np.array([[0, 1, 2], [2, 1, 3]], np.uint8)[:, :, None]
    pal = np.arange(9, dtype=np.uint8).reshape(3, 3)
    frames, status, _ = U.decode_host([U.png(idx, 3, palette=pal), U.png(np.minimum(idx, 2), 3, palette=pal)])
    assert status == [22, 0]
    assert np.array_equal(frames[1], U.expected(np.minimum(idx, 2), 3, pal)) and not frames[0, 1, 2].any()
    # an inflate status passes through: a stream cut short is 7 (input exhausted)
    frames, status, _ = U.decode_host(c.blobs, table_edit=lambda t: setattr(t[0], "in_len", t[0].in_len - 9))
    assert status[0] == 7 and status[1:] == [0, 0]
    frames, status, _ = U.decode_host(c.blobs, table_edit=lambda t: setattr(t[2], "in_off", t[2].in_off + 1))
    assert status == [0, 0, 12]


def test_pillow_reads_the_writers_files(cases):
    Image = pytest.importorskip("PIL.Image")
    for c in cases[::7] + U.frame_batch(1):
        for blob, px, pal in zip(c.blobs, c.pixels, c.palettes):
            im = Image.open(io.BytesIO(blob))
            im.load()
            want = U.expected(px, c.colour_type, pal)[:, :, ::-1]
            assert np.array_equal(np.asarray(im.convert("RGB")), want), c.name
            if c.colour_type in (4, 6):
                assert np.array_equal(np.asarray(im.convert("RGBA"))[:, :, 3], px[:, :, -1]), c.name


def test_decode_pngs_without_a_gpu_raises():
    import torch
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.dataset.frames import decode_frames, decode_pngs
    blob = U.png(SMALL, 2)
    with pytest.raises(ValueError, match="inflate='zlib' is not 'host' or 'device'"):
        decode_pngs([blob], inflate="zlib")
    if not torch.cuda.is_available():       # on a GPU box tests/test_png_gpu.py has the other half
        with pytest.raises(TbnHipError, match=r"decode_pngs: needs an MI355X \(no CPU fallback\)"):
            decode_pngs([blob])
        with pytest.raises(TbnHipError, match=r"decode_pngs: needs an MI355X"):
            decode_frames([blob])
