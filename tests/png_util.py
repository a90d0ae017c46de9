"""A PNG writer for the PNG tests (`struct` + `zlib` only), so that every case is chosen and none is left to an encoder:
the filter type of every row is forced, the zlib stream is cut into IDAT chunks at given lengths, the deflate level and
strategy pick stored / dynamic / fixed blocks, and ancillary chunks can be put in front of the data.

`case_set(limits)` is the case set both test files run: the smallest shapes at which the unfilter kernel can go wrong."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SPLITS = (1, 0, 7)          # a 1-byte first IDAT (inside the zlib header), an empty one, a 7-byte one, then the rest
SCHEDULES = ((0,), (1,), (2,), (3,), (4,), (4, 3, 2, 1, 0))
STREAMS = ((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_FIXED))     # stored, dynamic, fixed blocks
COLOUR_TYPES = (0, 2, 3, 4, 6)
kBand, kStep = 64, 64       # csrc/tbn_png_core.h (kBandRows, kStepTile); the tests read them from the library instead
BASE_SIZES = ((1, 1), (1, 2), (2, 3), (63, 5), (64, 64), (65, 67), (129, 3), (5, 130))


def chunk(kind, payload, crc=None):
    body = kind + payload
    return struct.pack(">I", len(payload)) + body + struct.pack(">I", zlib.crc32(body) if crc is None else crc)


def filter_rows(pixels, types):
    """(H, W, bpp) uint8 -> the scanlines with their filter bytes; row y is filtered with types[y % len(types)]"""
    h, w, bpp = pixels.shape
    cur = pixels.reshape(h, w * bpp).astype(np.int32)
    out = bytearray()
    zero = np.zeros(w * bpp, np.int32)
    for y in range(h):
        t = types[y % len(types)]
        x = cur[y]
        b = cur[y - 1] if y > 0 else zero
        a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if w > 1 else np.zeros(w * bpp, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if w > 1 else np.zeros(w * bpp, np.int32)
        if t == 0:
            pred = zero
        elif t == 1:
            pred = a
        elif t == 2:
            pred = b
        elif t == 3:
            pred = (a + b) >> 1
        elif t == 4:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        else:
            raise ValueError(t)
        out.append(t)
        out += ((x - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw, level, strategy):
    z = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return z.compress(raw) + z.flush()


def png(pixels, colour_type, filter_types=(0,), idat_splits=(), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, palette=None,
        ancillary=(), bit_depth=8, interlace=0, raw=None, zstream=None):
    """pixels (H, W, bpp) uint8 (palette indices for colour type 3) -> the bytes of a PNG file.  `ancillary`: (kind,
    payload) chunks placed between IHDR and PLTE / IDAT.  `raw` replaces the filtered scanlines, `zstream` the whole zlib
    stream (for damaged files)."""
    pixels = np.asarray(pixels, np.uint8)
    if pixels.ndim == 2:
        pixels = pixels[:, :, None]
    h, w, bpp = pixels.shape
    assert bpp == BPP[colour_type]
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth, colour_type, 0, 0, interlace))]
    for kind, payload in ancillary:
        out.append(chunk(kind, payload))
    if palette is not None:
        out.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    if zstream is None:
        zstream = deflate(filter_rows(pixels, filter_types) if raw is None else raw, level, strategy)
    at = 0
    for n in idat_splits:
        out.append(chunk(b"IDAT", zstream[at:at + n]))
        at += n
    out.append(chunk(b"IDAT", zstream[at:]))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def expected(pixels, colour_type, palette=None, gray=False):
    """what cv2.imread gives for the written pixels: (H, W, 3) B, G, R, or (H, W, 1) with gray=True (gray types only)"""
    pixels = np.asarray(pixels, np.uint8)
    if pixels.ndim == 2:
        pixels = pixels[:, :, None]
    if colour_type in (0, 4):
        g = pixels[:, :, :1]
        return g.copy() if gray else np.repeat(g, 3, 2)
    assert not gray
    if colour_type == 3:
        return np.asarray(palette, np.uint8).reshape(-1, 3)[pixels[:, :, 0]][:, :, ::-1].copy()
    return pixels[:, :, 2::-1].copy()


def make_pixels(rng, kind, h, w, colour_type):
    """-> (pixels, palette or None).  kind "random": uniform bytes (the Average 9-bit sum, Paeth ties); "levels": four
    values in runs (long matches for the inflate); "white": all 255"""
    bpp = BPP[colour_type]
    if kind == "random":
        px = rng.randint(0, 256, (h, w, bpp)).astype(np.uint8)
    elif kind == "levels":
        values = np.array([0, 2, 3, 6] if colour_type == 3 else [0, 85, 170, 255], np.uint8)
        runs = rng.randint(0, 4, (h, (w + 7) // 8, bpp))
        px = values[np.repeat(runs, 8, 1)[:, :w]]
    else:
        px = np.full((h, w, bpp), 255, np.uint8)
    palette = None
    if colour_type == 3:
        entries = 7 if kind == "levels" else 256
        palette = rng.randint(0, 256, (entries, 3)).astype(np.uint8)
    return px, palette


class Case(object):
    def __init__(self, name, colour_type, size, schedule, kind, stream, blobs, pixels, palettes):
        self.name, self.colour_type, self.size, self.schedule, self.kind, self.stream = name, colour_type, size, schedule, kind, stream
        self.blobs, self.pixels, self.palettes = blobs, pixels, palettes

    def frames(self, gray=False):
        return np.stack([expected(p, self.colour_type, q, gray) for p, q in zip(self.pixels, self.palettes)])


def make_case(seed, colour_type, size, schedule, kind, stream, n=1, splits=SPLITS):
    rng = np.random.RandomState(seed)
    pixels, palettes, blobs = [], [], []
    for _ in range(n):
        px, pal = make_pixels(rng, kind, size[0], size[1], colour_type)
        pixels.append(px)
        palettes.append(pal)
        blobs.append(png(px, colour_type, schedule, splits, stream[0], stream[1], pal))
    name = f"ct{colour_type}_{size[0]}x{size[1]}_f{''.join(map(str, schedule))}_{kind}_l{stream[0]}_n{n}"
    return Case(name, colour_type, size, schedule, kind, stream, blobs, pixels, palettes)


def sizes(limits):
    """the base sizes plus the heights and widths on both sides of the kernel's band and staging sizes"""
    band, step, _ = limits
    extra = ((band + 1, step + 1), (2, step), (2, 2 * step + 1), (2 * band, 2), (band - 1, step - 1))
    return BASE_SIZES + tuple(s for s in extra if s not in BASE_SIZES)


KINDS = ("random", "levels", "white")
BATCHES = (1, 3, 5)


def case_set(limits, colour_types=COLOUR_TYPES):
    """every size x colour type x filter schedule, with the pixel kind, the stream kind and the batch size rotating through
    them (each pair of pixel kind and stream kind comes up, at every colour type); then every pixel kind x stream kind x
    schedule at the one size that has more than one band and more than one staging pass"""
    out, k = [], 0
    for ct in colour_types:
        for size in sizes(limits):
            for schedule in SCHEDULES:
                r = k + k // len(SCHEDULES)             # shifts by one per size: every schedule meets every pixel kind
                kind, stream = KINDS[r % 3], STREAMS[(r // 3) % 3]
                n = BATCHES[k % 3] if size[0] * size[1] <= 64 * 64 else 1
                out.append(make_case(1000 + k, ct, size, schedule, kind, stream, n))
                k += 1
        for kind in KINDS:
            for stream in STREAMS:
                for schedule in SCHEDULES:
                    out.append(make_case(5000 + k, ct, (65, 67), schedule, kind, stream, 1))
                    k += 1
    return out


def frame_batch(n=4, size=(256, 456)):
    """ONE batch of frame size, gray and RGB, mixed schedule, level 6: n images with differing pixels"""
    return [make_case(77, 0, size, (4, 3, 2, 1, 0), "levels", STREAMS[1], n),
            make_case(78, 2, size, (4, 3, 2, 1, 0), "random", STREAMS[1], n)]


# ---- the library's host side, as both test files drive it ------------------------------------------------------------------
def limits():
    from attention_based_tbn_amd.core.dataset.frames import png_limits
    return png_limits()


def pack(blobs, damage=None):
    """gathers every file as `decode_pngs(inflate="device")` does -> (geometry, uint8 array `packed`, table (PngImage * n),
    in_bytes).  `damage(i, stream)` may change image i's gathered bytearray (its zlib stream starts at byte 2) in place."""
    import ctypes as C
    from attention_based_tbn_amd._lib import PngGeometry, PngImage, lib
    L = lib()
    geos = []
    for b in blobs:
        g = PngGeometry()
        assert L.tbn_png_parse(b, len(b), C.byref(g)) == 0, L.tbn_last_error()
        geos.append(g)
    n = len(blobs)
    slots = [(int(L.tbn_png_gather_bytes(g.idat_bytes)) + 15) // 16 * 16 for g in geos]
    offsets = [sum(slots[:i]) for i in range(n)]
    pal_at = sum(slots)
    packed = np.zeros(pal_at + n * 1024, np.uint8)
    base = packed.ctypes.data
    table = (PngImage * n)()
    begin, end, adler = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    for i, b in enumerate(blobs):
        rc = L.tbn_png_gather(b, len(b), C.byref(geos[i]), base + offsets[i], base + pal_at + i * 1024, C.byref(begin),
                              C.byref(end), C.byref(adler))
        assert rc == 0, L.tbn_last_error()
        if damage is not None:
            damage(i, packed[offsets[i]:offsets[i] + slots[i]])
        table[i].in_off, table[i].in_len = offsets[i] + begin.value, end.value - begin.value
        table[i].palette_off, table[i].adler = pal_at + i * 1024, adler.value
    return geos[0], packed, table, packed.size


def decode_host(blobs, gray=False, damage=None, table_edit=None):
    """tbn_png_decode_host over `blobs` -> (frames (n, H, W, C) uint8, statuses, info)"""
    import ctypes as C
    from attention_based_tbn_amd._lib import lib
    geo, packed, table, in_bytes = pack(blobs, damage)
    if table_edit is not None:
        table_edit(table)
    n, ch = len(blobs), 1 if gray else 3
    frames = np.zeros((n, geo.height, geo.width, ch), np.uint8)
    ws = np.zeros(int(lib().tbn_png_workspace_bytes(C.byref(geo), n)), np.uint8)
    status, info = (C.c_int * n)(), (C.c_int * n)()
    rc = lib().tbn_png_decode_host(packed.ctypes.data, in_bytes, C.addressof(table), n, C.byref(geo), ch, frames.ctypes.data,
                                   ws.ctypes.data, C.addressof(status), C.addressof(info))
    assert rc == 0, lib().tbn_last_error()
    return frames, list(status), list(info)


if __name__ == "__main__":      # python -m tests.png_util --dump DIR: NAME.png and NAME.bgr for scripts/png_check.cpp
    import os
    import sys
    if len(sys.argv) != 3 or sys.argv[1] != "--dump":
        sys.exit("usage: python -m tests.png_util --dump DIR")
    os.makedirs(sys.argv[2], exist_ok=True)
    for case in case_set((kBand, kStep, 16384)) + frame_batch(1):
        for i, (blob, frame) in enumerate(zip(case.blobs, case.frames())):
            stem = os.path.join(sys.argv[2], f"{case.name}_{i}")
            with open(stem + ".png", "wb") as f:
                f.write(blob)
            with open(stem + ".bgr", "wb") as f:
                f.write(frame.tobytes())
