"""Frame loading: JPEG and PNG files -> uint8 frames on the device, the input of `DevicePipeline` (transform.py).

Reference core/dataset/dataset.py:241-420 reads every frame with cv2.imread on the host (libjpeg-turbo: about 1.6 ms of
one core per 456x256 frame).  Here only the serial half stays on the host -- marker parsing and Huffman decoding, in
worker threads (ctypes releases the GIL) -- and the coefficients cross to the device once, where two kernels do
dequantisation, the IDCT, chroma upsampling and the colour conversion (csrc/jpeg.hip).  The frames are byte-identical
to cv2.imread's: (n, H, W, 3) in B, G, R order, or (n, H, W, 1) for cv2.imread(path, 0).

entropy="device" (opt-in) moves the Huffman decoding to the device as well (csrc/jpeg_entropy.hip: self-synchronising
subsequence decoding, one workgroup per image): the workers only unstuff and pack the scan, and roughly the file's
bytes cross to the device instead of its coefficients.  An image the device decoder flags, or one with more restart
intervals than it has lanes, takes the host stage, so the frames are the same either way.

PNG (data.rgb.file_ext / data.flow.file_ext: "png"; cv2.imread decodes by content, so does `decode_frames`): the container
walk and the zlib inflate are the serial half -- host threads by default, `zlib` of the standard library -- and scanline
unfiltering with the conversion to B, G, R (or gray) is one kernel (csrc/png.hip).  inflate="device" (opt-in) moves the
inflate to the device too, one wavefront per image with the decoder core of the flow pickles (csrc/tbn_inflate.h)."""
import ctypes
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import torch

from ..._lib import JpegGeometry, PngGeometry, PngImage, TbnHipError, call, lib, ptr, stream_ptr

MAX_THREADS = 16      # what one job gets on a shared GPU host; never derived from the machine's core count
MAX_INTERVALS = 1024  # lanes of the device entropy decoder: an image of more restart intervals takes the host stage
NO_RECORD = 0xFFFFFFFF
PACK_THREADS = 4      # the pack stage takes some 10 us per call, about what handing the GIL over costs: measured, 16 workers
                      # pack a batch slower than 4, and 4 no faster than 1 for small files (profiles/jpeg_decode.md)

_pools = {}


def _pool(threads):
    if threads not in _pools:
        _pools[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="tbn_jpeg")
    return _pools[threads]


def _last_error():
    msg = lib().tbn_last_error()
    return msg.decode() if msg else ""


def _describe(geo):
    return f"{geo.width}x{geo.height} ({geo.components} component{'s' if geo.components > 1 else ''}, " \
           f"luma sampling {geo.hsamp[0]}x{geo.vsamp[0]})"


def _same(a, b):
    return (a.width, a.height, a.components, list(a.hsamp), list(a.vsamp)) == \
           (b.width, b.height, b.components, list(b.hsamp), list(b.vsamp))


def jpeg_geometry(blob):
    """`tbn_jpeg_parse` of one file (host only, no GPU): the `JpegGeometry` `decode_jpegs` groups by -- files of one
    width, height, component count and sampling decode in one call.  Raises the parser's refusal."""
    blob = blob if isinstance(blob, bytes) else bytes(blob)
    g = JpegGeometry()
    if lib().tbn_jpeg_parse(blob, len(blob), ctypes.byref(g)) != 0:
        raise TbnHipError(f"jpeg_geometry: {_last_error()}")
    return g


def geometry_key(geo):
    """what makes two files one `decode_jpegs` batch: (width, height, components, hsamp, vsamp); of a `png_geometry`
    result, one `decode_pngs` batch: (width, height, "png", colour type)"""
    if isinstance(geo, PngGeometry):
        return (geo.width, geo.height, "png", geo.colour_type)
    return (geo.width, geo.height, geo.components, tuple(geo.hsamp), tuple(geo.vsamp))


def decode_jpegs(blobs, gray=False, device="cuda", threads=8, entropy="host"):
    """list of `bytes` (baseline JPEG files of ONE geometry) -> uint8 (n, H, W, 1 if gray else 3) on `device`.

    Each blob is parsed once; the entropy decoding runs in `threads` (at most 16) workers into one pinned staging
    tensor; one asynchronous copy and one tbn_jpeg_reconstruct follow on the current stream.

    entropy="device": the workers (at most 4 of them) pack the scans (tbn_jpeg_scan_pack), the packed bytes are copied, and
    tbn_jpeg_entropy_decode_dev and tbn_jpeg_reconstruct run on the current stream; reading the status vector is the
    only synchronisation.  Images with a non-zero status, images the pack stage refuses and images of more than 1024
    restart intervals are decoded by the host stage into their slot and reconstructed again; if the host stage refuses
    one too, its message is raised.  Known strictness gap: stray bytes between the last block and the next marker are
    judged by the host stage according to its refill state, so this mode may accept a file there that the host mode
    refuses; whenever both accept, the frames are identical."""
    if entropy not in ("host", "device"):
        raise ValueError(f"decode_jpegs: entropy={entropy!r} is not 'host' or 'device'")
    if not torch.cuda.is_available():
        raise TbnHipError("decode_jpegs: needs an MI355X (no CPU fallback)")
    if not (isinstance(blobs, (list, tuple)) and len(blobs) > 0):
        raise TbnHipError("decode_jpegs: expected a non-empty list of bytes")
    blobs = [b if isinstance(b, bytes) else bytes(b) for b in blobs]
    L = lib()
    geos = []
    for i, b in enumerate(blobs):
        g = JpegGeometry()
        if L.tbn_jpeg_parse(b, len(b), ctypes.byref(g)) != 0:
            raise TbnHipError(f"decode_jpegs: image {i}: {_last_error()}")
        if geos and not _same(geos[0], g):
            raise TbnHipError(f"decode_jpegs: mixed geometries in one batch: image 0 is {_describe(geos[0])}, "
                              f"image {i} is {_describe(g)}")
        geos.append(g)
    geo, n = geos[0], len(blobs)
    device = torch.device(device)
    if entropy == "device":
        return _decode_on_device(L, blobs, geos, gray, device, threads)
    coef_bytes = int(geo.coef_count) * 2                       # a multiple of 128
    quant_bytes = geo.components * 128
    # ONE pinned staging tensor: the coefficients of every image, then the quantisation tables of every image
    # (torch's pinned-memory allocator keeps the block alive until the asynchronous copy below has passed)
    staging = torch.empty(n * (coef_bytes + quant_bytes), dtype=torch.uint8, pin_memory=True)
    base = staging.data_ptr()
    quant_base = base + n * coef_bytes

    def work(first):
        # one task per worker, images first, first + threads, ...: a task per image would cost more in the executor than
        # the ~50 us the decode itself takes
        bad = []
        for i in range(first, n, threads):
            if L.tbn_jpeg_entropy_decode(blobs[i], len(blobs[i]), ctypes.byref(geo), base + i * coef_bytes,
                                         quant_base + i * quant_bytes) != 0:
                bad.append((i, _last_error()))                      # the error string is the worker thread's own
        return bad

    threads = max(1, min(int(threads), MAX_THREADS, n))
    done = [work(0)] if threads == 1 else _pool(threads).map(work, range(threads))
    errors = [f"image {i}: {msg}" for i, msg in sorted(e for part in done for e in part)]
    if errors:
        raise TbnHipError("decode_jpegs: " + "; ".join(errors[:4]))
    dev = staging.to(device, non_blocking=True)
    channels = 1 if gray else 3
    frames = torch.empty((n, geo.height, geo.width, channels), dtype=torch.uint8, device=device)
    ws_bytes = int(L.tbn_jpeg_workspace_bytes(ctypes.byref(geo), n))
    if ws_bytes == 0:
        raise TbnHipError(f"decode_jpegs: {_last_error()}")
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    call("tbn_jpeg_reconstruct", ptr(dev), ptr(dev) + n * coef_bytes, n, ctypes.byref(geo), channels, ptr(frames),
         ptr(workspace), stream_ptr())
    return frames


def _host_decode(L, blobs, geo, indices, threads, coef_bytes, quant_bytes):
    """the host stage for images `indices` -> pinned uint8 (len(indices), coef_bytes + quant_bytes); raises its refusals"""
    k = len(indices)
    staging = torch.empty((k, coef_bytes + quant_bytes), dtype=torch.uint8, pin_memory=True)
    base, stride = staging.data_ptr(), coef_bytes + quant_bytes

    def work(first):
        bad = []
        for j in range(first, k, threads):
            i = indices[j]
            if L.tbn_jpeg_entropy_decode(blobs[i], len(blobs[i]), ctypes.byref(geo), base + j * stride,
                                         base + j * stride + coef_bytes) != 0:
                bad.append((i, _last_error()))
        return bad

    threads = max(1, min(threads, k))
    done = [work(0)] if threads == 1 else _pool(threads).map(work, range(threads))
    errors = [f"image {i}: {msg}" for i, msg in sorted(e for part in done for e in part)]
    if errors:
        raise TbnHipError("decode_jpegs: " + "; ".join(errors[:4]))
    return staging


def _decode_on_device(L, blobs, geos, gray, device, threads):
    geo, n = geos[0], len(blobs)
    coef_bytes = int(geo.coef_count) * 2                       # a multiple of 128
    quant_bytes = geo.components * 128
    mcus = (geo.blocks_w[0] // geo.hsamp[0]) * (geo.blocks_h[0] // geo.vsamp[0])
    # restart_interval is per file (informational in the geometry): so is the interval count
    intervals = [-(-mcus // g.restart_interval) if g.restart_interval else 1 for g in geos]
    caps = [int(L.tbn_jpeg_scan_pack_bytes(len(b), k)) if k <= MAX_INTERVALS else 0 for b, k in zip(blobs, intervals)]
    offsets = [0] * n
    total = 0
    for i in range(n):
        offsets[i], total = total, total + caps[i]
    if total >= 1 << 32:
        raise TbnHipError(f"decode_jpegs: {total} packed bytes are too many for one launch")
    # ONE pinned staging tensor: the records, the record offsets, the quantisation tables (each part 16-byte aligned)
    offsets_at = max(total, 16)
    quant_at = offsets_at + (4 * n + 15) // 16 * 16
    staging = torch.empty(quant_at + n * quant_bytes, dtype=torch.uint8, pin_memory=True)
    base = staging.data_ptr()
    offset_words = staging[offsets_at:offsets_at + 4 * n].view(torch.int32)

    def work(first):
        packed = []
        count, used = ctypes.c_int(0), ctypes.c_size_t(0)
        for i in range(first, n, threads):
            if caps[i] and L.tbn_jpeg_scan_pack(blobs[i], len(blobs[i]), ctypes.byref(geo), base + offsets[i], caps[i],
                                                MAX_INTERVALS, base + quant_at + i * quant_bytes, ctypes.byref(count),
                                                ctypes.byref(used)) == 0 and used.value:
                packed.append(i)
        return packed                     # whatever is not packed takes the host stage, which words the refusal

    host_threads = max(1, min(int(threads), MAX_THREADS, n))
    threads = min(host_threads, PACK_THREADS)
    done = [work(0)] if threads == 1 else _pool(threads).map(work, range(threads))
    packed = set(i for part in done for i in part)
    offset_words.copy_(torch.tensor([offsets[i] if i in packed else NO_RECORD - (1 << 32) for i in range(n)], dtype=torch.int32))
    dev = staging.to(device, non_blocking=True)
    channels = 1 if gray else 3
    coef = torch.empty(n * coef_bytes, dtype=torch.uint8, device=device)
    status = torch.empty(n, dtype=torch.int32, device=device)
    info = torch.empty((n, 2), dtype=torch.int32, device=device)
    frames = torch.empty((n, geo.height, geo.width, channels), dtype=torch.uint8, device=device)
    ews_bytes = int(L.tbn_jpeg_entropy_workspace_bytes(ctypes.byref(geo), n))
    ws_bytes = int(L.tbn_jpeg_workspace_bytes(ctypes.byref(geo), n))
    if ews_bytes == 0 or ws_bytes == 0:
        raise TbnHipError(f"decode_jpegs: {_last_error()}")
    entropy_ws = torch.empty(ews_bytes, dtype=torch.uint8, device=device)
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    call("tbn_jpeg_entropy_decode_dev", ptr(dev), max(total, 16), ptr(dev) + offsets_at, n, ctypes.byref(geo), 0, ptr(coef),
         ptr(status), ptr(info), ptr(entropy_ws), stream_ptr())
    call("tbn_jpeg_reconstruct", ptr(coef), ptr(dev) + quant_at, n, ctypes.byref(geo), channels, ptr(frames),
         ptr(workspace), stream_ptr())
    redo = [i for i, s in enumerate(status.tolist()) if s != 0]        # one small copy back: the only synchronisation
    if redo:
        host = _host_decode(L, blobs, geo, redo, host_threads, coef_bytes, quant_bytes)
        fixed = host.to(device, non_blocking=True)
        frame_bytes = geo.height * geo.width * channels
        for j, i in enumerate(redo):
            coef[i * coef_bytes:(i + 1) * coef_bytes].copy_(fixed[j, :coef_bytes], non_blocking=True)
            quant_i = torch.empty(quant_bytes, dtype=torch.uint8, device=device)
            quant_i.copy_(fixed[j, coef_bytes:], non_blocking=True)
            call("tbn_jpeg_reconstruct", ptr(coef) + i * coef_bytes, ptr(quant_i), 1, ctypes.byref(geo), channels,
                 ptr(frames) + i * frame_bytes, ptr(workspace), stream_ptr())
    return frames


# ---- PNG ---------------------------------------------------------------------------------------------------------------
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_HEADER_BYTES = 33        # signature + IHDR with its CRC: all `png_frame_size` reads
PNG_PALETTE_BYTES = 1024     # one image's palette slot (include/tbn_hip.h, tbn_png_gather)
_PNG_GRAY_TYPES = (0, 4)
_png_fallbacks = 0


def is_png(blob):
    """does the file start with the PNG signature?  (cv2.imread picks its decoder the same way: by content)"""
    return bytes(blob[:8]) == PNG_SIGNATURE


def png_limits():
    """the sizes at which the unfilter kernel changes its path: (rows of a band, pixel steps between two staging passes,
    longest scanline in bytes) -- tests put heights and widths on both sides of them"""
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    call("tbn_png_limits", ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def png_geometry(blob):
    """`tbn_png_parse` of one file (host only, no GPU): the `PngGeometry` `decode_pngs` groups by -- files of one width,
    height and colour type decode in one call.  Raises the parser's refusal."""
    blob = blob if isinstance(blob, bytes) else bytes(blob)
    g = PngGeometry()
    if lib().tbn_png_parse(blob, len(blob), ctypes.byref(g)) != 0:
        raise TbnHipError(f"png_geometry: {_last_error()}")
    return g


def png_frame_size(head):
    """(H, W) from the first 33 bytes of a PNG file (signature and IHDR, its CRC checked); host only"""
    head = bytes(head[:PNG_HEADER_BYTES])
    g = PngGeometry()
    if lib().tbn_png_parse_header(head, len(head), ctypes.byref(g)) != 0:
        raise TbnHipError(f"png_frame_size: {_last_error()}")
    return (g.height, g.width)


def png_fallback_count():
    """images that `decode_pngs(inflate="device")` has sent to the host stage since the process began"""
    return _png_fallbacks


def _describe_png(geo):
    return f"{geo.width}x{geo.height} (colour type {geo.colour_type})"


def _png_host_stage(L, blobs, geos, indices, threads):
    """the host stage for images `indices`: gather, zlib inflate (which checks the Adler-32), filter bytes and palette
    indices looked over -> (pinned uint8 staging, offset of the palettes in it): the scanlines of every image, dense,
    then a palette slot per image.  Raises its refusals, naming the images."""
    geo, k = geos[indices[0]], len(indices)
    raw_bytes, stride = int(geo.raw_bytes), 1 + geo.width * geo.bpp
    pal_at = (k * raw_bytes + 15) // 16 * 16
    staging = torch.empty(pal_at + k * PNG_PALETTE_BYTES, dtype=torch.uint8, pin_memory=True)
    base = staging.data_ptr()
    threads = max(1, min(int(threads), MAX_THREADS, k))

    def work(first):
        bad = []
        begin, end, adler = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        for j in range(first, k, threads):
            i = indices[j]
            g = geos[i]
            z = bytearray(int(L.tbn_png_gather_bytes(g.idat_bytes)))
            zbuf = (ctypes.c_ubyte * len(z)).from_buffer(z)
            if L.tbn_png_gather(blobs[i], len(blobs[i]), ctypes.byref(g), ctypes.addressof(zbuf), base + pal_at + j * PNG_PALETTE_BYTES,
                                ctypes.byref(begin), ctypes.byref(end), ctypes.byref(adler)) != 0:
                bad.append((i, _last_error()))
                continue
            del zbuf
            try:
                inflater = zlib.decompressobj()
                raw = inflater.decompress(memoryview(z)[2:2 + int(g.idat_bytes)], raw_bytes + 1)     # zlib releases the GIL
            except zlib.error as e:
                bad.append((i, f"png: zlib stream: {e}"))
                continue
            if len(raw) > raw_bytes:
                bad.append((i, f"png: the zlib stream inflates to more than the {raw_bytes} bytes of the scanlines"))
                continue
            if len(raw) < raw_bytes or not inflater.eof:
                bad.append((i, f"png: the zlib stream ends early, after {len(raw)} of {raw_bytes} scanline bytes"))
                continue
            ctypes.memmove(base + j * raw_bytes, raw, raw_bytes)
            lines = staging[j * raw_bytes:(j + 1) * raw_bytes].view(g.height, stride)
            filters = lines[:, 0]
            if int(filters.max()) > 4:
                y = int((filters > 4).nonzero()[0])
                bad.append((i, f"png: scanline {y} has filter type {int(filters[y])} (0..4 exist)"))
            # a palette index beyond PLTE cannot be seen before unfiltering: the kernel's status 22 says so (decode_pngs)
        return bad

    done = [work(0)] if threads == 1 else _pool(threads).map(work, range(threads))
    errors = [f"image {i}: {msg}" for i, msg in sorted(e for part in done for e in part)]
    if errors:
        raise TbnHipError("decode_pngs: " + "; ".join(errors[:4]))
    return staging, pal_at


def _png_unfilter(L, staging, pal_at, k, geo, channels, device, indices):
    """staging (from `_png_host_stage`) -> frames (k, H, W, channels) on `device`: one copy, one tbn_png_unfilter.  Of
    palette files alone the status vector is read back (an index beyond PLTE cannot be judged before unfiltering); the
    filter bytes of every file were looked over on the host, so the other colour types need no synchronisation."""
    dev = staging.to(device, non_blocking=True)
    frames = torch.empty((k, geo.height, geo.width, channels), dtype=torch.uint8, device=device)
    status = torch.empty(k, dtype=torch.int32, device=device)
    call("tbn_png_unfilter", ptr(dev), ptr(dev) + pal_at, k, ctypes.byref(geo), channels, ptr(frames), ptr(status), stream_ptr())
    if geo.colour_type == 3:
        bad = [(indices[j], s) for j, s in enumerate(status.tolist()) if s != 0]
        if bad:
            raise TbnHipError("decode_pngs: " + "; ".join(
                f"image {i}: png: a palette index at or beyond the {'PLTE entry count' if s == 22 else f'limit (status {s})'}"
                for i, s in bad[:4]))
    return frames


def decode_pngs(blobs, gray=False, device="cuda", threads=8, inflate="host"):
    """list of `bytes` (PNG files of ONE geometry: width, height, colour type) -> uint8 (n, H, W, 1 if gray else 3) on
    `device`: B, G, R as cv2.imread(path) gives them (gray replicated, alpha dropped, palette looked up), or the gray
    plane of a gray file for cv2.imread(path, 0).  A colour or palette file with gray=True raises: cv2 converts it
    through a formula that is not reproduced here.

    inflate="host" (the default): `threads` (at most 16) workers gather the IDAT chunks and inflate them with `zlib`
    (Adler-32 checked) into one pinned staging tensor; one asynchronous copy and one tbn_png_unfilter follow on the
    current stream.

    inflate="device": the workers only gather, roughly the files' bytes are copied, and tbn_png_decode (inflate, Adler-32,
    unfilter) runs on the current stream; reading the status vector is the only synchronisation.  An image with a
    non-zero status takes the host stage into its slot and is unfiltered again (`png_fallback_count()` counts them); if
    the host stage refuses it too, its message is raised, naming the image."""
    global _png_fallbacks
    if inflate not in ("host", "device"):
        raise ValueError(f"decode_pngs: inflate={inflate!r} is not 'host' or 'device'")
    if not torch.cuda.is_available():
        raise TbnHipError("decode_pngs: needs an MI355X (no CPU fallback)")
    if not (isinstance(blobs, (list, tuple)) and len(blobs) > 0):
        raise TbnHipError("decode_pngs: expected a non-empty list of bytes")
    blobs = [b if isinstance(b, bytes) else bytes(b) for b in blobs]
    L = lib()
    geos = []
    for i, b in enumerate(blobs):
        g = PngGeometry()
        if L.tbn_png_parse(b, len(b), ctypes.byref(g)) != 0:
            raise TbnHipError(f"decode_pngs: image {i}: {_last_error()}")
        if geos and geometry_key(geos[0]) != geometry_key(g):
            raise TbnHipError(f"decode_pngs: mixed geometries in one batch: image 0 is {_describe_png(geos[0])}, "
                              f"image {i} is {_describe_png(g)}")
        geos.append(g)
    geo, n = geos[0], len(blobs)
    if gray and geo.colour_type not in _PNG_GRAY_TYPES:
        raise TbnHipError(f"decode_pngs: gray=True with colour type {geo.colour_type}: a colour or palette file read as gray "
                          "is not supported (types 0 and 4 are)")
    device = torch.device(device)
    channels = 1 if gray else 3
    if inflate == "host":
        staging, pal_at = _png_host_stage(L, blobs, geos, list(range(n)), threads)
        return _png_unfilter(L, staging, pal_at, n, geo, channels, device, list(range(n)))
    # ONE pinned staging tensor: every image's zlib stream (16-byte aligned slots), its palette slot, then the image table
    slots = [(int(L.tbn_png_gather_bytes(g.idat_bytes)) + 15) // 16 * 16 for g in geos]
    offsets, total = [0] * n, 0
    for i in range(n):
        offsets[i], total = total, total + slots[i]
    pal_at = total
    table_at = pal_at + n * PNG_PALETTE_BYTES
    in_bytes = table_at
    staging = torch.empty(table_at + n * ctypes.sizeof(PngImage), dtype=torch.uint8, pin_memory=True)
    base = staging.data_ptr()
    table = (PngImage * n).from_address(base + table_at)
    threads = max(1, min(int(threads), MAX_THREADS, n))

    def work(first):
        begin, end, adler = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        for i in range(first, n, threads):
            row = table[i]
            row.in_off, row.palette_off, row.in_len, row.adler = offsets[i] + 4, pal_at + i * PNG_PALETTE_BYTES, 0, 0
            if L.tbn_png_gather(blobs[i], len(blobs[i]), ctypes.byref(geos[i]), base + offsets[i], base + row.palette_off,
                                ctypes.byref(begin), ctypes.byref(end), ctypes.byref(adler)) == 0:
                row.in_off, row.in_len, row.adler = offsets[i] + begin.value, end.value - begin.value, adler.value
            # a refused file keeps in_len 0: status 7 on the device, and the host stage words the refusal

    if threads == 1:
        work(0)
    else:
        list(_pool(threads).map(work, range(threads)))
    dev = staging.to(device, non_blocking=True)
    frames = torch.empty((n, geo.height, geo.width, channels), dtype=torch.uint8, device=device)
    status = torch.empty(n, dtype=torch.int32, device=device)
    info = torch.empty(n, dtype=torch.int32, device=device)
    ws_bytes = int(L.tbn_png_workspace_bytes(ctypes.byref(geo), n))
    if ws_bytes == 0:
        raise TbnHipError(f"decode_pngs: {_last_error()}")
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    call("tbn_png_decode", ptr(dev), in_bytes, ptr(dev) + table_at, n, ctypes.byref(geo), channels, ptr(frames), ptr(workspace),
         ptr(status), ptr(info), stream_ptr())
    redo = [i for i, s in enumerate(status.tolist()) if s != 0]        # one small copy back: the only synchronisation
    if redo:
        _png_fallbacks += len(redo)
        fixed, fixed_pal = _png_host_stage(L, blobs, geos, redo, threads)
        part = _png_unfilter(L, fixed, fixed_pal, len(redo), geo, channels, device, redo)
        frames.index_copy_(0, torch.tensor(redo, device=device), part)
    return frames


def decode_frames(blobs, gray=False, device="cuda", threads=8, entropy="host", inflate="host"):
    """list of `bytes`, JPEG or PNG by content (the PNG signature; cv2.imread of reference core/dataset/dataset.py:305
    decides the same way), of ONE frame size -> uint8 (n, H, W, 1 if gray else 3) on `device`.  All JPEG: exactly
    `decode_jpegs(blobs, gray, device, threads, entropy)`; all PNG: `decode_pngs(..., inflate)`; mixed: one call per
    kind, scattered into place."""
    if not (isinstance(blobs, (list, tuple)) and len(blobs) > 0):
        raise TbnHipError("decode_frames: expected a non-empty list of bytes")
    png = [i for i, b in enumerate(blobs) if is_png(b)]
    if not png:
        return decode_jpegs(blobs, gray=gray, device=device, threads=threads, entropy=entropy)
    if len(png) == len(blobs):
        return decode_pngs(blobs, gray=gray, device=device, threads=threads, inflate=inflate)
    marked = set(png)
    jpg = [i for i in range(len(blobs)) if i not in marked]
    a = decode_jpegs([blobs[i] for i in jpg], gray=gray, device=device, threads=threads, entropy=entropy)
    b = decode_pngs([blobs[i] for i in png], gray=gray, device=device, threads=threads, inflate=inflate)
    if a.shape[1:] != b.shape[1:]:
        raise TbnHipError(f"decode_frames: mixed frame sizes in one batch: the JPEG files are {a.shape[2]}x{a.shape[1]}, "
                          f"the PNG files {b.shape[2]}x{b.shape[1]}")
    frames = torch.empty((len(blobs),) + tuple(a.shape[1:]), dtype=torch.uint8, device=a.device)
    frames.index_copy_(0, torch.tensor(jpg, device=a.device), a)
    frames.index_copy_(0, torch.tensor(png, device=a.device), b)
    return frames


class FrameReader(object):
    """The file layout of reference core/dataset/dataset.py: root_dir/<prefix>/<vid_id>/img_%010d.ext (RGB) and
    x_%010d.ext, y_%010d.ext (Flow).  Both readers return the uint8 device tensor `DevicePipeline.__call__` takes.
    JPEG or PNG is decided per file by content (`decode_frames`), whatever `file_ext` says."""

    def __init__(self, root_dir, rgb_prefix, flow_prefix, file_ext="jpg", device="cuda", threads=8, entropy="host",
                 inflate="host"):
        if entropy not in ("host", "device"):
            raise ValueError(f"FrameReader: entropy={entropy!r} is not 'host' or 'device'")
        if inflate not in ("host", "device"):
            raise ValueError(f"FrameReader: inflate={inflate!r} is not 'host' or 'device'")
        self.root_dir, self.rgb_prefix, self.flow_prefix, self.file_ext = root_dir, rgb_prefix, flow_prefix, file_ext
        self.device, self.threads, self.entropy, self.inflate = device, threads, entropy, inflate

    @staticmethod
    def _read(path):
        try:
            with open(path, "rb") as f:
                return f.read()
        except OSError:
            raise Exception(f"Problem reading file {path}")         # the reference's words (dataset.py:306-309)

    def read_rgb(self, vid_id, indices):
        """dataset.py:303-305: img_{:010d}.ext per index -> (len(indices), H, W, 3) B, G, R"""
        d = os.path.join(self.root_dir, self.rgb_prefix, vid_id)
        blobs = [self._read(os.path.join(d, "img_{:010d}.{}".format(int(i), self.file_ext))) for i in indices]
        return decode_frames(blobs, gray=False, device=self.device, threads=self.threads, entropy=self.entropy,
                             inflate=self.inflate)

    def read_flow(self, vid_id, indices):
        """dataset.py:355-370: x_{:010d}.ext, y_{:010d}.ext per index, interleaved x, y, x, y ... as _read_flow_frames
        returns them -> (2 * len(indices), H, W, 1)"""
        d = os.path.join(self.root_dir, self.flow_prefix, vid_id)
        blobs = []
        for i in indices:
            for axis in ("x", "y"):
                blobs.append(self._read(os.path.join(d, "{}_{:010d}.{}".format(axis, int(i), self.file_ext))))
        return decode_frames(blobs, gray=True, device=self.device, threads=self.threads, entropy=self.entropy,
                             inflate=self.inflate)
