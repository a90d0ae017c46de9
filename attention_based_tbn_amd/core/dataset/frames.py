"""Frame loading: JPEG files -> uint8 frames on the device, the input of `DevicePipeline` (transform.py).

Reference core/dataset/dataset.py:241-420 reads every frame with cv2.imread on the host (libjpeg-turbo: about 1.6 ms of
one core per 456x256 frame).  Here only the serial half stays on the host -- marker parsing and Huffman decoding, in
worker threads (ctypes releases the GIL) -- and the coefficients cross to the device once, where two kernels do
dequantisation, the IDCT, chroma upsampling and the colour conversion (csrc/jpeg.hip).  The frames are byte-identical
to cv2.imread's: (n, H, W, 3) in B, G, R order, or (n, H, W, 1) for cv2.imread(path, 0).

entropy="device" (opt-in) moves the Huffman decoding to the device as well (csrc/jpeg_entropy.hip: self-synchronising
subsequence decoding, one workgroup per image): the workers only unstuff and pack the scan, and roughly the file's
bytes cross to the device instead of its coefficients.  An image the device decoder flags, or one with more restart
intervals than it has lanes, takes the host stage, so the frames are the same either way."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import torch

from ..._lib import JpegGeometry, TbnHipError, call, lib, ptr, stream_ptr

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
    """what makes two files one `decode_jpegs` batch: (width, height, components, hsamp, vsamp)"""
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


class FrameReader(object):
    """The file layout of reference core/dataset/dataset.py: root_dir/<prefix>/<vid_id>/img_%010d.ext (RGB) and
    x_%010d.ext, y_%010d.ext (Flow).  Both readers return the uint8 device tensor `DevicePipeline.__call__` takes."""

    def __init__(self, root_dir, rgb_prefix, flow_prefix, file_ext="jpg", device="cuda", threads=8, entropy="host"):
        if entropy not in ("host", "device"):
            raise ValueError(f"FrameReader: entropy={entropy!r} is not 'host' or 'device'")
        self.root_dir, self.rgb_prefix, self.flow_prefix, self.file_ext = root_dir, rgb_prefix, flow_prefix, file_ext
        self.device, self.threads, self.entropy = device, threads, entropy

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
        return decode_jpegs(blobs, gray=False, device=self.device, threads=self.threads, entropy=self.entropy)

    def read_flow(self, vid_id, indices):
        """dataset.py:355-370: x_{:010d}.ext, y_{:010d}.ext per index, interleaved x, y, x, y ... as _read_flow_frames
        returns them -> (2 * len(indices), H, W, 1)"""
        d = os.path.join(self.root_dir, self.flow_prefix, vid_id)
        blobs = []
        for i in indices:
            for axis in ("x", "y"):
                blobs.append(self._read(os.path.join(d, "{}_{:010d}.{}".format(axis, int(i), self.file_ext))))
        return decode_jpegs(blobs, gray=True, device=self.device, threads=self.threads, entropy=self.entropy)
