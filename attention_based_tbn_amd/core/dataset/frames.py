"""Frame loading: JPEG files -> uint8 frames on the device, the input of `DevicePipeline` (transform.py).

Reference core/dataset/dataset.py:241-420 reads every frame with cv2.imread on the host (libjpeg-turbo: about 1.6 ms of
one core per 456x256 frame).  Here only the serial half stays on the host -- marker parsing and Huffman decoding, in
worker threads (ctypes releases the GIL) -- and the coefficients cross to the device once, where two kernels do
dequantisation, the IDCT, chroma upsampling and the colour conversion (csrc/jpeg.hip).  The frames are byte-identical
to cv2.imread's: (n, H, W, 3) in B, G, R order, or (n, H, W, 1) for cv2.imread(path, 0)."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import torch

from ..._lib import JpegGeometry, TbnHipError, call, lib, ptr, stream_ptr

MAX_THREADS = 16      # what one job gets on a shared GPU host; never derived from the machine's core count

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


def decode_jpegs(blobs, gray=False, device="cuda", threads=8):
    """list of `bytes` (baseline JPEG files of ONE geometry) -> uint8 (n, H, W, 1 if gray else 3) on `device`.

    Each blob is parsed once; the entropy decoding runs in `threads` (at most 16) workers into one pinned staging
    tensor; one asynchronous copy and one tbn_jpeg_reconstruct follow on the current stream."""
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


class FrameReader(object):
    """The file layout of reference core/dataset/dataset.py: root_dir/<prefix>/<vid_id>/img_%010d.ext (RGB) and
    x_%010d.ext, y_%010d.ext (Flow).  Both readers return the uint8 device tensor `DevicePipeline.__call__` takes."""

    def __init__(self, root_dir, rgb_prefix, flow_prefix, file_ext="jpg", device="cuda", threads=8):
        self.root_dir, self.rgb_prefix, self.flow_prefix, self.file_ext = root_dir, rgb_prefix, flow_prefix, file_ext
        self.device, self.threads = device, threads

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
        return decode_jpegs(blobs, gray=False, device=self.device, threads=self.threads)

    def read_flow(self, vid_id, indices):
        """dataset.py:355-370: x_{:010d}.ext, y_{:010d}.ext per index, interleaved x, y, x, y ... as _read_flow_frames
        returns them -> (2 * len(indices), H, W, 1)"""
        d = os.path.join(self.root_dir, self.flow_prefix, vid_id)
        blobs = []
        for i in indices:
            for axis in ("x", "y"):
                blobs.append(self._read(os.path.join(d, "{}_{:010d}.{}".format(axis, int(i), self.file_ext))))
        return decode_jpegs(blobs, gray=True, device=self.device, threads=self.threads)
