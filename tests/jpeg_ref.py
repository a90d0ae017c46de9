"""numpy restatement of the JPEG reconstruction arithmetic (libjpeg's ISLOW IDCT, fancy upsampling, fixed-point YCbCr ->
BGR) and the helpers the JPEG tests share: the fixture, and the host stage called through ctypes with guard words
round its output buffers.  Everything here is int64 numpy on values that fit 32 bits, so nothing wraps."""
import ctypes as C
import os

import numpy as np

from tests.util import GOLDEN

FIXTURE = os.path.join(GOLDEN, "jpeg_cases.npz")
GUARD = 64           # guard elements on each side of a buffer
COEF_GUARD = 0x5A5A
QUANT_GUARD = 0xA5A5

_cases = None


def cases():
    """the fixture as a dict of arrays, loaded once"""
    global _cases
    if _cases is None:
        with np.load(FIXTURE) as z:
            _cases = {k: z[k] for k in z.files}
    return _cases


def color_names():
    return sorted(k[:-4] for k in cases() if k.endswith(".bgr"))


def gray_names():
    return sorted(k[:-5] for k in cases() if k.endswith(".gray"))


def blob(name):
    return cases()[name + ".jpg"].tobytes()


def golden(name, mode):
    """expected (H, W, C) pixels of a case: mode 'bgr' (3 channels) or 'gray' (1 channel)"""
    z = cases()
    if name + ".bgr" in z:
        return z[name + ".bgr"] if mode == "bgr" else z[name + ".luma"][:, :, None]
    g = z[name + ".gray"]
    return np.repeat(g[:, :, None], 3, 2) if mode == "bgr" else g[:, :, None]


# ---------------------------------------------------------------- host stage through ctypes ---------------------------
def parse(data):
    from attention_based_tbn_amd import _lib
    geo = _lib.JpegGeometry()
    rc = _lib.lib().tbn_jpeg_parse(data, len(data), C.byref(geo))
    return rc, geo, (_lib.lib().tbn_last_error() or b"").decode()


def entropy_decode(data, geo):
    """-> (rc, coef int16 (coef_count,), quant uint16 (components, 64), message); asserts the guard words"""
    from attention_based_tbn_amd import _lib
    n, nq = int(geo.coef_count), geo.components * 64
    coef = np.full(n + 2 * GUARD, COEF_GUARD, np.int16)
    quant = np.full(nq + 2 * GUARD, QUANT_GUARD, np.uint16)
    rc = _lib.lib().tbn_jpeg_entropy_decode(data, len(data), C.byref(geo), coef.ctypes.data + 2 * GUARD,
                                            quant.ctypes.data + 2 * GUARD)
    msg = (_lib.lib().tbn_last_error() or b"").decode() if rc else ""
    assert (coef[:GUARD] == COEF_GUARD).all() and (coef[GUARD + n:] == COEF_GUARD).all(), "write outside coef"
    assert (quant[:GUARD] == QUANT_GUARD).all() and (quant[GUARD + nq:] == QUANT_GUARD).all(), "write outside quant"
    return rc, coef[GUARD:GUARD + n].copy(), quant[GUARD:GUARD + nq].reshape(geo.components, 64).copy(), msg


# ---------------------------------------------------------------- the arithmetic ---------------------------------------
def _idct_1d(x, shift):
    """x: (..., 8) int64 along the last axis"""
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., i] for i in range(8)]
    z1 = (x2 + x6) * 4433
    t2 = z1 - x6 * 15137
    t3 = z1 + x2 * 6270
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = x7, x5, x3, x1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_plane(coef, quant, blocks_h, blocks_w):
    """coef (blocks_h * blocks_w * 64,) quantised, quant (64,) -> uint8 plane (blocks_h * 8, blocks_w * 8)"""
    blk = coef.astype(np.int64).reshape(blocks_h, blocks_w, 8, 8) * quant.astype(np.int64).reshape(8, 8)
    ws = _idct_1d(blk.swapaxes(-1, -2), 11).swapaxes(-1, -2)      # columns first
    px = np.clip(_idct_1d(ws, 18) + 128, 0, 255)                   # then rows
    return px.transpose(0, 2, 1, 3).reshape(blocks_h * 8, blocks_w * 8).astype(np.uint8)


def _h2v1(p):
    p = p.astype(np.int64)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], p.shape[1] * 2), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def _h2v2(p):
    p = p.astype(np.int64)
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    s = np.empty((p.shape[0] * 2, p.shape[1]), np.int64)
    s[0::2] = 3 * p + above
    s[1::2] = 3 * p + below
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], s.shape[1] * 2), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    out[:, 0] = (4 * s[:, 0] + 8) >> 4
    out[:, -1] = (4 * s[:, -1] + 7) >> 4
    return out


def reconstruct(coef, quant, geo, out_channels):
    """coefficients of ONE image in the host stage's layout -> (H, W, out_channels) uint8"""
    W, H, nc = geo.width, geo.height, geo.components
    planes, off = [], 0
    for c in range(nc if out_channels == 3 else 1):
        bh, bw = geo.blocks_h[c], geo.blocks_w[c]
        planes.append(idct_plane(coef[off:off + 64 * bh * bw], quant[c], bh, bw))
        off += 64 * bh * bw
    y = planes[0][:H, :W].astype(np.int64)
    if out_channels == 1:
        return y.astype(np.uint8)[:, :, None]
    if nc == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, 2)
    hs, vs = geo.hsamp[0], geo.vsamp[0]
    cw, ch = -(-W // hs), -(-H // vs)                               # the TRUE downsampled extent
    chroma = []
    for p in planes[1:]:
        p = p[:ch, :cw]
        up = p.astype(np.int64) if hs == 1 else (_h2v1(p) if vs == 1 else _h2v2(p))
        chroma.append(up[:H, :W] - 128)
    cb, cr = chroma
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)
