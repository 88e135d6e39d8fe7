"""The five pixel layouts (AGMV_PIXFMT of include/agmv.h) stated in numpy, for tests/test_pixfmt_cpu.py,
tests/test_gpu_pixfmt.py and tests/test_gpu_pixfmt_files.py.  Packed pixels are uint32 0x00RRGGBB, shape [n, npx]; a clip in a
byte format is uint8 [n, frame bytes]."""
import numpy as np

XRGB32, RGB24, BGR24, RGBA32, RGB8P = 1, 2, 3, 4, 5
NAMES = {XRGB32: "xrgb32", RGB24: "rgb24", BGR24: "bgr24", RGBA32: "rgba32", RGB8P: "rgb8p"}
NEW = (RGB24, BGR24, RGBA32, RGB8P)
BYTES_PER_PIXEL = {XRGB32: 4, RGB24: 3, BGR24: 3, RGBA32: 4, RGB8P: 3}

# one pixel, 0x00112233 (R 0x11, G 0x22, B 0x33), as its bytes lie in memory in each layout -- written out by hand
ONE_PIXEL = {XRGB32: bytes([0x33, 0x22, 0x11, 0x00]), RGB24: bytes([0x11, 0x22, 0x33]), BGR24: bytes([0x33, 0x22, 0x11]),
             RGBA32: bytes([0x11, 0x22, 0x33, 0xFF]), RGB8P: bytes([0x11, 0x22, 0x33])}


def frame_bytes(fmt, npx):
    return BYTES_PER_PIXEL[fmt] * npx


def from_packed(fmt, pix, alpha=None):
    """pix uint32 [n, npx] -> uint8 [n, frame_bytes]; alpha: uint8 [n, npx] for RGBA32 (default 0xFF)"""
    pix = np.asarray(pix, np.uint32)
    n, npx = pix.shape
    r, g, b = ((pix >> 16) & 255).astype(np.uint8), ((pix >> 8) & 255).astype(np.uint8), (pix & 255).astype(np.uint8)
    if fmt == XRGB32:
        return np.ascontiguousarray(pix & 0xFFFFFF).view(np.uint8).reshape(n, 4 * npx)
    if fmt == RGB24:
        return np.stack([r, g, b], axis=2).reshape(n, 3 * npx)
    if fmt == BGR24:
        return np.stack([b, g, r], axis=2).reshape(n, 3 * npx)
    if fmt == RGBA32:
        a = np.full((n, npx), 0xFF, np.uint8) if alpha is None else alpha
        return np.stack([r, g, b, a], axis=2).reshape(n, 4 * npx)
    assert fmt == RGB8P
    return np.stack([r, g, b], axis=1).reshape(n, 3 * npx)


def to_packed(fmt, raw, npx):
    """uint8 [n, frame_bytes] -> (uint32 [n, npx] 0x00RRGGBB, alpha uint8 [n, npx] or None)"""
    raw = np.asarray(raw, np.uint8)
    n = raw.shape[0]
    alpha = None
    if fmt == XRGB32:
        return np.ascontiguousarray(raw).view(np.uint32).reshape(n, npx) & 0xFFFFFF, None
    if fmt == RGB8P:
        c = raw.reshape(n, 3, npx).astype(np.uint32)
        r, g, b = c[:, 0], c[:, 1], c[:, 2]
    else:
        c = raw.reshape(n, npx, BYTES_PER_PIXEL[fmt]).astype(np.uint32)
        r, g, b = (c[..., 2], c[..., 1], c[..., 0]) if fmt == BGR24 else (c[..., 0], c[..., 1], c[..., 2])
        if fmt == RGBA32:
            alpha = c[..., 3].astype(np.uint8)
    return r << 16 | g << 8 | b, alpha
