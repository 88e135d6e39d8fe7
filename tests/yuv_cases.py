"""8-bit YUV 4:2:0 (AGMV_PIXFMT_NV12 / AGMV_PIXFMT_I420 of include/agmv.h) stated in numpy from the tables of that header, for
tests/test_yuv_cpu.py, tests/test_gpu_yuv.py and tests/test_gpu_yuv_files.py.  Packed pixels are uint32 0x00RRGGBB, shape
[n, h, w]; a YUV clip is uint8 [n, frame bytes].  Everything is integer arithmetic in int32, `>>` an arithmetic shift."""
import numpy as np

NV12, I420 = 16, 17
BT709, FULL_RANGE = 0x100, 0x200
NAMES = {NV12: "nv12", I420: "i420"}
LAYOUTS = (NV12, I420)
FLAGS = (0, BT709, FULL_RANGE, BT709 | FULL_RANGE)
FLAG_NAMES = {0: "bt601", BT709: "bt709", FULL_RANGE: "bt601full", BT709 | FULL_RANGE: "bt709full"}

# reading: ky yo rv gu gv bu
READ = {0: (298, 16, 409, 100, 208, 516),
        BT709: (298, 16, 459, 55, 136, 541),
        FULL_RANGE: (256, 0, 359, 88, 183, 454),
        BT709 | FULL_RANGE: (256, 0, 403, 48, 120, 475)}
# writing: (yr yg yb) yo (ur ug ub) (vr vg vb)
WRITE = {0: ((66, 129, 25), 16, (-38, -74, 112), (112, -94, -18)),
         BT709: ((47, 157, 16), 16, (-26, -86, 112), (112, -102, -10)),
         FULL_RANGE: ((77, 150, 29), 0, (-43, -85, 128), (128, -107, -21)),
         BT709 | FULL_RANGE: ((54, 183, 19), 0, (-29, -99, 128), (128, -116, -12))}


def chroma_size(w, h):
    return (w + 1) // 2, (h + 1) // 2


def frame_bytes(fmt, w, h):
    if fmt & ~0x3FF or (fmt & 0xFF) not in LAYOUTS:
        return 0
    cw, ch = chroma_size(w, h)
    return w * h + 2 * cw * ch


def clip8(a):
    return np.clip(a, 0, 255)


def yuv_to_rgb(flags, y, u, v):
    """arrays of Y, U, V (any equal shape) -> uint32 0x00RRGGBB"""
    ky, yo, rv, gu, gv, bu = READ[flags]
    c = ky * (y.astype(np.int32) - yo)
    d, e = u.astype(np.int32) - 128, v.astype(np.int32) - 128
    r = clip8((c + rv * e + 128) >> 8)
    g = clip8((c - gu * d - gv * e + 128) >> 8)
    b = clip8((c + bu * d + 128) >> 8)
    return (r << 16 | g << 8 | b).astype(np.uint32)


def planes(fmt, raw, w, h):
    """uint8 [n, frame_bytes] -> Y [n, h, w], U [n, ch, cw], V [n, ch, cw]"""
    raw = np.asarray(raw, np.uint8)
    n = raw.shape[0]
    cw, ch = chroma_size(w, h)
    y = raw[:, :w * h].reshape(n, h, w)
    if fmt & 0xFF == NV12:
        uv = raw[:, w * h:].reshape(n, ch, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    return y, raw[:, w * h:w * h + cw * ch].reshape(n, ch, cw), raw[:, w * h + cw * ch:].reshape(n, ch, cw)


def to_packed(fmt, raw, w, h):
    """uint8 [n, frame_bytes] -> uint32 [n, h, w]: pixel (x, y) takes Y at (x, y) and U, V at (x >> 1, y >> 1)"""
    y, u, v = planes(fmt, raw, w, h)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)[:, :h, :w]
    return yuv_to_rgb(fmt & 0x300, y, up(u), up(v))


def from_packed(fmt, pix, w, h):
    """uint32 [n, h, w] (bits >= 24 ignored) -> uint8 [n, frame_bytes]"""
    pix = np.asarray(pix, np.uint32).reshape(-1, h, w)
    n = pix.shape[0]
    (yr, yg, yb), yo, cu, cv = WRITE[fmt & 0x300]
    rgb = [((pix >> s) & 255).astype(np.int32) for s in (16, 8, 0)]
    y = clip8(((yr * rgb[0] + yg * rgb[1] + yb * rgb[2] + 128) >> 8) + yo).astype(np.uint8)
    cw, ch = chroma_size(w, h)
    cnt = np.zeros((ch, cw), np.int32)
    sums = [np.zeros((n, ch, cw), np.int32) for _ in range(3)]
    for dy in (0, 1):
        for dx in (0, 1):
            hh, ww = len(range(dy, h, 2)), len(range(dx, w, 2))           # the blocks whose pixel (dx, dy) exists
            cnt[:hh, :ww] += 1
            for s, c in zip(sums, rgb):
                s[:, :hh, :ww] += c[:, dy::2, dx::2]
    assert set(np.unique(cnt)) <= {1, 2, 4}
    mean = [(s + (cnt >> 1)) // cnt for s in sums]
    u = clip8(((cu[0] * mean[0] + cu[1] * mean[1] + cu[2] * mean[2] + 128) >> 8) + 128).astype(np.uint8)
    v = clip8(((cv[0] * mean[0] + cv[1] * mean[1] + cv[2] * mean[2] + 128) >> 8) + 128).astype(np.uint8)
    out = np.empty((n, frame_bytes(fmt, w, h)), np.uint8)
    out[:, :w * h] = y.reshape(n, -1)
    if fmt & 0xFF == NV12:
        out[:, w * h:] = np.stack([u, v], axis=3).reshape(n, -1)
    else:
        out[:, w * h:w * h + cw * ch] = u.reshape(n, -1)
        out[:, w * h + cw * ch:] = v.reshape(n, -1)
    return out
