"""Normalised float tensor clips (AGMV_TENSORFMT of include/agmv.h) stated in numpy: the writing table, the three conversions and
the reading rule.  Elements travel as their bit patterns -- uint32 for F32, uint16 for F16 and BF16 -- so that every comparison
is one of bits (NaNs included).  A tensor clip is [n, 3, h, w]; the packed clips are uint32 [n, h, w] of 0x00RRGGBB."""
import numpy as np

F32, F16, BF16 = 1, 2, 3
TYPES = (F32, F16, BF16)
NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}

# (mean, std): what the tests share
NORMS = {"identity": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
         "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
         "half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
         "bytes": ((0.0, 0.0, 0.0), (1.0 / 255, 1.0 / 255, 1.0 / 255))}


def f32(x):
    """the float (or three floats) as the C `float` the library receives"""
    return np.asarray(x, np.float32)


def narrow(t, x):
    """float32 array -> the bit patterns of type t, rounded to nearest-even, overflow = infinity"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    if t == F32:
        return u.copy()
    if t == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = u.astype(np.uint64)                                        # BF16 by the integer rule
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(t, bits):
    """bit patterns of type t -> the float32 of the same value (exact)"""
    bits = np.ascontiguousarray(bits, BITS[t])
    if t == F32:
        return bits.view(np.float32)
    if t == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def table(t, mean, std):
    """T[c][v] as bit patterns [3, 256]: the float32 nearest to the double (v / 255 - mean[c]) / std[c], narrowed"""
    m, s = f32(mean).astype(np.float64), f32(std).astype(np.float64)
    v = np.arange(256, dtype=np.float64)
    return narrow(t, ((v[None, :] / 255.0 - m[:, None]) / s[:, None]).astype(np.float32))


def coefficients(mean, std):
    """a[3], b[3] as float32"""
    return (255.0 * f32(std).astype(np.float64)).astype(np.float32), (255.0 * f32(mean).astype(np.float64)).astype(np.float32)


def _ftz(x):
    """float32 subnormals flushed to a zero of their sign"""
    u = x.view(np.uint32)
    return np.where((u & 0x7F800000) == 0, u & 0x80000000, u).astype(np.uint32).view(np.float32)


def read_channel(x, a, b, ftz=False):
    """float32 array x of one channel, float32 scalars a, b -> the byte: two separately rounded operations, NaN = 0, half to even.
    ftz: every input and intermediate result passes through a flush of subnormals, as a device that flushes would compute"""
    x, a, b = np.ascontiguousarray(x, np.float32), np.float32(a), np.float32(b)
    with np.errstate(all="ignore"):
        if ftz:
            x, a, b = _ftz(x), _ftz(np.array([a]))[0], _ftz(np.array([b]))[0]
            p = _ftz(np.ascontiguousarray(x * a, np.float32))
            t = _ftz(np.ascontiguousarray(p + b, np.float32))
        else:
            p = (x * a).astype(np.float32)
            t = (p + b).astype(np.float32)
        v = np.rint(np.minimum(np.maximum(np.where(np.isnan(t), np.float32(0), t), np.float32(0)), np.float32(255)))
    return v.astype(np.uint32)


def to_packed(t, bits, mean, std, ftz=False):
    """a tensor clip, bit patterns [n, 3, h, w] -> uint32 [n, h, w] of 0x00RRGGBB by the reading rule"""
    a, b = coefficients(mean, std)
    x = widen(t, bits)
    r, g, bl = (read_channel(x[:, c], a[c], b[c], ftz) for c in range(3))
    return r << 16 | g << 8 | bl


def from_packed(tab, pix):
    """uint32 [n, h, w] (bits >= 24 ignored) -> the tensor clip's bit patterns [n, 3, h, w] through the table [3, 256]"""
    pix = np.asarray(pix, np.uint32)
    return np.stack([tab[0][(pix >> 16) & 255], tab[1][(pix >> 8) & 255], tab[2][pix & 255]], axis=1)
