"""Whole .agmv sequences from and to frames in GPU memory: ctypes calls of AGMV_EncodeFramesFmtDev / AGMV_DecodeFramesFmtDev
(include/agmv.h, libagmv.so).  No logic here: the schedules, the container, both LZ stages and the reading and writing of the
caller's pixel layout are the library's; torch holds the frames.  The frames live on the library's own device (env AGMV_DEVICE,
default 0).

Pixel layouts (AGMV_PIXFMT) and the tensors that hold n frames of h x w:
  "xrgb32"  int32 / uint32 [n, h, w]   0x00RRGGBB
  "rgb24"   uint8 [n, h, w, 3]         R, G, B     (video readers)
  "bgr24"   uint8 [n, h, w, 3]         B, G, R     (OpenCV)
  "rgba32"  uint8 [n, h, w, 4]         R, G, B, A  (image decoders; A is ignored on input and 0xFF on output)
  "rgb8p"   uint8 [n, 3, h, w]         planes R, G, B (models)"""
import ctypes as C
import os

from .hip import HERE, PIXFMT, HipUnavailable, pixfmt

SCHEDULE_FULL, SCHEDULE_PDIFS, SCHEDULE_ADAPTIVE = 1, 2, 3


class AGMV_INFO(C.Structure):
    # include/agmv.h (u32 is `unsigned long` there)
    _fields_ = [("width", C.c_ulong), ("height", C.c_ulong), ("number_of_frames", C.c_ulong), ("version", C.c_ubyte),
                ("total_audio_duration", C.c_ulong), ("sample_rate", C.c_ulong), ("audio_size", C.c_ulong),
                ("number_of_channels", C.c_ushort), ("bits_per_sample", C.c_ushort)]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (torch's HIP runtime first, as in hip.load_library)
        p = os.path.join(HERE, "libagmv.so")
        if not os.path.exists(p):
            raise HipUnavailable("%s is missing: run `python -m libagmv_amd.build`; the AGMV hot path has no CPU fallback" % p)
        L = C.CDLL(p)
        L.AGMV_EncodeFramesDev.restype = C.c_int
        L.AGMV_EncodeFramesDev.argtypes = [C.c_char_p, C.c_void_p] + [C.c_ulong] * 4 + [C.c_int] * 4
        L.AGMV_DecodeFramesDev.restype = C.c_int
        L.AGMV_DecodeFramesDev.argtypes = [C.c_char_p, C.c_void_p, C.c_ulong, C.POINTER(AGMV_INFO)]
        L.AGMV_EncodeFramesFmtDev.restype = C.c_int
        L.AGMV_EncodeFramesFmtDev.argtypes = [C.c_char_p, C.c_void_p, C.c_int] + [C.c_ulong] * 4 + [C.c_int] * 4
        L.AGMV_DecodeFramesFmtDev.restype = C.c_int
        L.AGMV_DecodeFramesFmtDev.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_ulong, C.POINTER(AGMV_INFO)]
        _lib = L
    return _lib


def _device():
    return "cuda:%d" % int(os.environ.get("AGMV_DEVICE", "0"))


def _clip_geometry(frames, fmt):
    """(AGMV_PIXFMT value, n, h, w) of a tensor of frames; fmt None = inferred from dtype and shape.  Raises ValueError naming
    `fmt` for a tensor that holds no clip of that layout; touches neither the library nor the device."""
    import torch
    shape, packed = tuple(frames.shape), frames.element_size() == 4 and not frames.dtype.is_floating_point and not frames.dtype.is_complex
    if fmt is None:
        fits = []
        if packed and len(shape) == 3:
            fits.append("xrgb32")
        if frames.dtype == torch.uint8 and len(shape) == 4:
            fits += [name for name, ok in (("rgb24", shape[3] == 3), ("rgba32", shape[3] == 4), ("rgb8p", shape[1] == 3)) if ok]
        if len(fits) != 1:
            raise ValueError("encode_frames: fmt cannot be inferred from a %s tensor of shape %s (%s): pass fmt=" %
                             (frames.dtype, shape, "it fits " + " and ".join(fits) if fits else "int32/uint32 [n,h,w], uint8 [n,h,w,3|4] or uint8 [n,3,h,w] is needed"))
        fmt = fits[0]
    v = pixfmt(fmt)
    ok = (packed and len(shape) == 3) if v == 1 else (frames.dtype == torch.uint8 and len(shape) == 4 and
                                                      (shape[1] == 3 if v == 5 else shape[3] == (4 if v == 4 else 3)))
    if not ok:
        raise ValueError("encode_frames: fmt %r does not fit a %s tensor of shape %s" % (fmt, frames.dtype, shape))
    if not frames.is_contiguous():
        raise ValueError("encode_frames: fmt %r needs a contiguous tensor (strides %s of shape %s)" % (fmt, frames.stride(), shape))
    n, h, w = (shape[0], shape[2], shape[3]) if v == 5 else shape[:3]
    return v, n, h, w


def encode_frames(path, frames, fps=24, opt=3, quality=3, compression=1, schedule=SCHEDULE_PDIFS, fmt=None):
    """frames: contiguous CUDA tensor of n frames on the library's device, in the layout `fmt` (see the module text; None = inferred
    from the tensor) -> the file at `path`"""
    import torch
    v, n, h, w = _clip_geometry(frames, fmt)
    if not (frames.is_cuda and frames.device == torch.device(_device())):
        raise ValueError("encode_frames: the frames must be on %s, got %s" % (_device(), frames.device))
    torch.cuda.synchronize(frames.device)          # the library works on streams of its own
    rc = load_library().AGMV_EncodeFramesFmtDev(os.fsencode(path), frames.data_ptr(), v, n, w, h, fps, opt, quality, compression, schedule)
    if rc:
        raise ValueError("AGMV_EncodeFramesFmtDev refused its arguments (%d): %d frames of %dx%d, opt %d, schedule %d" % (rc, n, w, h, opt, schedule))


def decode_frames(path, fmt="xrgb32"):
    """-> (CUDA tensor of the file's frames on the library's device in the layout `fmt`: int32 [n, h, w] of 0x00RRGGBB for "xrgb32",
    uint8 [n, h, w, 3] / [n, h, w, 4] / [n, 3, h, w] for the byte formats; AGMV_INFO of the header)"""
    import torch
    v = pixfmt(fmt)
    L = load_library()
    info = AGMV_INFO()
    rc = L.AGMV_DecodeFramesFmtDev(os.fsencode(path), None, v, 0, C.byref(info))
    if rc < 0:
        raise RuntimeError("AGMV_DecodeFramesFmtDev(%s): Error %d" % (path, -rc))
    n, h, w = info.number_of_frames, info.height, info.width
    shape = {1: (n, h, w), 2: (n, h, w, 3), 3: (n, h, w, 3), 4: (n, h, w, 4), 5: (n, 3, h, w)}[v]
    out = torch.empty(shape, dtype=torch.int32 if v == 1 else torch.uint8, device=_device())
    rc = L.AGMV_DecodeFramesFmtDev(os.fsencode(path), out.data_ptr(), v, n, None)
    if rc < 0:
        raise RuntimeError("AGMV_DecodeFramesFmtDev(%s): Error %d" % (path, -rc))
    return out[:rc], info
