"""Whole .agmv sequences from and to frames in GPU memory: ctypes calls of AGMV_EncodeFramesDev / AGMV_DecodeFramesDev
(include/agmv.h, libagmv.so).  No logic here: the schedules, the container and both LZ stages are the library's; torch holds
the frames.  The frames live on the library's own device (env AGMV_DEVICE, default 0)."""
import ctypes as C
import os

from .hip import HERE, HipUnavailable

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
        _lib = L
    return _lib


def _device():
    return "cuda:%d" % int(os.environ.get("AGMV_DEVICE", "0"))


def encode_frames(path, frames, fps=24, opt=3, quality=3, compression=1, schedule=SCHEDULE_PDIFS):
    """frames: contiguous int32 / uint32 CUDA tensor [n, h, w] of 0x00RRGGBB on the library's device -> the file at `path`"""
    import torch
    if not (frames.is_cuda and frames.dim() == 3 and frames.element_size() == 4 and not frames.dtype.is_floating_point and
            frames.is_contiguous() and frames.device == torch.device(_device())):
        raise ValueError("encode_frames: a contiguous int32/uint32 tensor [n, h, w] on %s is needed, got %s %s on %s"
                         % (_device(), frames.dtype, tuple(frames.shape), frames.device))
    n, h, w = frames.shape
    torch.cuda.synchronize(frames.device)          # the library works on streams of its own
    rc = load_library().AGMV_EncodeFramesDev(os.fsencode(path), frames.data_ptr(), n, w, h, fps, opt, quality, compression, schedule)
    if rc:
        raise ValueError("AGMV_EncodeFramesDev refused its arguments (%d): %d frames of %dx%d, opt %d, schedule %d" % (rc, n, w, h, opt, schedule))


def decode_frames(path):
    """-> (int32 CUDA tensor [n, h, w] of 0x00RRGGBB on the library's device, AGMV_INFO of the header)"""
    import torch
    L = load_library()
    info = AGMV_INFO()
    rc = L.AGMV_DecodeFramesDev(os.fsencode(path), None, 0, C.byref(info))
    if rc < 0:
        raise RuntimeError("AGMV_DecodeFramesDev(%s): Error %d" % (path, -rc))
    out = torch.empty((info.number_of_frames, info.height, info.width), dtype=torch.int32, device=_device())
    rc = L.AGMV_DecodeFramesDev(os.fsencode(path), out.data_ptr(), info.number_of_frames, None)
    if rc < 0:
        raise RuntimeError("AGMV_DecodeFramesDev(%s): Error %d" % (path, -rc))
    return out[:rc], info
