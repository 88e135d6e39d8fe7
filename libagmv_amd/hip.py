"""ctypes binding of include/agmv_hip.h (the signatures are abi.HIP), include/agmv_hip_view.h (abi.HIP_VIEW),
include/agmv_hip_view_source.h (abi.HIP_VIEW_SOURCE), include/agmv_hip_stabilise.h (abi.HIP_STABILISE),
include/agmv_hip_deblock.h (abi.HIP_DEBLOCK) and include/agmv_hip_time.h (abi.HIP_TIME).

The product is the shared library; this module only marshals pointers.  torch is used for
device memory and streams (plumbing).  Every failure is loud: a missing library raises
HipUnavailable at load time, a failing call raises RuntimeError with the library's message.
"""
import ctypes as C
import os

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))

# every symbol include/agmv_hip.h declares (tests check the built library exports them all)
ABI_SYMBOLS = list(abi.HIP)


class HipUnavailable(RuntimeError):
    pass


def lib_path():
    # AGMV_HIP_LIB: tools/ablate.sh points the probe at instrumented builds of the same source
    return os.environ.get("AGMV_HIP_LIB") or os.path.join(HERE, "libagmv_hip.so")


_libs = {}


def load_library(path=None):
    """dlopen libagmv_hip.so (built in-tree by libagmv_amd/build.py). No fallback.
    `path` selects another build of the same source (tools/probe_multi.py times several in one process)."""
    p = path or lib_path()
    if p in _libs:
        return _libs[p]
    if not os.path.exists(p):
        raise HipUnavailable("%s is missing: run `python -m libagmv_amd.build` (or "
                             "__graft_entry__.build()); the AGMV hot path has no CPU fallback" % p)
    # PyTorch ships its own copies of the HIP / HSA runtimes.  This module works on torch device tensors, so torch's runtime is
    # loaded FIRST: with libagmv_hip.so (linked against /opt/rocm) in the process before `import torch`, the two resolve against
    # each other's libraries and hipGetDeviceCount then reports no device (seen with build() followed by smoke() in one process).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        L = C.CDLL(p)
    except OSError as e:
        raise HipUnavailable("cannot load %s: %s" % (p, e))
    # only an explicitly named other build of the same source may lack symbols; the default library has them all
    abi.bind(L, abi.HIP, missing_ok=path is not None)
    abi.bind(L, abi.HIP_VIEW, missing_ok=path is not None)
    abi.bind(L, abi.HIP_VIEW_SOURCE, missing_ok=path is not None)
    abi.bind(L, abi.HIP_STABILISE, missing_ok=path is not None)
    abi.bind(L, abi.HIP_DEBLOCK, missing_ok=path is not None)
    abi.bind(L, abi.HIP_TIME, missing_ok=path is not None)
    _libs[p] = L
    return L


# AGMV_PIXFMT of include/agmv.h: name -> value
PIXFMT = {"xrgb32": 1, "rgb24": 2, "bgr24": 3, "rgba32": 4, "rgb8p": 5}


def pixfmt(fmt):
    """the AGMV_PIXFMT value of a name or of a value"""
    v = PIXFMT.get(fmt, fmt)
    if v not in PIXFMT.values():
        raise ValueError("fmt: one of %s is needed, got %r" % (", ".join(sorted(PIXFMT)), fmt))
    return v


# the YUV 4:2:0 formats of include/agmv.h and the flags that are OR-ed into them (PIXFMT and pixfmt() stay the five RGB layouts)
YUVFMT = {"nv12": 16, "i420": 17}
YUV_BT709, YUV_FULL_RANGE = 0x100, 0x200


def yuvfmt(fmt, yuv=None, full_range=False):
    """the fmt argument of the agmv_hip_yuv_* functions: a name of YUVFMT with yuv "bt601" (default) / "bt709" and full_range, or
    such a value itself (then yuv and full_range must be left alone)"""
    if fmt in YUVFMT:
        if yuv not in (None, "bt601", "bt709"):
            raise ValueError("yuv: \"bt601\" or \"bt709\" is needed, got %r" % (yuv,))
        return YUVFMT[fmt] | (YUV_BT709 if yuv == "bt709" else 0) | (YUV_FULL_RANGE if full_range else 0)
    if isinstance(fmt, int) and (fmt & 0xFF) in YUVFMT.values() and not fmt & ~0x3FF and yuv is None and not full_range:
        return fmt
    raise ValueError("fmt: one of %s (or its value with flags) is needed, got %r" % (", ".join(sorted(YUVFMT)), fmt))


# AGMV_TIME of include/agmv.h: name -> value
TIME = {"nearest": 1, "area": 2}

# AGMV_PCMFMT of include/agmv.h: name -> value
PCMFMT = {"s16": 1, "u8": 2, "f32p": 3}


def pcmfmt(fmt):
    """the AGMV_PCMFMT value of a name or of a value"""
    v = PCMFMT.get(fmt, fmt)
    if v not in PCMFMT.values():
        raise ValueError("fmt: one of %s is needed, got %r" % (", ".join(sorted(PCMFMT)), fmt))
    return v


# AGMV_TENSORFMT of include/agmv.h: name -> value; the numpy storage of one element's bit pattern
TENSORFMT = {"f32": 1, "f16": 2, "bf16": 3}
TENSOR_BITS = {1: np.uint32, 2: np.uint16, 3: np.uint16}


def tensorfmt(fmt):
    """the AGMV_TENSORFMT value of a name or of a value"""
    v = TENSORFMT.get(fmt, fmt) if isinstance(fmt, (str, int)) and not isinstance(fmt, bool) else None
    if v not in TENSORFMT.values():
        raise ValueError("fmt: one of %s is needed, got %r" % (", ".join(sorted(TENSORFMT)), fmt))
    return v


def tensor_normalisation(who, mean, std):
    """(mean, std) as two ctypes float[3]; a number stands for all three channels.  Raises ValueError for anything else; the
    bounds are the library's to check"""
    out = []
    for name, v in (("mean", mean), ("std", std)):
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            v = (v, v, v)
        if not (isinstance(v, (tuple, list)) and len(v) == 3 and all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v)):
            raise ValueError("%s: %s must be a number or three numbers, got %r" % (who, name, v))
        out.append((C.c_float * 3)(*[float(np.float32(x)) for x in v]))
    return out


def tensor_table(fmt, mean=0.0, std=1.0):
    """agmv_hip_tensor_table: the 3 x 256 bit patterns of the writing rule as a numpy array [3, 256] of uint32 ("f32") or uint16;
    host only, no GPU.  ValueError for a normalisation the library refuses."""
    v = tensorfmt(fmt)
    m, s = tensor_normalisation("tensor_table", mean, std)
    table = np.zeros((3, 256), dtype=TENSOR_BITS[v])
    if load_library().agmv_hip_tensor_table(v, m, s, _np_ptr(table)):
        raise ValueError("tensor_table: mean %r / std %r: %s" % (mean, std, load_library().agmv_hip_last_error().decode()))
    return table


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# the C-ABI sees a pointer and a row stride: a tensor of another dtype or layout would be read as other bytes, without an error
def _check_rows(name, t, n):
    import torch
    if not (t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= n):
        raise ValueError("%s: a CUDA uint8 tensor [>= %d, stride] with unit inner stride is needed, got %s %s strides %s on %s"
                         % (name, n, t.dtype, tuple(t.shape), t.stride(), t.device))


def _check_vec(name, t, n):
    import torch
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n):
        raise ValueError("%s: a contiguous CUDA int32 tensor of >= %d entries is needed, got %s %s strides %s on %s"
                         % (name, n, t.dtype, tuple(t.shape), t.stride(), t.device))


class AgmvHip:
    """One context = one GPU + one palette.  Device-resident calls take torch CUDA tensors
    (uint8 / int16 / int32 storage: torch has no unsigned 16/32-bit arithmetic types, the bytes
    are what matters) and run on torch's current stream."""

    def __init__(self, device=0, lib=None):
        self.L = load_library(lib)
        self.ctx = self.L.agmv_hip_create(int(device))
        if not self.ctx:
            raise HipUnavailable(self.L.agmv_hip_last_error().decode())
        self.device = int(device)
        self.mode512 = None

    def close(self):
        if getattr(self, "ctx", None):
            self.L.agmv_hip_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    # ------------------------------------------------------------------ helpers
    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.agmv_hip_last_error().decode())

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def max_usize(self, w, h):
        return self.L.agmv_hip_max_usize(w, h, int(self.mode512))

    def set_palette(self, p0, p1, mode512=True):
        p0 = np.ascontiguousarray(p0, np.uint32)
        p1 = np.ascontiguousarray(p1, np.uint32) if p1 is not None else np.zeros(256, np.uint32)
        self.mode512 = bool(mode512)
        self._ck(self.L.agmv_hip_set_palette(self.ctx, _np_ptr(p0), _np_ptr(p1), int(mode512), self._stream()))

    def enable_timing(self, on=True):
        self._ck(self.L.agmv_hip_enable_timing(self.ctx, int(on)))

    def last_kernel_ms(self, which):
        return float(self.L.agmv_hip_last_kernel_ms(self.ctx, which))

    def check(self):
        self._ck(self.L.agmv_hip_check(self.ctx, self._stream()))

    # ------------------------------------------------------------------ device-resident path
    def quantise_dev(self, pix):
        import torch
        out = torch.empty(pix.numel(), dtype=torch.int16, device=pix.device)
        self._ck(self.L.agmv_hip_quantise_dev(self.ctx, pix.data_ptr(), pix.numel(), out.data_ptr(), self._stream()))
        return out

    def encode_dev(self, pix, n_frames, w, h, first_frame_count=0, out=None, sizes=None, ientries=None):
        """pix: int32 CUDA tensor of n_frames*w*h pixels. Returns (out u8 [n, stride], sizes i32 [n])."""
        import torch
        stride = self.max_usize(w, h)
        if out is None:
            out = torch.empty((n_frames, stride), dtype=torch.uint8, device=pix.device)
        if sizes is None:
            sizes = torch.empty(n_frames, dtype=torch.int32, device=pix.device)
        self._ck(self.L.agmv_hip_encode_frames_dev(
            self.ctx, pix.data_ptr(), n_frames, w, h, first_frame_count, out.data_ptr(), out.stride(0),
            sizes.data_ptr(), ientries.data_ptr() if ientries is not None else None, self._stream()))
        return out, sizes

    def encode_entries_host(self, entries, first_frame_count=0, ientries=None):
        """entries: uint32 ndarray [n, h, w] of pal_num << 8 | index. Returns the per-frame bitstreams."""
        entries = np.ascontiguousarray(entries, np.uint32)
        n, h, w = entries.shape
        stride = self.max_usize(w, h)
        out = np.zeros((n, stride), np.uint8)
        sizes = np.zeros(n, np.uint32)
        self._ck(self.L.agmv_hip_encode_entries(self.ctx, _np_ptr(entries), n, w, h, first_frame_count,
                                                _np_ptr(out), stride, _np_ptr(sizes), _np_ptr(ientries)))
        return [out[i, :sizes[i]].copy() for i in range(n)]

    def nearest_host(self, p0, p1, pix, mode512=True):
        """exact nearest entries of `pix` against (p0, p1) without building a table"""
        p0 = np.ascontiguousarray(p0, np.uint32)
        p1 = np.ascontiguousarray(p1 if p1 is not None else np.zeros(256), np.uint32)
        pix = np.ascontiguousarray(pix, np.uint32).reshape(-1)
        out = np.zeros(pix.size, np.uint16)
        self._ck(self.L.agmv_hip_nearest(self.ctx, _np_ptr(p0), _np_ptr(p1), int(mode512), _np_ptr(pix), pix.size, _np_ptr(out)))
        return out

    def parse_dev(self, bits, bpos, n_frames, w, h, offsets=None, nentered=None):
        import torch
        nblk = (w // 4) * (h // 4)
        if offsets is None:
            offsets = torch.empty((n_frames, nblk), dtype=torch.int32, device=bits.device)
        if nentered is None:
            nentered = torch.empty(n_frames, dtype=torch.int32, device=bits.device)
        self._ck(self.L.agmv_hip_parse_frames_dev(self.ctx, bits.data_ptr(), bits.stride(0), bpos.data_ptr(),
                                                  n_frames, w, h, offsets.data_ptr(), nentered.data_ptr(),
                                                  self._stream()))
        return offsets, nentered

    def decode_dev(self, bits, bpos, offsets, nentered, n_frames, w, h, first_frame_count=0, out=None,
                   prev=None, prev_iframe=None):
        import torch
        if out is None:
            out = torch.empty((n_frames, h, w), dtype=torch.int32, device=bits.device)
        self._ck(self.L.agmv_hip_decode_frames_dev(
            self.ctx, bits.data_ptr(), bits.stride(0), bpos.data_ptr(), offsets.data_ptr(), nentered.data_ptr(),
            n_frames, w, h, first_frame_count, out.data_ptr(),
            prev.data_ptr() if prev is not None else None,
            prev_iframe.data_ptr() if prev_iframe is not None else None, self._stream()))
        return out

    def pack_frames_dev(self, out, sizes, total=None):
        """slab [n, stride] u8 + sizes [n] i32 (CUDA) -> (packed u8 [sum(sizes)], offsets i64 [n + 1]); `total` = sum(sizes) if the
        caller knows it (otherwise one device -> host read)"""
        import torch
        n = int(sizes.numel())
        if total is None:
            total = int(sizes.sum().item()) if n else 0
        packed = torch.empty(total, dtype=torch.uint8, device=out.device)
        offs = torch.zeros(n + 1, dtype=torch.int64, device=out.device)
        if n and total:                                        # (nothing but empty frames: the offsets are all 0)
            self._ck(self.L.agmv_hip_pack_frames_dev(self.ctx, out.data_ptr(), out.stride(0), sizes.data_ptr(), n,
                                                     packed.data_ptr(), offs.data_ptr(), self._stream()))
        return packed, offs

    def unpack_frames_dev(self, packed, sizes, stride, out=None):
        """the inverse: packed u8 + sizes [n] i32 (CUDA) -> slab [n, stride] u8 (rows zero behind their size unless `out` is given)"""
        import torch
        n = int(sizes.numel())
        if out is None:
            out = torch.zeros((n, stride), dtype=torch.uint8, device=packed.device)
        offs = torch.empty(n + 1, dtype=torch.int64, device=packed.device)
        if n and packed.numel():
            self._ck(self.L.agmv_hip_unpack_frames_dev(self.ctx, packed.data_ptr(), sizes.data_ptr(), n, out.data_ptr(), out.stride(0),
                                                       offs.data_ptr(), self._stream()))
        return out

    def lzss_max_csize(self, n):
        """bytes a payload row must hold for a pre-LZ bitstream of n bytes"""
        return int(self.L.agmv_hip_lzss_max_csize(int(n)))

    def lzss_frames_dev(self, bits, sizes, n_frames, out=None, csize=None):
        """LZSS stage of AGMV_EncodeFrame on the GPU: bits u8 [n, stride] (rows of pre-LZ bitstreams), sizes int32 [n].
        Returns (out u8 [n, out_stride], csize int32 [n]); row f holds the csize[f] payload bytes the reference's file holds.
        Reads the sizes once (synchronises torch's current stream)."""
        import torch
        _check_rows("bits", bits, n_frames)
        _check_vec("sizes", sizes, n_frames)
        if out is None:
            out = torch.empty((n_frames, self.lzss_max_csize(bits.stride(0))), dtype=torch.uint8, device=bits.device)
        if csize is None:
            csize = torch.empty(n_frames, dtype=torch.int32, device=bits.device)
        _check_rows("out", out, n_frames)
        _check_vec("csize", csize, n_frames)
        self._ck(self.L.agmv_hip_lzss_frames_dev(self.ctx, bits.data_ptr(), bits.stride(0), sizes.data_ptr(), n_frames,
                                                 out.data_ptr(), out.stride(0), csize.data_ptr(), self._stream()))
        return out, csize

    def lzss_frames(self, streams):
        """host form: a list of u8 arrays (pre-LZ bitstreams) -> list of payloads (csize bytes each)"""
        streams = [np.ascontiguousarray(x, np.uint8) for x in streams]
        n = len(streams)
        sizes = np.array([len(x) for x in streams], np.uint32)
        stride = max([1] + [len(x) for x in streams])
        ostride = self.lzss_max_csize(stride)
        bits = np.zeros((max(n, 1), stride), np.uint8)
        for i, x in enumerate(streams):
            bits[i, :len(x)] = x
        out = np.zeros((max(n, 1), ostride), np.uint8)
        cs = np.zeros(max(n, 1), np.uint32)
        self._ck(self.L.agmv_hip_lzss_frames(self.ctx, _np_ptr(bits), stride, _np_ptr(sizes), n, _np_ptr(out), ostride,
                                             _np_ptr(cs)))
        return [out[i, :cs[i]].copy() for i in range(n)]

    def lz77_max_csize(self, n):
        """bytes a payload row must hold for a pre-LZ bitstream of n bytes (4 * n)"""
        return int(self.L.agmv_hip_lz77_max_csize(int(n)))

    def lz77_peek_dev(self, bits, sizes, n_frames, persist, peek=None):
        """the byte behind each stream in the reference's persistent bitstream buffer, in frame order: peek[f] =
        persist[sizes[f]] (0 at or behind its end), then persist takes row f.  persist: u8 [persist_len], updated in place.
        Returns peek u8 [n]."""
        import torch
        _check_rows("bits", bits, n_frames)
        _check_vec("sizes", sizes, n_frames)
        if not (persist.is_cuda and persist.dtype == torch.uint8 and persist.dim() == 1 and persist.is_contiguous()):
            raise ValueError("persist: a contiguous 1-D CUDA uint8 tensor is needed, got %s %s on %s"
                             % (persist.dtype, tuple(persist.shape), persist.device))
        if peek is None:
            peek = torch.empty(max(n_frames, 1), dtype=torch.uint8, device=bits.device)
        if not (peek.is_cuda and peek.dtype == torch.uint8 and peek.is_contiguous() and peek.numel() >= n_frames):
            raise ValueError("peek: a contiguous CUDA uint8 tensor of >= %d entries is needed" % n_frames)
        self._ck(self.L.agmv_hip_lz77_peek_dev(self.ctx, bits.data_ptr(), bits.stride(0), sizes.data_ptr(), n_frames,
                                               persist.data_ptr(), persist.numel(), peek.data_ptr(), self._stream()))
        return peek

    def lz77_frames_dev(self, bits, sizes, n_frames, peek=None, out=None, csize=None):
        """LZ77 stage of AGMV_EncodeFrame on the GPU: bits u8 [n, stride] (rows of pre-LZ bitstreams), sizes int32 [n],
        peek u8 [n] or None (zeros): the byte a match that runs to the end of its stream emits.
        Returns (out u8 [n, out_stride], csize int32 [n]); row f holds the csize[f] payload bytes the reference's file holds.
        Reads the sizes once (synchronises torch's current stream)."""
        import torch
        _check_rows("bits", bits, n_frames)
        _check_vec("sizes", sizes, n_frames)
        if peek is not None and not (peek.is_cuda and peek.dtype == torch.uint8 and peek.is_contiguous() and peek.numel() >= n_frames):
            raise ValueError("peek: a contiguous CUDA uint8 tensor of >= %d entries is needed" % n_frames)
        if out is None:
            out = torch.empty((n_frames, max(self.lz77_max_csize(bits.stride(0)), 1)), dtype=torch.uint8, device=bits.device)
        if csize is None:
            csize = torch.empty(n_frames, dtype=torch.int32, device=bits.device)
        _check_rows("out", out, n_frames)
        _check_vec("csize", csize, n_frames)
        self._ck(self.L.agmv_hip_lz77_frames_dev(self.ctx, bits.data_ptr(), bits.stride(0), sizes.data_ptr(), n_frames,
                                                 peek.data_ptr() if peek is not None else None, out.data_ptr(), out.stride(0),
                                                 csize.data_ptr(), self._stream()))
        return out, csize

    def lz77_frames(self, streams, persist=None):
        """host form of lz77_peek_dev + lz77_frames_dev: a list of u8 arrays (pre-LZ bitstreams) -> list of payloads (csize
        bytes each).  persist: the persistent buffer before the call (u8 array, updated in place), None = none (peek 0)."""
        streams = [np.ascontiguousarray(x, np.uint8) for x in streams]
        n = len(streams)
        sizes = np.array([len(x) for x in streams], np.uint32)
        stride = max([1] + [len(x) for x in streams])
        ostride = self.lz77_max_csize(stride)
        bits = np.zeros((max(n, 1), stride), np.uint8)
        for i, x in enumerate(streams):
            bits[i, :len(x)] = x
        out = np.zeros((max(n, 1), ostride), np.uint8)
        cs = np.zeros(max(n, 1), np.uint32)
        if persist is not None and not (isinstance(persist, np.ndarray) and persist.dtype == np.uint8 and persist.flags.c_contiguous):
            raise ValueError("persist: a contiguous uint8 array is needed")
        self._ck(self.L.agmv_hip_lz77_frames(self.ctx, _np_ptr(bits), stride, _np_ptr(sizes), n, _np_ptr(persist),
                                             persist.size if persist is not None else 0, _np_ptr(out), ostride, _np_ptr(cs)))
        return [out[i, :cs[i]].copy() for i in range(n)]

    def lz77_reparsed_segments(self):
        """segments of the last lz77_frames_dev call that were parsed again from their true entry (a statistic)"""
        rc = self.L.agmv_hip_lz77_reparsed_segments(self.ctx, self._stream())
        if rc < 0:
            raise RuntimeError(self.L.agmv_hip_last_error().decode())
        return rc

    def lz_decode_frames_dev(self, version, src, off, avail, usize, csize, n_frames, cap, bits=None, bpos=None, used=None):
        """LZ stage of AGMV_DecodeFrameChunk on the GPU: frame f's payload is src[off[f]:] (u8 [N], off int64 [n]) with
        avail[f] bytes that exist and the chunk's usize[f] / csize[f] (int32 [n]).  Version 1 or 2 is LZSS, any other LZ77.
        Returns (bits u8 [n, stride >= cap], bpos int32 [n], used int32 [n]); row f holds data[0, bpos) of a buffer of cap
        bytes.  Reads avail / usize / csize once (synchronises torch's current stream); given as host numpy arrays instead,
        they go to agmv_hip_lz_decode_frames_sized_dev, which does not synchronise."""
        import torch
        if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous()):
            raise ValueError("src: a contiguous 1-D CUDA uint8 tensor is needed, got %s %s on %s" % (src.dtype, tuple(src.shape), src.device))
        if not (off.is_cuda and off.dtype == torch.int64 and off.is_contiguous() and off.numel() >= n_frames):
            raise ValueError("off: a contiguous CUDA int64 tensor of >= %d entries is needed, got %s %s on %s"
                             % (n_frames, off.dtype, tuple(off.shape), off.device))
        host = [isinstance(t, np.ndarray) for t in (avail, usize, csize)]
        if any(host) and not all(host):
            raise ValueError("avail, usize, csize: all CUDA int32 tensors or all host arrays")
        if all(host):
            sizes = [np.ascontiguousarray(np.asarray(t).astype(np.uint32)) for t in (avail, usize, csize)]
            if any(t.ndim != 1 or t.size < n_frames for t in sizes):
                raise ValueError("avail, usize, csize: 1-D host arrays of >= %d entries are needed" % n_frames)
        else:
            for name, t in (("avail", avail), ("usize", usize), ("csize", csize)):
                _check_vec(name, t, n_frames)
        if bits is None:
            bits = torch.zeros((n_frames, max(int(cap), 1)), dtype=torch.uint8, device=src.device)
        if bpos is None:
            bpos = torch.empty(n_frames, dtype=torch.int32, device=src.device)
        if used is None:
            used = torch.empty(n_frames, dtype=torch.int32, device=src.device)
        _check_rows("bits", bits, n_frames)
        _check_vec("bpos", bpos, n_frames)
        _check_vec("used", used, n_frames)
        if int(cap) > bits.stride(0):
            raise ValueError("cap %d exceeds the row stride %d of bits" % (cap, bits.stride(0)))
        if all(host):
            self._ck(self.L.agmv_hip_lz_decode_frames_sized_dev(self.ctx, int(version), src.data_ptr(), off.data_ptr(), _np_ptr(sizes[0]),
                                                                _np_ptr(sizes[1]), _np_ptr(sizes[2]), n_frames, bits.data_ptr(),
                                                                bits.stride(0), int(cap), bpos.data_ptr(), used.data_ptr(), self._stream()))
        else:
            self._ck(self.L.agmv_hip_lz_decode_frames_dev(self.ctx, int(version), src.data_ptr(), off.data_ptr(), avail.data_ptr(),
                                                          usize.data_ptr(), csize.data_ptr(), n_frames, bits.data_ptr(), bits.stride(0),
                                                          int(cap), bpos.data_ptr(), used.data_ptr(), self._stream()))
        return bits, bpos, used

    def lz_decode_commit_dev(self, bits, bpos, n_frames, persist):
        """the reference's persistent buffer over the first n_frames rows, in frame order: each row's 16 bytes behind bpos
        come from the buffer, then the buffer takes the row's [0, bpos).  persist: u8 [cap], updated in place."""
        import torch
        _check_rows("bits", bits, n_frames)
        _check_vec("bpos", bpos, n_frames)
        if not (persist.is_cuda and persist.dtype == torch.uint8 and persist.dim() == 1 and persist.is_contiguous()):
            raise ValueError("persist: a contiguous 1-D CUDA uint8 tensor is needed, got %s %s on %s"
                             % (persist.dtype, tuple(persist.shape), persist.device))
        self._ck(self.L.agmv_hip_lz_decode_commit_dev(self.ctx, bits.data_ptr(), bits.stride(0), bpos.data_ptr(), n_frames,
                                                      persist.data_ptr(), persist.numel(), self._stream()))
        return bits, persist

    def lz_decode_fallback_frames(self):
        """frames of the last lz_decode_frames_dev call that went to the serial kernel (a statistic)"""
        rc = self.L.agmv_hip_lz_decode_fallback_frames(self.ctx, self._stream())
        if rc < 0:
            raise RuntimeError(self.L.agmv_hip_last_error().decode())
        return rc

    def lz_decode_frames(self, version, payloads, usizes, csizes, cap, persist=None):
        """host form of lz_decode_frames_dev + lz_decode_commit_dev: payloads is a list of u8 arrays (every byte that
        exists behind each chunk header).  Returns (rows u8 [n, cap], bpos, used, persist u8 [cap]); row f holds
        data[0, bpos) and the 16 bytes behind it from the persistent buffer (zero-initialised when persist is None)."""
        payloads = [np.ascontiguousarray(x, np.uint8) for x in payloads]
        n = len(payloads)
        if len(usizes) != n or len(csizes) != n:
            raise ValueError("payloads, usizes and csizes must have the same length")
        cap = int(cap)
        lens = np.array([len(x) for x in payloads], np.uint64)
        off = np.zeros(max(n, 1), np.uint64)
        if n:
            off[1:n] = np.cumsum(lens)[:-1]
        src = np.concatenate(payloads + [np.zeros(1, np.uint8)])
        avail = lens.astype(np.uint32) if n else np.zeros(1, np.uint32)
        us = np.ascontiguousarray(np.asarray(usizes, np.uint64).astype(np.uint32)) if n else np.zeros(1, np.uint32)
        cs = np.ascontiguousarray(np.asarray(csizes, np.uint64).astype(np.uint32)) if n else np.zeros(1, np.uint32)
        rows = np.zeros((max(n, 1), max(cap, 1)), np.uint8)
        per = np.zeros(max(cap, 1), np.uint8) if persist is None else np.array(persist, np.uint8, copy=True)
        if per.size < cap:
            raise ValueError("persist: %d bytes, cap is %d" % (per.size, cap))
        bpos = np.zeros(max(n, 1), np.uint32)
        used = np.zeros(max(n, 1), np.uint32)
        self._ck(self.L.agmv_hip_lz_decode_frames(self.ctx, int(version), _np_ptr(src), src.size - 1, _np_ptr(off), _np_ptr(avail),
                                                  _np_ptr(us), _np_ptr(cs), n, _np_ptr(rows), rows.shape[1], cap,
                                                  _np_ptr(bpos), _np_ptr(used), _np_ptr(per)))
        return rows[:n], bpos[:n], used[:n], per[:cap]

    def parse_fallback_frames(self):
        """frames of the last parse that went to the robust kernels (a statistic)"""
        rc = self.L.agmv_hip_parse_fallback_frames(self.ctx, self._stream())
        if rc < 0:
            raise RuntimeError(self.L.agmv_hip_last_error().decode())
        return rc

    def parse_decode_dev(self, bits, bpos, n_frames, w, h, first_frame_count=0, out=None, offsets=None, nentered=None,
                         prev=None, prev_iframe=None):
        """parse + reconstruct in one overlapped call; returns (pixels, offsets, nentered)"""
        import torch
        nblk = (w // 4) * (h // 4)
        if offsets is None:
            offsets = torch.empty((n_frames, nblk), dtype=torch.int32, device=bits.device)
        if nentered is None:
            nentered = torch.empty(n_frames, dtype=torch.int32, device=bits.device)
        if out is None:
            out = torch.empty((n_frames, h, w), dtype=torch.int32, device=bits.device)
        self._ck(self.L.agmv_hip_parse_decode_frames_dev(
            self.ctx, bits.data_ptr(), bits.stride(0), bpos.data_ptr(), n_frames, w, h, first_frame_count,
            offsets.data_ptr(), nentered.data_ptr(), out.data_ptr(),
            prev.data_ptr() if prev is not None else None,
            prev_iframe.data_ptr() if prev_iframe is not None else None, self._stream()))
        return out, offsets, nentered

    def decode_bitstreams_dev(self, bits, bpos, n_frames, w, h, first_frame_count=0, out=None, nentered=None,
                              prev=None, prev_iframe=None):
        """parse + reconstruct without offsets[] (entry bitmaps straight into k_decode); returns the pixels"""
        import torch
        if out is None:
            out = torch.empty((n_frames, h, w), dtype=torch.int32, device=bits.device)
        self._ck(self.L.agmv_hip_decode_bitstreams_dev(
            self.ctx, bits.data_ptr(), bits.stride(0), bpos.data_ptr(), n_frames, w, h, first_frame_count,
            nentered.data_ptr() if nentered is not None else None, out.data_ptr(),
            prev.data_ptr() if prev is not None else None,
            prev_iframe.data_ptr() if prev_iframe is not None else None, self._stream()))
        return out

    def decode_depends_on_prior(self, w, h):
        """after decode_dev: does any pixel of that batch derive from prev / prev_iframe (see agmv_hip.h)?"""
        rc = self.L.agmv_hip_decode_prior_dependent(self.ctx, w, h, self._stream())
        if rc < 0:
            raise RuntimeError(self.L.agmv_hip_last_error().decode())
        return bool(rc)

    def synth_dev(self, w, h, t0, n_frames, seed=0xA6D5, out=None, device=None):
        import torch
        if out is None:
            out = torch.empty((n_frames, h, w), dtype=torch.int32, device=device or ("cuda:%d" % self.device))
        self._ck(self.L.agmv_hip_synth_dev(self.ctx, out.data_ptr(), w, h, t0, n_frames, seed, self._stream()))
        return out

    def interp_dev(self, f1, f2):
        import torch
        out = torch.empty_like(f1)
        self._ck(self.L.agmv_hip_interp_dev(self.ctx, out.data_ptr(), f1.data_ptr(), f2.data_ptr(), f1.numel(),
                                            self._stream()))
        return out

    def histogram_dev(self, pix, quality=1, hist=None):
        import torch
        if hist is None:
            hist = torch.zeros(1 << 19, dtype=torch.int32, device=pix.device)
        self._ck(self.L.agmv_hip_histogram_dev(self.ctx, pix.data_ptr(), pix.numel(), quality, hist.data_ptr(),
                                               self._stream()))
        return hist

    def similarity_dev(self, pix, counts=None):
        """pix: int32 CUDA tensor [n_frames, ...]; returns counts[n_frames - 1] (int32 storage) of equal-grey positions of
        each adjacent pair.  `counts` is overwritten."""
        import torch
        n = pix.shape[0]
        if not (pix.is_cuda and pix.dtype == torch.int32 and pix.is_contiguous() and n >= 1 and pix.numel() > 0):
            raise ValueError("similarity_dev: a contiguous CUDA int32 tensor [n_frames, ...] is needed")
        if counts is None:
            counts = torch.empty(max(n - 1, 0), dtype=torch.int32, device=pix.device)
        _check_vec("similarity_dev: counts", counts, n - 1)
        self._ck(self.L.agmv_hip_similarity_dev(self.ctx, pix.data_ptr(), n, pix.numel() // n, counts.data_ptr(), self._stream()))
        return counts

    def gather_dev(self, src, index, out=None):
        """src: int32 CUDA tensor [n_frames, src_px]; index: int32 storage of uint32 [n_out] (-1 = no source pixel);
        returns [n_frames, n_out]"""
        import torch
        if not (src.is_cuda and src.dtype == torch.int32 and src.dim() == 2 and src.is_contiguous()):
            raise ValueError("gather_dev: a contiguous CUDA int32 tensor [n_frames, src_px] is needed")
        _check_vec("gather_dev: index", index, 1)
        n, n_out = src.shape[0], index.numel()
        if out is None:
            out = torch.empty((n, n_out), dtype=torch.int32, device=src.device)
        if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n * n_out):
            raise ValueError("gather_dev: out must be a contiguous CUDA int32 tensor of n_frames * n_out entries")
        self._ck(self.L.agmv_hip_gather_dev(self.ctx, src.data_ptr(), src.shape[1], n, index.data_ptr(), n_out, out.data_ptr(),
                                            self._stream()))
        return out

    # ------------------------------------------------------------------ clips in the caller's pixel layout
    # A clip in a byte format is a CUDA uint8 tensor of any shape holding whole frames back to back (it may be a view at any byte
    # offset of an allocation); packed pixels are int32 storage as everywhere else.
    def _check_clip(self, name, fmt, t, n_bytes):
        import torch
        fmt = pixfmt(fmt)
        dt = torch.int32 if fmt == 1 else torch.uint8
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() * t.element_size() >= n_bytes):
            raise ValueError("%s: a contiguous CUDA %s tensor of >= %d bytes is needed, got %s %s on %s"
                             % (name, dt, n_bytes, t.dtype, tuple(t.shape), t.device))
        return fmt

    def pixfmt_frame_bytes(self, fmt, n_pixels):
        return self.L.agmv_hip_pixfmt_frame_bytes(pixfmt(fmt), n_pixels)

    def pixels_to_xrgb_dev(self, fmt, src, frame_pixels, n_frames, n_pixels=None, out=None):
        """src: clip of n_frames frames of frame_pixels in fmt -> int32 [n_frames, n_pixels] of 0x00RRGGBB (the first n_pixels of each)"""
        import torch
        n_pixels = frame_pixels if n_pixels is None else n_pixels
        fmt = self._check_clip("pixels_to_xrgb_dev: src", fmt, src, n_frames * self.pixfmt_frame_bytes(fmt, frame_pixels))
        if out is None:
            out = torch.empty((n_frames, n_pixels), dtype=torch.int32, device=src.device)
        _check_vec("pixels_to_xrgb_dev: out", out, n_frames * n_pixels)
        self._ck(self.L.agmv_hip_pixels_to_xrgb_dev(self.ctx, fmt, src.data_ptr(), frame_pixels, n_frames, n_pixels, out.data_ptr(), self._stream()))
        return out

    def pixels_from_xrgb_dev(self, fmt, src, out=None):
        """src: int32 [n_frames, n_pixels] -> the clip in fmt (uint8 [n_frames, frame bytes]; int32 [n_frames, n_pixels] for xrgb32)"""
        import torch
        if not (src.is_cuda and src.dtype == torch.int32 and src.dim() == 2 and src.is_contiguous()):
            raise ValueError("pixels_from_xrgb_dev: a contiguous CUDA int32 tensor [n_frames, n_pixels] is needed")
        n, npx = src.shape
        fb = self.pixfmt_frame_bytes(fmt, npx)
        if out is None:
            out = torch.empty((n, npx), dtype=torch.int32, device=src.device) if pixfmt(fmt) == 1 else torch.empty((n, fb), dtype=torch.uint8, device=src.device)
        fmt = self._check_clip("pixels_from_xrgb_dev: out", fmt, out, n * fb)
        self._ck(self.L.agmv_hip_pixels_from_xrgb_dev(self.ctx, fmt, src.data_ptr(), n, npx, out.data_ptr(), self._stream()))
        return out

    def gather_fmt_dev(self, fmt, src, src_frame_pixels, n_frames, index, out=None):
        """gather_dev on a clip of n_frames frames of src_frame_pixels in fmt; returns int32 [n_frames, n_out]"""
        import torch
        fmt = self._check_clip("gather_fmt_dev: src", fmt, src, n_frames * self.pixfmt_frame_bytes(fmt, src_frame_pixels))
        _check_vec("gather_fmt_dev: index", index, 1)
        n_out = index.numel()
        if out is None:
            out = torch.empty((n_frames, n_out), dtype=torch.int32, device=src.device)
        _check_vec("gather_fmt_dev: out", out, n_frames * n_out)
        self._ck(self.L.agmv_hip_gather_fmt_dev(self.ctx, fmt, src.data_ptr(), src_frame_pixels, n_frames, index.data_ptr(), n_out, out.data_ptr(),
                                                self._stream()))
        return out

    def histogram_fmt_dev(self, fmt, src, frame_pixels, n_frames, n_pixels=None, quality=1, hist=None):
        """histogram_dev over the first n_pixels of each frame of a clip in fmt; `hist` is added to"""
        import torch
        n_pixels = frame_pixels if n_pixels is None else n_pixels
        fmt = self._check_clip("histogram_fmt_dev: src", fmt, src, n_frames * self.pixfmt_frame_bytes(fmt, frame_pixels))
        if hist is None:
            hist = torch.zeros(1 << 19, dtype=torch.int32, device=src.device)
        _check_vec("histogram_fmt_dev: hist", hist, 1 << 19)
        self._ck(self.L.agmv_hip_histogram_fmt_dev(self.ctx, fmt, src.data_ptr(), frame_pixels, n_frames, n_pixels, quality, hist.data_ptr(),
                                                   self._stream()))
        return hist

    def similarity_fmt_dev(self, fmt, src, n_frames, n_pixels, counts=None):
        """similarity_dev on a clip of n_frames frames of n_pixels in fmt; `counts` [n_frames - 1] is overwritten"""
        import torch
        fmt = self._check_clip("similarity_fmt_dev: src", fmt, src, n_frames * self.pixfmt_frame_bytes(fmt, n_pixels))
        if counts is None:
            counts = torch.empty(max(n_frames - 1, 0), dtype=torch.int32, device=src.device)
        _check_vec("similarity_fmt_dev: counts", counts, n_frames - 1)
        self._ck(self.L.agmv_hip_similarity_fmt_dev(self.ctx, fmt, src.data_ptr(), n_frames, n_pixels, counts.data_ptr(), self._stream()))
        return counts

    # ------------------------------------------------------------------ clips in YUV 4:2:0 (NV12 / I420)
    # A clip is a contiguous CUDA uint8 tensor of any shape holding whole frames back to back (a view at any byte offset will do);
    # fmt is a name of YUVFMT plus yuv= / full_range=, or the value with its flags.
    def yuv_frame_bytes(self, fmt, w, h):
        return self.L.agmv_hip_yuv_frame_bytes(yuvfmt(fmt), w, h)

    def _check_yuv(self, name, fmt, t, w, h, n_frames, yuv, full_range):
        import torch
        fmt = yuvfmt(fmt, yuv, full_range)
        need = n_frames * self.L.agmv_hip_yuv_frame_bytes(fmt, w, h)
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= need):
            raise ValueError("%s: a contiguous CUDA uint8 tensor of >= %d bytes is needed, got %s %s on %s" % (name, need, t.dtype, tuple(t.shape), t.device))
        return fmt

    def yuv_to_xrgb_dev(self, fmt, src, w, h, n_frames, n_pixels=None, out=None, yuv=None, full_range=False):
        """src: clip of n_frames frames of w x h -> int32 [n_frames, n_pixels] of 0x00RRGGBB (the first n_pixels of each, raster order)"""
        import torch
        n_pixels = w * h if n_pixels is None else n_pixels
        fmt = self._check_yuv("yuv_to_xrgb_dev: src", fmt, src, w, h, n_frames, yuv, full_range)
        if out is None:
            out = torch.empty((n_frames, n_pixels), dtype=torch.int32, device=src.device)
        _check_vec("yuv_to_xrgb_dev: out", out, n_frames * n_pixels)
        self._ck(self.L.agmv_hip_yuv_to_xrgb_dev(self.ctx, fmt, src.data_ptr(), w, h, n_frames, n_pixels, out.data_ptr(), self._stream()))
        return out

    def yuv_from_xrgb_dev(self, fmt, src, w, h, out=None, yuv=None, full_range=False):
        """src: int32 [n_frames, w * h] -> the clip as uint8 [n_frames, frame bytes]"""
        import torch
        if not (src.is_cuda and src.dtype == torch.int32 and src.dim() == 2 and src.is_contiguous() and src.shape[1] == w * h):
            raise ValueError("yuv_from_xrgb_dev: a contiguous CUDA int32 tensor [n_frames, w * h] is needed")
        n = src.shape[0]
        if out is None:
            out = torch.empty((n, self.L.agmv_hip_yuv_frame_bytes(yuvfmt(fmt, yuv, full_range), w, h)), dtype=torch.uint8, device=src.device)
        fmt = self._check_yuv("yuv_from_xrgb_dev: out", fmt, out, w, h, n, yuv, full_range)
        self._ck(self.L.agmv_hip_yuv_from_xrgb_dev(self.ctx, fmt, src.data_ptr(), w, h, n, out.data_ptr(), self._stream()))
        return out

    def yuv_gather_dev(self, fmt, src, w, h, n_frames, index, out=None, yuv=None, full_range=False):
        """gather_dev on a YUV clip of n_frames frames of w x h (index: y * w + x); returns int32 [n_frames, n_out]"""
        import torch
        fmt = self._check_yuv("yuv_gather_dev: src", fmt, src, w, h, n_frames, yuv, full_range)
        _check_vec("yuv_gather_dev: index", index, 1)
        n_out = index.numel()
        if out is None:
            out = torch.empty((n_frames, n_out), dtype=torch.int32, device=src.device)
        _check_vec("yuv_gather_dev: out", out, n_frames * n_out)
        self._ck(self.L.agmv_hip_yuv_gather_dev(self.ctx, fmt, src.data_ptr(), w, h, n_frames, index.data_ptr(), n_out, out.data_ptr(), self._stream()))
        return out

    def yuv_histogram_dev(self, fmt, src, w, h, n_frames, n_pixels=None, quality=1, hist=None, yuv=None, full_range=False):
        """histogram_dev over the first n_pixels of each frame of a YUV clip; `hist` is added to"""
        import torch
        n_pixels = w * h if n_pixels is None else n_pixels
        fmt = self._check_yuv("yuv_histogram_dev: src", fmt, src, w, h, n_frames, yuv, full_range)
        if hist is None:
            hist = torch.zeros(1 << 19, dtype=torch.int32, device=src.device)
        _check_vec("yuv_histogram_dev: hist", hist, 1 << 19)
        self._ck(self.L.agmv_hip_yuv_histogram_dev(self.ctx, fmt, src.data_ptr(), w, h, n_frames, n_pixels, quality, hist.data_ptr(), self._stream()))
        return hist

    def yuv_similarity_dev(self, fmt, src, w, h, n_frames, counts=None, yuv=None, full_range=False):
        """similarity_dev on a YUV clip of n_frames frames of w x h; `counts` [n_frames - 1] is overwritten"""
        import torch
        fmt = self._check_yuv("yuv_similarity_dev: src", fmt, src, w, h, n_frames, yuv, full_range)
        if counts is None:
            counts = torch.empty(max(n_frames - 1, 0), dtype=torch.int32, device=src.device)
        _check_vec("yuv_similarity_dev: counts", counts, n_frames - 1)
        self._ck(self.L.agmv_hip_yuv_similarity_dev(self.ctx, fmt, src.data_ptr(), w, h, n_frames, counts.data_ptr(), self._stream()))
        return counts

    # ------------------------------------------------------------------ a clip scaled down (AGMV_SCALE_AREA of include/agmv.h)
    def scale_area_dev(self, fmt, src, w, h, n_frames, dst_w, dst_h, out=None, yuv=None, full_range=False):
        """src: clip of n_frames frames of w x h in fmt (any name of PIXFMT or YUVFMT, or its value) -> int32 [n_frames, dst_h, dst_w]
        of 0x00RRGGBB: the exact box filter, dst_w <= w, dst_h <= h, w * h <= 2^24"""
        import torch
        if fmt in YUVFMT or (isinstance(fmt, int) and (fmt & 0xFF) in YUVFMT.values()):
            fmt = self._check_yuv("scale_area_dev: src", fmt, src, w, h, n_frames, yuv, full_range)
        else:
            if yuv is not None or full_range:
                raise ValueError("scale_area_dev: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (fmt,))
            fmt = self._check_clip("scale_area_dev: src", fmt, src, n_frames * self.pixfmt_frame_bytes(fmt, w * h))
        if out is None:
            out = torch.empty((n_frames, dst_h, dst_w), dtype=torch.int32, device=src.device)
        _check_vec("scale_area_dev: out", out, n_frames * dst_w * dst_h)
        self._ck(self.L.agmv_hip_scale_area_dev(self.ctx, fmt, src.data_ptr(), w, h, n_frames, dst_w, dst_h, out.data_ptr(), self._stream()))
        return out

    # ------------------------------------------------------------------ a decoded clip at a target size (AGMV_SCALE_NEAREST / _BILINEAR of include/agmv.h)
    def scale_frames_async(self, filt, src, w, h, n_frames, fmt, dst_w, dst_h, out=None, yuv=None, full_range=False, stream=None):
        """src: int32 CUDA tensor of n_frames frames of w x h pixels 0x00RRGGBB -> the clip scaled to dst_w x dst_h with `filt`
        (1 nearest, 3 bilinear) in fmt (any name of PIXFMT or YUVFMT, or its value): uint8 [n_frames, frame bytes], or `out`, a
        contiguous CUDA tensor of at least that many bytes (agmv_hip_scale_frames_async) on `stream` (a torch stream; None =
        torch's current one).  Nothing waits."""
        import torch
        w, h, n_frames, dst_w, dst_h = int(w), int(h), int(n_frames), int(dst_w), int(dst_h)
        _check_vec("scale_frames_async: src", src, n_frames * w * h)
        if fmt in YUVFMT or (isinstance(fmt, int) and (fmt & 0xFF) in YUVFMT.values()):
            fmt = yuvfmt(fmt, yuv, full_range)
            fb = self.L.agmv_hip_yuv_frame_bytes(fmt, dst_w, dst_h)
        else:
            if yuv is not None or full_range:
                raise ValueError("scale_frames_async: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (fmt,))
            fmt = pixfmt(fmt)
            fb = self.pixfmt_frame_bytes(fmt, dst_w * dst_h)
        if out is None:
            out = torch.empty((n_frames, fb), dtype=torch.uint8, device=src.device)
        elif not (out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= n_frames * fb):
            raise ValueError("scale_frames_async: out must be a contiguous CUDA tensor of >= %d bytes" % (n_frames * fb))
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_scale_frames_async(self.ctx, int(filt), src.data_ptr(), w, h, n_frames, fmt, dst_w, dst_h, out.data_ptr(), s))
        return out

    # ------------------------------------------------------------------ a view of a decoded clip (agmv_hip_view_frames_async of include/agmv_hip_view.h)
    def view_frames_async(self, src, w, h, first, step, count, x, y, win_w, win_h, out=None, stream=None):
        """src: int32 CUDA tensor of whole frames of w x h pixels -> int32 [count, win_h, win_w]: the window win_w x win_h at (x, y) of
        the frames first, first + step, ... (count of them, all inside src), whole words copied as they are, or `out`, a contiguous
        CUDA int32 tensor (or view at any element offset) of at least that many words (agmv_hip_view_frames_async) on `stream` (a
        torch stream; None = torch's current one).  Nothing waits."""
        import torch
        w, h, first, step, count, x, y, win_w, win_h = (int(v) for v in (w, h, first, step, count, x, y, win_w, win_h))
        if step < 1 or count < 0 or first < 0:
            raise ValueError("view_frames_async: first >= 0, step >= 1 and count >= 0 are needed, got %d, %d, %d" % (first, step, count))
        _check_vec("view_frames_async: src", src, (first + (count - 1) * step + 1) * w * h if count else 0)
        if out is None:
            out = torch.empty((count, win_h, win_w), dtype=torch.int32, device=src.device)
        _check_vec("view_frames_async: out", out, count * win_w * win_h)
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_view_frames_async(self.ctx, src.data_ptr(), w, h, first, step, count, x, y, win_w, win_h, out.data_ptr(), s))
        return out

    # ------------------------------------------------------------------ a view of a clip in any layout (agmv_hip_view_source_async of include/agmv_hip_view_source.h)
    def view_source(self, fmt, src, w, h, first, step, count, x, y, win_w, win_h, out=None, yuv=None, full_range=False, stream=None):
        """src: clip of whole frames of w x h pixels in fmt (any name of PIXFMT or YUVFMT, or its value) -> int32 [count, win_h, win_w]
        of 0x00RRGGBB: the window win_w x win_h at (x, y) of the frames first, first + step, ... (count of them, all inside src) as
        pixels_to_xrgb_dev / yuv_to_xrgb_dev give them ("xrgb32": whole words as they are), or `out`, a contiguous CUDA int32 tensor
        (or view at any element offset) of at least that many words (agmv_hip_view_source_async) on `stream` (a torch stream;
        None = torch's current one).  Nothing waits."""
        import torch
        w, h, first, step, count, x, y, win_w, win_h = (int(v) for v in (w, h, first, step, count, x, y, win_w, win_h))
        if step < 1 or count < 0 or first < 0:
            raise ValueError("view_source: first >= 0, step >= 1 and count >= 0 are needed, got %d, %d, %d" % (first, step, count))
        n = first + (count - 1) * step + 1 if count else 0
        if fmt in YUVFMT or (isinstance(fmt, int) and (fmt & 0xFF) in YUVFMT.values()):
            fmt = self._check_yuv("view_source: src", fmt, src, w, h, n, yuv, full_range)
        else:
            if yuv is not None or full_range:
                raise ValueError("view_source: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (fmt,))
            fmt = self._check_clip("view_source: src", fmt, src, n * self.pixfmt_frame_bytes(fmt, w * h))
        if out is None:
            out = torch.empty((count, win_h, win_w), dtype=torch.int32, device=src.device)
        _check_vec("view_source: out", out, count * win_w * win_h)
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_view_source_async(self.ctx, fmt, src.data_ptr(), w, h, first, step, count, x, y, win_w, win_h, out.data_ptr(), s))
        return out

    # ------------------------------------------------------------------ such a view at another frame rate (agmv_hip_time_frames_async of include/agmv_hip_time.h)
    def time_frames(self, fmt, src, w, h, n_frames, first, step, view_len, x, y, win_w, win_h, rate, time="area", j0=0, count=None, out=None,
                    yuv=None, full_range=False, stream=None):
        """src: clip of n_frames whole frames of w x h pixels in fmt (any name of PIXFMT or YUVFMT, or its value) -> int32
        [count, win_h, win_w] of 0x00RRGGBB: frames j0 .. j0 + count - 1 (count None: to the last) of the view view_source gives for
        first, step, count=view_len and the window, resampled in time at rate = (src, dst), a reduced pair, with the filter
        time = "area" or "nearest" (AGMV_RATE of include/agmv.h holds the rule), or `out`, a contiguous CUDA int32 tensor (or view at
        any element offset) of at least that many words (agmv_hip_time_frames_async) on `stream` (a torch stream; None = torch's
        current one).  Nothing waits."""
        import torch
        w, h, n_frames, first, step, view_len, x, y, win_w, win_h, j0 = (int(v) for v in (w, h, n_frames, first, step, view_len, x, y, win_w, win_h, j0))
        if time not in TIME:
            raise ValueError("time_frames: time %r is unknown: one of %s is needed" % (time, ", ".join("\"%s\"" % k for k in sorted(TIME))))
        rs, rd = (int(v) for v in rate)
        if rs < 1 or rd < 1:
            raise ValueError("time_frames: rate must be a pair of ints above 0, got %r" % (rate,))
        if step < 1 or view_len < 0 or first < 0 or n_frames < 0 or j0 < 0:
            raise ValueError("time_frames: first >= 0, step >= 1, view_len >= 0 and j0 >= 0 are needed, got %d, %d, %d, %d" % (first, step, view_len, j0))
        if count is None:
            count = max(view_len * rd // rs - j0, 0)
        count = int(count)
        if fmt in YUVFMT or (isinstance(fmt, int) and (fmt & 0xFF) in YUVFMT.values()):
            fmt = self._check_yuv("time_frames: src", fmt, src, w, h, n_frames, yuv, full_range)
        else:
            if yuv is not None or full_range:
                raise ValueError("time_frames: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (fmt,))
            fmt = self._check_clip("time_frames: src", fmt, src, n_frames * self.pixfmt_frame_bytes(fmt, w * h))
        if out is None:
            out = torch.empty((count, win_h, win_w), dtype=torch.int32, device=src.device)
        _check_vec("time_frames: out", out, count * win_w * win_h)
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_time_frames_async(self.ctx, fmt, src.data_ptr(), w, h, n_frames, first, step, view_len, x, y, win_w, win_h, rs, rd, TIME[time], j0,
                                                   count, out.data_ptr(), s))
        return out

    # ------------------------------------------------------------------ normalised float tensor clips (AGMV_TENSORFMT of include/agmv.h)
    def tensor_from_xrgb_async(self, fmt, src, w, h, n_frames, table, out, filt=0, dst_w=None, dst_h=None, stream=None):
        """src: int32 CUDA tensor of n_frames frames of w x h pixels 0x00RRGGBB -> out, a contiguous CUDA tensor (or view at any
        element offset) of n_frames * 3 * dst_h * dst_w elements of fmt ("f32", "f16", "bf16" or its value), through `table`, the
        768 elements of tensor_table() on the device (agmv_hip_tensor_from_xrgb_async).  filt 0 = no scale, 1 nearest, 3 bilinear.
        On `stream` (a torch stream; None = torch's current one).  Nothing waits."""
        v = tensorfmt(fmt)
        w, h, n_frames = int(w), int(h), int(n_frames)
        dst_w, dst_h = (w if dst_w is None else int(dst_w)), (h if dst_h is None else int(dst_h))
        _check_vec("tensor_from_xrgb_async: src", src, n_frames * w * h)
        need = n_frames * self.L.agmv_hip_tensor_frame_bytes(v, dst_w * dst_h)
        if not (out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= need):
            raise ValueError("tensor_from_xrgb_async: out must be a contiguous CUDA tensor of >= %d bytes" % need)
        if not (table.is_cuda and table.is_contiguous() and table.numel() * table.element_size() >= 768 * (4 if v == 1 else 2)):
            raise ValueError("tensor_from_xrgb_async: table must be a contiguous CUDA tensor of 768 elements")
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_tensor_from_xrgb_async(self.ctx, v, src.data_ptr(), w, h, n_frames, int(filt), dst_w, dst_h, table.data_ptr(),
                                                        out.data_ptr(), s))
        return out

    def tensor_to_xrgb_async(self, fmt, src, frame_pixels, n_frames, ab, out=None, stream=None):
        """src: contiguous CUDA tensor (or view) of n_frames frames of 3 * frame_pixels elements of fmt -> int32 [n_frames,
        frame_pixels] of 0x00RRGGBB by the reading rule (agmv_hip_tensor_to_xrgb_async); ab: six numbers, a[3] then b[3], taken as
        float32.  On `stream` (a torch stream; None = torch's current one).  Nothing waits."""
        import torch
        v = tensorfmt(fmt)
        frame_pixels, n_frames = int(frame_pixels), int(n_frames)
        need = n_frames * self.L.agmv_hip_tensor_frame_bytes(v, frame_pixels)
        if not (src.is_cuda and src.is_contiguous() and src.numel() * src.element_size() >= need):
            raise ValueError("tensor_to_xrgb_async: src must be a contiguous CUDA tensor of >= %d bytes" % need)
        if out is None:
            out = torch.empty((n_frames, frame_pixels), dtype=torch.int32, device=src.device)
        _check_vec("tensor_to_xrgb_async: out", out, n_frames * frame_pixels)
        k = (C.c_float * 6)(*[float(x) for x in ab])
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_tensor_to_xrgb_async(self.ctx, v, src.data_ptr(), frame_pixels, n_frames, k, out.data_ptr(), s))
        return out

    # ------------------------------------------------------------------ the palette refined by weighted k-means (include/agmv.h)
    def palette_refine_dev(self, hist, quality, pal, n_free, iterations):
        """hist: int32 storage of the 2^19 u32 bins (not modified); pal: int32 storage of k colours 0x00RRGGBB, refined in place (the
        first n_free move).  Returns (rounds int32 [1], sse int64 storage of two u64: before, after), device tensors; nothing waits."""
        import torch
        _check_vec("palette_refine_dev: hist", hist, 1 << 19)
        _check_vec("palette_refine_dev: pal", pal, 1)
        rounds = torch.empty(1, dtype=torch.int32, device=hist.device)
        sse = torch.empty(2, dtype=torch.int64, device=hist.device)
        self._ck(self.L.agmv_hip_palette_refine_dev(self.ctx, hist.data_ptr(), int(quality), pal.data_ptr(), pal.numel(), int(n_free), int(iterations),
                                                    rounds.data_ptr(), sse.data_ptr(), self._stream()))
        return rounds, sse

    # ------------------------------------------------------------------ temporal stabilisation of a batch (include/agmv.h; agmv_hip_stabilise_frames_async of include/agmv_hip_stabilise.h)
    def stabilise_frames(self, pix, w, h, strength, first_fc=0, count=None, stream=None):
        """pix: int32 CUDA tensor (or view at any element offset) of whole frames of w x h pixels with frame counts first_fc,
        first_fc + 1, ..., stabilised in place (agmv_hip_stabilise_frames_async) on `stream` (a torch stream; None = torch's current
        stream).  strength 1 .. 64.  count: None, or an int64 CUDA tensor of one element on the same device, to which the number of
        replaced blocks is added (the caller sets it to zero).  Returns pix; nothing waits."""
        import torch
        _check_vec("stabilise_frames: pix", pix, 0)
        w, h = int(w), int(h)
        if w < 1 or h < 1 or pix.numel() % (w * h):
            raise ValueError("stabilise_frames: pix must hold whole frames of %d x %d pixels, got %d words" % (w, h, pix.numel()))
        if count is not None and not (count.is_cuda and count.dtype == torch.int64 and count.numel() == 1 and count.device == pix.device):
            raise ValueError("stabilise_frames: count must be an int64 CUDA tensor of one element on the device of pix")
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_stabilise_frames_async(self.ctx, int(strength), pix.data_ptr(), w, h, pix.numel() // (w * h), int(first_fc),
                                                        count.data_ptr() if count is not None else None, s))
        return pix

    # ------------------------------------------------------------------ deblocking of a decoded clip (include/agmv.h; agmv_hip_deblock_frames_async of include/agmv_hip_deblock.h)
    def deblock_frames(self, pix, w, h, strength, out=None, counts=None, stream=None):
        """pix: int32 CUDA tensor (or view at any element offset) of whole frames of w x h pixels, deblocked (agmv_hip_deblock_frames_async)
        into out -- None = a new tensor of the same shape; pix itself is allowed, any other overlap is the caller's error -- on `stream`
        (a torch stream; None = torch's current stream).  strength 1 .. 64.  counts: None, or an int64 CUDA tensor of two elements on
        the same device, to which the weak and the strong lines are added (the caller sets them to zero).  Returns out; nothing waits."""
        import torch
        _check_vec("deblock_frames: pix", pix, 0)
        w, h = int(w), int(h)
        if w < 1 or h < 1 or pix.numel() % (w * h):
            raise ValueError("deblock_frames: pix must hold whole frames of %d x %d pixels, got %d words" % (w, h, pix.numel()))
        if out is None:
            out = torch.empty_like(pix)
        else:
            _check_vec("deblock_frames: out", out, 0)
            if out.numel() != pix.numel() or out.device != pix.device:
                raise ValueError("deblock_frames: out must hold as many words as pix, on its device")
        if counts is not None and not (counts.is_cuda and counts.dtype == torch.int64 and counts.numel() == 2 and counts.is_contiguous()
                                       and counts.device == pix.device):
            raise ValueError("deblock_frames: counts must be a contiguous int64 CUDA tensor of two elements on the device of pix")
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_deblock_frames_async(self.ctx, int(strength), pix.data_ptr(), w, h, pix.numel() // (w * h), out.data_ptr(),
                                                      counts.data_ptr() if counts is not None else None, s))
        return out

    # ------------------------------------------------------------------ pattern dithering against the context's palette (include/agmv.h)
    def dither_frames(self, pix, w, h, strength, stream=None):
        """pix: int32 CUDA tensor of whole frames of w x h pixels 0x00RRGGBB, dithered in place (agmv_hip_dither_frames_async) on
        `stream` (a torch stream; None = torch's current stream).  strength 1 .. 64.  Returns pix; nothing waits."""
        _check_vec("dither_frames: pix", pix, 0)
        w, h = int(w), int(h)
        if w < 1 or h < 1 or pix.numel() % (w * h):
            raise ValueError("dither_frames: pix must hold whole frames of %d x %d pixels, got %d words" % (w, h, pix.numel()))
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_dither_frames_async(self.ctx, int(strength), pix.data_ptr(), w, h, pix.numel() // (w * h), s))
        return pix

    # ------------------------------------------------------------------ a decoded clip measured against its reference (include/agmv.h)
    def measure_frames(self, test, fmt, ref, w, h, n_frames, out=None, yuv=None, full_range=False, stream=None):
        """test: int32 CUDA tensor of n_frames frames of w x h pixels 0x00RRGGBB; ref: the same frames in fmt (any name of PIXFMT or
        YUVFMT, or its value) -> int64 [n_frames, 12]: sse, block_sse, max_err and ssim (Q20 sums) of R, G, B per frame
        (agmv_hip_measure_frames_async) on `stream` (a torch stream; None = torch's current one).  Nothing waits."""
        import torch
        w, h, n_frames = int(w), int(h), int(n_frames)
        _check_vec("measure_frames: test", test, n_frames * w * h)
        if fmt in YUVFMT or (isinstance(fmt, int) and (fmt & 0xFF) in YUVFMT.values()):
            fmt = self._check_yuv("measure_frames: ref", fmt, ref, w, h, n_frames, yuv, full_range)
        else:
            if yuv is not None or full_range:
                raise ValueError("measure_frames: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (fmt,))
            fmt = self._check_clip("measure_frames: ref", fmt, ref, n_frames * self.pixfmt_frame_bytes(fmt, w * h))
        if out is None:
            out = torch.empty((n_frames, 12), dtype=torch.int64, device=test.device)
        elif not (out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= 12 * n_frames):
            raise ValueError("measure_frames: out must be a contiguous CUDA int64 tensor of >= %d entries" % (12 * n_frames))
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_measure_frames_async(self.ctx, test.data_ptr(), fmt, ref.data_ptr(), w, h, n_frames, out.data_ptr(), s))
        return out

    # ------------------------------------------------------------------ audio tracks (include/agmv.h, "audio tracks")
    @staticmethod
    def _pcm_shape(name, fmt, pcm):
        """(AGMV_PCMFMT value, channels, samples per channel) of a contiguous CUDA tensor: int16 [n, ch] / uint8 [n, ch] / float32 [ch, n]"""
        import torch
        v = pcmfmt(fmt)
        want = {1: torch.int16, 2: torch.uint8, 3: torch.float32}[v]
        if not (pcm.is_cuda and pcm.dtype == want and pcm.dim() == 2 and pcm.is_contiguous()):
            raise ValueError("%s: fmt %r needs a contiguous CUDA %s tensor %s, got %s %s strides %s on %s"
                             % (name, fmt, want, "[channels, samples]" if v == 3 else "[samples, channels]", pcm.dtype, tuple(pcm.shape), pcm.stride(), pcm.device))
        return (v, pcm.shape[0], pcm.shape[1]) if v == 3 else (v, pcm.shape[1], pcm.shape[0])

    def audio_compand(self, fmt, pcm, codes=None, stream=None):
        """pcm in the layout `fmt` ("s16", "u8" or "f32p") -> uint8 [samples, channels], the track's code bytes
        (agmv_hip_audio_compand_async) on `stream` (a torch stream; None = torch's current one).  Nothing waits."""
        import torch
        v, ch, n = self._pcm_shape("audio_compand", fmt, pcm)
        if codes is None:
            codes = torch.empty((n, ch), dtype=torch.uint8, device=pcm.device)
        elif not (codes.is_cuda and codes.dtype == torch.uint8 and codes.is_contiguous() and codes.numel() == n * ch):
            raise ValueError("audio_compand: codes must be a contiguous CUDA uint8 tensor of %d bytes" % (n * ch))
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_audio_compand_async(self.ctx, v, pcm.data_ptr(), ch, n, codes.data_ptr(), s))
        return codes

    def audio_expand(self, fmt, codes, pcm=None, stream=None):
        """codes uint8 [samples, channels] -> the PCM in the layout `fmt` (agmv_hip_audio_expand_async): int16 / uint8
        [samples, channels] or float32 [channels, samples].  Nothing waits."""
        import torch
        v = pcmfmt(fmt)
        if not (codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2 and codes.is_contiguous()):
            raise ValueError("audio_expand: codes must be a contiguous CUDA uint8 tensor [samples, channels], got %s %s" % (codes.dtype, tuple(codes.shape)))
        n, ch = codes.shape
        if pcm is None:
            pcm = torch.empty((ch, n) if v == 3 else (n, ch), dtype={1: torch.int16, 2: torch.uint8, 3: torch.float32}[v], device=codes.device)
        elif self._pcm_shape("audio_expand", fmt, pcm) != (v, ch, n):
            raise ValueError("audio_expand: pcm of shape %s does not hold %d samples in %d channels as %r" % (tuple(pcm.shape), n, ch, fmt))
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._ck(self.L.agmv_hip_audio_expand_async(self.ctx, v, codes.data_ptr(), ch, n, pcm.data_ptr(), s))
        return pcm

    # ------------------------------------------------------------------ host-buffer path
    def encode_host(self, frames, first_frame_count=0, ientries=None):
        """frames: uint32 ndarray [n, h, w]. Returns list of per-frame bitstreams (uint8 arrays)."""
        frames = np.ascontiguousarray(frames, np.uint32)
        n, h, w = frames.shape
        stride = self.max_usize(w, h)
        out = np.zeros((n, stride), np.uint8)
        sizes = np.zeros(n, np.uint32)
        self._ck(self.L.agmv_hip_encode_frames(self.ctx, _np_ptr(frames), n, w, h, first_frame_count,
                                               _np_ptr(out), stride, _np_ptr(sizes), _np_ptr(ientries)))
        return [out[i, :sizes[i]].copy() for i in range(n)]

    def decode_host(self, bits_list, w, h, first_frame_count=0, prev=None, prev_iframe=None, pad=None):
        """bits_list: per-frame decompressed bitstreams. `pad`[f] = the 16 bytes that follow bpos in
        the reference's persistent buffer (stale bytes), zeros if None."""
        n = len(bits_list)
        stride = (max(len(b) for b in bits_list) + 16 + 255) & ~255
        bits = np.zeros((n, stride), np.uint8)
        bpos = np.zeros(n, np.uint32)
        for i, b in enumerate(bits_list):
            bits[i, :len(b)] = b
            bpos[i] = len(b)
            if pad is not None:
                bits[i, len(b):len(b) + 16] = pad[i]
        out = np.zeros((n, h, w), np.uint32)
        self._ck(self.L.agmv_hip_decode_frames(self.ctx, _np_ptr(bits), stride, _np_ptr(bpos), n, w, h,
                                               first_frame_count, _np_ptr(out), _np_ptr(prev), _np_ptr(prev_iframe)))
        return out
