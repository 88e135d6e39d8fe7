"""Whole .agmv sequences from and to frames in GPU memory: ctypes calls of AGMV_EncodeFramesFmtDev / AGMV_EncodeFramesScaledDev /
AGMV_EncodeViewDev / AGMV_EncodeViewRateDev / AGMV_DecodeFramesFmtDev / AGMV_DecodeFramesScaledDev / AGMV_EncodeFramesTensorDev / AGMV_DecodeFramesTensorDev (include/agmv.h, libagmv.so).  No logic here: the schedules, the container, both LZ stages and the reading and writing of the
caller's pixel layout are the library's; torch holds the frames.  The frames live on the library's own device (env AGMV_DEVICE,
default 0).
Reader (AGMV_OpenReaderDev ... of include/agmv_reader.h) is a file opened once and read in pieces with the decoder's state kept: what
decode_frames(frames=, crop=) returns chunk by chunk, without the call's fixed cost and without the LZ stage from frame 0 each time.
Writer (AGMV_OpenWriterDev ... of include/agmv_writer.h) is the encoder's counterpart: a clip analysed and written in pieces, from
buffers that may be reused, into the file encode_frames writes for the whole of it, with memory bounded by its staging ring.
clip_quality / file_quality (AGMV_MeasureFramesDev / AGMV_MeasureFileDev) measure a decoded clip, or a file batch by batch, against
the frames it was made from, in any of the layouts below, and return a Quality: exact integers per frame and channel, and the
PSNR, block-mean PSNR and mean SSIM formed from them.

Pixel layouts (AGMV_PIXFMT) and the tensors that hold n frames of h x w:
  "xrgb32"  int32 / uint32 [n, h, w]   0x00RRGGBB
  "rgb24"   uint8 [n, h, w, 3]         R, G, B     (video readers)
  "bgr24"   uint8 [n, h, w, 3]         B, G, R     (OpenCV)
  "rgba32"  uint8 [n, h, w, 4]         R, G, B, A  (image decoders; A is ignored on input and 0xFF on output)
  "rgb8p"   uint8 [n, 3, h, w]         planes R, G, B (models)
  "nv12"    uint8 [n, h * 3 / 2, w]    h rows of Y, then h / 2 rows of U, V pairs      (hardware video decoders and encoders)
  "i420"    uint8 [n, h * 3 / 2, w]    h rows of Y, then the U plane, then the V plane (software decoders, raw .yuv files)
The two YUV 4:2:0 layouts (include/agmv.h has their definition) need even h and w here, are never inferred from a tensor, and
take yuv="bt601" (default) or "bt709" and full_range=False (limited range) or True.

Normalised float tensors (AGMV_TENSORFMT; include/agmv.h, "normalised float tensors"), what a model takes and gives:
  "f32" / "f16" / "bf16"   float32 / float16 / bfloat16 [n, 3, h, w]   planes R, G, B; a byte v stands for (v / 255 - mean[c]) / std[c]
with mean= and std= (a number or three; defaults 0 and 1).  decode_frames writes them through a table, encode_frames reads them by
the header's rule: both are exact, bit for bit.  A floating [n, 3, h, w] tensor is inferred as a tensor clip from its dtype.

Audio tracks (AGMV_PCMFMT; include/agmv.h, "audio tracks") and the tensors that hold n samples per channel of ch channels:
  "s16"   int16 [n, ch]     interleaved, the WAV samples as they are     (16-bit track)
  "u8"    uint8 [n, ch]     interleaved unsigned bytes                   (8-bit track)
  "f32p"  float32 [ch, n]   planar, -1 .. 1, at most 8 channels (torchaudio)   (16-bit track)"""
import contextlib
import ctypes as C
import os

from . import abi
from .abi import AGMV_FRAME_QUALITY, AGMV_INFO  # noqa: F401  (importable from here as before)
from .hip import HERE, PIXFMT, TENSORFMT, TIME, YUVFMT, HipUnavailable, pcmfmt, pixfmt, tensor_normalisation, yuvfmt

SCHEDULE_FULL, SCHEDULE_PDIFS, SCHEDULE_ADAPTIVE = 1, 2, 3
SCALE = {"nearest": 1, "area": 2}          # AGMV_SCALE of include/agmv.h, which defines both filters
DECODE_SCALE = {"nearest": 1, "area": 2, "bilinear": 3}      # ... and the filters of decode_frames(size=): AGMV_DecodeFramesScaledDev


_lib = None


def load_library():
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (torch's HIP runtime first, as in hip.load_library)
        p = os.path.join(HERE, "libagmv.so")
        if not os.path.exists(p):
            raise HipUnavailable("%s is missing: run `python -m libagmv_amd.build`; the AGMV hot path has no CPU fallback" % p)
        _lib = abi.bind(abi.bind(abi.bind(C.CDLL(p), abi.AGMV), abi.READER), abi.WRITER)
    return _lib


def _device():
    return "cuda:%d" % int(os.environ.get("AGMV_DEVICE", "0"))


def _fmt_value(who, fmt, yuv, full_range):
    """the fmt argument of the library for a name (or value) and the two YUV options, which only a YUV layout may carry"""
    if fmt in YUVFMT:
        return yuvfmt(fmt, yuv, full_range)
    if yuv is not None or full_range:
        raise ValueError("%s: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (who, fmt))
    return pixfmt(fmt)


def _clip_geometry(frames, fmt, yuv=None, full_range=False, who="encode_frames"):
    """(fmt value for the library, n, h, w) of a tensor of frames; fmt None = inferred from dtype and shape (never a YUV layout).
    Raises ValueError naming `fmt` for a tensor that holds no clip of that layout, in the name of the caller `who`; touches neither
    the library nor the device."""
    import torch
    if fmt is None and (yuv is not None or full_range):
        raise ValueError(who + ": yuv= and full_range= need fmt \"nv12\" or \"i420\": a YUV layout is never inferred from a tensor")
    if fmt in YUVFMT:
        v, shape = _fmt_value(who, fmt, yuv, full_range), tuple(frames.shape)
        if not (frames.dtype == torch.uint8 and len(shape) == 3 and shape[1] % 3 == 0 and shape[2] % 2 == 0 and shape[1] > 0 and shape[2] > 0):
            raise ValueError(who + ": fmt %r does not fit a %s tensor of shape %s: uint8 [n, h * 3 / 2, w] with even h and w is needed"
                             % (fmt, frames.dtype, shape))
        if not frames.is_contiguous():
            raise ValueError(who + ": fmt %r needs a contiguous tensor (strides %s of shape %s)" % (fmt, frames.stride(), shape))
        return v, shape[0], shape[1] // 3 * 2, shape[2]
    if fmt is not None:
        _fmt_value(who, fmt, yuv, full_range)
    shape, packed = tuple(frames.shape), frames.element_size() == 4 and not frames.dtype.is_floating_point and not frames.dtype.is_complex
    if fmt is None:
        fits = []
        if packed and len(shape) == 3:
            fits.append("xrgb32")
        if frames.dtype == torch.uint8 and len(shape) == 4:
            fits += [name for name, ok in (("rgb24", shape[3] == 3), ("rgba32", shape[3] == 4), ("rgb8p", shape[1] == 3)) if ok]
        if len(fits) != 1:
            raise ValueError(who + ": fmt cannot be inferred from a %s tensor of shape %s (%s): pass fmt=" %
                             (frames.dtype, shape, "it fits " + " and ".join(fits) if fits else "int32/uint32 [n,h,w], uint8 [n,h,w,3|4] or uint8 [n,3,h,w] is needed"))
        fmt = fits[0]
    v = pixfmt(fmt)
    ok = (packed and len(shape) == 3) if v == 1 else (frames.dtype == torch.uint8 and len(shape) == 4 and
                                                      (shape[1] == 3 if v == 5 else shape[3] == (4 if v == 4 else 3)))
    if not ok:
        raise ValueError(who + ": fmt %r does not fit a %s tensor of shape %s" % (fmt, frames.dtype, shape))
    if not frames.is_contiguous():
        raise ValueError(who + ": fmt %r needs a contiguous tensor (strides %s of shape %s)" % (fmt, frames.stride(), shape))
    n, h, w = (shape[0], shape[2], shape[3]) if v == 5 else shape[:3]
    return v, n, h, w


def _tensor_dtypes():
    import torch
    return {1: torch.float32, 2: torch.float16, 3: torch.bfloat16}


def _tensor_clip(frames, fmt, mean, std, who):
    """(AGMV_TENSORFMT value, n, h, w, mean, std as ctypes float[3]) where the arguments name a tensor clip -- fmt one of TENSORFMT,
    or fmt None and a floating [n, 3, h, w] tensor -- else None, after refusing mean= / std= on any other layout.  Touches neither
    the library nor the device."""
    named = isinstance(fmt, str) and fmt in TENSORFMT
    shape = tuple(frames.shape) if frames is not None else None
    if not (named or (fmt is None and frames is not None and frames.dtype.is_floating_point and len(shape) == 4 and shape[1] == 3)):
        if mean is not None or std is not None:
            raise ValueError("%s: mean= and std= belong to the tensor layouts %s, not to fmt %r" % (who, ", ".join("\"%s\"" % k for k in sorted(TENSORFMT)), fmt))
        return None
    m, s = tensor_normalisation(who, 0.0 if mean is None else mean, 1.0 if std is None else std)
    if frames is None:
        return TENSORFMT[fmt], None, None, None, m, s
    v = {d: k for k, d in _tensor_dtypes().items()}.get(frames.dtype)
    if v is None or (named and v != TENSORFMT[fmt]) or len(shape) != 4 or shape[1] != 3:
        raise ValueError("%s: fmt %r does not fit a %s tensor of shape %s: float32, float16 or bfloat16 [n, 3, h, w] of the named type is needed"
                         % (who, fmt, frames.dtype, shape))
    if not frames.is_contiguous():
        raise ValueError("%s: fmt %r needs a contiguous tensor (strides %s of shape %s)" % (who, fmt, frames.stride(), shape))
    return v, shape[0], shape[2], shape[3], m, s


def _scale_target(size, scale):
    """(filter value, h, w) of encode_frames' size= and scale=, or None for size=None; touches neither the library nor the device"""
    if scale not in SCALE:
        raise ValueError("encode_frames: scale %r is unknown: one of %s is needed" % (scale, ", ".join("\"%s\"" % k for k in sorted(SCALE))))
    if size is None:
        if scale != "area":
            raise ValueError("encode_frames: scale=%r needs size=(h, w): without a target size nothing is scaled" % (scale,))
        return None
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size)):
        raise ValueError("encode_frames: size must be (h, w), two positive ints, got %r" % (size,))
    return SCALE[scale], size[0], size[1]


def _time_rate(rate, time):
    """the AGMV_RATE of encode_frames' rate= and time=, or None for rate=None; touches neither the library nor the device"""
    import math
    if not isinstance(time, str) or time not in TIME:
        raise ValueError("encode_frames: time %r is unknown: one of %s is needed" % (time, ", ".join("\"%s\"" % k for k in sorted(TIME))))
    if rate is None:
        if time != "area":
            raise ValueError("encode_frames: time=%r needs rate=(src, dst): without a rate nothing is resampled" % (time,))
        return None
    if not (isinstance(rate, (tuple, list)) and len(rate) == 2 and all(_is_int(v) and v >= 1 for v in rate)):
        raise ValueError("encode_frames: rate must be (src, dst), two ints of 1 or more, got %r" % (rate,))
    g = math.gcd(*rate)
    src, dst = rate[0] // g, rate[1] // g
    if src > 65535 or dst > 65535:
        raise ValueError("encode_frames: rate %r reduces to %d : %d, above 65535" % (tuple(rate), src, dst))
    if time == "area" and dst > src:
        raise ValueError("encode_frames: rate %r raises the frame rate, which time=\"area\" does not do: time=\"nearest\" duplicates frames" % (tuple(rate),))
    return abi.AGMV_RATE(rate[0], rate[1], TIME[time])


def _track_geometry(audio, sample_rate):
    """(AGMV_PCMFMT value, samples per channel, channels) of encode_frames' audio= tensor; touches neither the library nor the device"""
    import torch
    if not (isinstance(sample_rate, int) and not isinstance(sample_rate, bool) and sample_rate > 0):
        raise ValueError("encode_frames: audio= needs sample_rate=, a positive int, got %r" % (sample_rate,))
    shape = tuple(audio.shape)
    v = {torch.int16: 1, torch.uint8: 2, torch.float32: 3}.get(audio.dtype)
    if v is None or len(shape) != 2:
        raise ValueError("encode_frames: audio must be int16 [n, ch], uint8 [n, ch] or float32 [ch, n], got %s %s" % (audio.dtype, shape))
    if not audio.is_contiguous():
        raise ValueError("encode_frames: audio needs a contiguous tensor (strides %s of shape %s)" % (audio.stride(), shape))
    n, ch = (shape[1], shape[0]) if v == 3 else shape
    return v, n, ch


def encode_frames(path, frames, fps=24, opt=3, quality=3, compression=1, schedule=SCHEDULE_PDIFS, fmt=None, yuv=None, full_range=False,
                  size=None, scale="area", palette_refine=None, dither=None, audio=None, sample_rate=None, mean=None, std=None, stabilise=None,
                  select=None, crop=None, fit=None, rate=None, time="area"):
    """frames: contiguous CUDA tensor of n frames on the library's device, in the layout `fmt` (see the module text; None = inferred
    from the tensor, which never gives "nv12" or "i420") -> the file at `path`.  yuv ("bt601", the default, or "bt709") and
    full_range go with the two YUV layouts only.  size=(h, w), in tensor order, scales the clip to that size first
    (AGMV_EncodeFramesScaledDev): scale "area" is the exact box filter (a downscale), "nearest" the pixel under the target
    pixel's centre; the target must be multiples of 4, the source need not be.  palette_refine=n, an int from 1 to 64, moves the
    palette's colours by at most n rounds of weighted k-means over the clip's histogram (AGMV_SetPaletteRefine of include/agmv.h,
    set for this call only); None leaves the library's knob as it is.  dither=s, an int from 1 to 64, pattern-dithers the frames
    against the palette with that strength before they are quantised (AGMV_SetDither of include/agmv.h, which holds the
    definition; set for this call only); None leaves the library's knob as it is.  stabilise=s, an int from 1 to 64, gives the
    blocks of a P-frame that differ from their GOP's I-frame by no more than that strength allows the I-frame's pixels, before the
    dither (AGMV_SetStabilise of include/agmv.h, which holds the rule; set for this call only; stabilise_stats() says what it did);
    None leaves the library's knob as it is.  audio= is the clip's sound, a contiguous CUDA
    tensor on the same device -- int16 [n, ch], uint8 [n, ch] or float32 [ch, n] (see the module text) -- at sample_rate= samples
    per second; it is companded on the GPU and interleaved with the frames as AGAC chunks (AGMV_SetAudioDev, for this call only).
    A track shorter than one second and SCHEDULE_ADAPTIVE with a track are refused.
    A float32 / float16 / bfloat16 [n, 3, h, w] tensor (fmt "f32" / "f16" / "bf16", or inferred from the dtype) is a normalised
    tensor clip, model output as it is: mean= and std= (a number or three per channel; defaults 0 and 1) say what its values
    stand for, and the file is that of the XRGB32 clip the reading rule of include/agmv.h gives (AGMV_EncodeFramesTensorDev).
    yuv=, full_range= and size= do not go with a tensor clip; mean= and std= go with nothing else.
    select=, crop= and fit= encode a view of the clip (AGMV_EncodeViewDev of include/agmv.h) without a copy of the selection: select is
    a range, a slice (resolved against the clip's length) or a tuple (start, stop, step), steps >= 1 only, as decode_frames(frames=)
    takes them; crop=(top, left, height, width), in tensor order, is a window of every frame, which must lie inside it -- anywhere,
    odd offsets and sizes included, for "nv12" and "i420" too; fit="crop" needs size= and no crop= and takes fit_window() of the
    frame and the target, the largest centred window of the target's aspect.  The file is that of the contiguous XRGB32 clip of the
    selected windows, scaled to size= where that is given; fps is written as given.  An empty selection is refused, and none of
    the three goes with a tensor clip.  encode_view_stats() says what the call materialised.
    rate=(src, dst) encodes the clip -- or the view select=, crop=, fit= and size= describe -- at another frame rate
    (AGMV_EncodeViewRateDev of include/agmv.h, which holds the rule): src frames become dst frames, 60 fps to 24 is rate=(5, 2).
    time "area", the default, is the exact box filter in time and only lowers the rate; "nearest" takes the frame under each
    target interval's centre and may also duplicate frames.  The two values are reduced by their gcd and must then be at most 65535.
    The file is that of the resampled XRGB32 clip; fps is written as given.  time= needs rate=, and rate= does not go with a tensor
    clip.  encode_rate_stats() says how many frames went in and came out."""
    import torch
    select, crop = _decode_selection(select, crop, who="encode_frames", name="select")
    if fit is not None and not (fit == "crop" and size is not None and crop is None):
        raise ValueError("encode_frames: fit must be None or \"crop\", which needs size=(h, w) and no crop=, got fit=%r, size=%r, crop=%r" % (fit, size, crop))
    if dither is not None and not (isinstance(dither, int) and not isinstance(dither, bool) and 1 <= dither <= 64):
        raise ValueError("encode_frames: dither must be None or an int from 1 to 64, got %r" % (dither,))
    if stabilise is not None and not (isinstance(stabilise, int) and not isinstance(stabilise, bool) and 1 <= stabilise <= 64):
        raise ValueError("encode_frames: stabilise must be None or an int from 1 to 64, got %r" % (stabilise,))
    if palette_refine is not None and not (isinstance(palette_refine, int) and not isinstance(palette_refine, bool) and 1 <= palette_refine <= 64):
        raise ValueError("encode_frames: palette_refine must be None or an int from 1 to 64, got %r" % (palette_refine,))
    target = _scale_target(size, scale)
    rated = _time_rate(rate, time)
    tensor = _tensor_clip(frames, fmt, mean, std, "encode_frames")
    if tensor is not None:
        if rated is not None:
            raise ValueError("encode_frames: rate= does not go with a tensor clip (fmt %r)" % (fmt,))
        if yuv is not None or full_range or target is not None:
            raise ValueError("encode_frames: yuv=, full_range= and size= do not go with a tensor clip (fmt %r)" % (fmt,))
        if select is not None or crop is not None or fit is not None:
            raise ValueError("encode_frames: select=, crop= and fit= do not go with a tensor clip (fmt %r)" % (fmt,))
        v, n, h, w = tensor[:4]
    else:
        v, n, h, w = _clip_geometry(frames, fmt, yuv, full_range)
    view = None
    if select is not None or crop is not None or fit is not None:
        sel = _resolve_selection(select, n)
        if len(sel) == 0:
            raise ValueError("encode_frames: select=%r takes no frame of a clip of %d" % (select, n))
        if fit is not None:
            crop = fit_window(h, w, target[1], target[2])
        view = abi.AGMV_VIEW(sel.start, len(sel), sel.step, 0, 0, 0, 0)
        if crop is not None:
            top, left, ch, cw = crop
            if top + ch > h or left + cw > w:
                raise ValueError("encode_frames: crop %r does not lie inside the %d x %d frames of the clip" % (tuple(crop), w, h))
            view.x, view.y, view.width, view.height = left, top, cw, ch
    track = None
    if audio is not None:
        track = _track_geometry(audio, sample_rate)
    elif sample_rate is not None:
        raise ValueError("encode_frames: sample_rate= goes with audio=")
    if not (frames.is_cuda and frames.device == torch.device(_device())):
        raise ValueError("encode_frames: the frames must be on %s, got %s" % (_device(), frames.device))
    if audio is not None and not (audio.is_cuda and audio.device == torch.device(_device())):
        raise ValueError("encode_frames: the audio must be on %s, got %s" % (_device(), audio.device))
    torch.cuda.synchronize(frames.device)          # the library works on streams of its own
    L = load_library()
    if track is not None:
        rc = L.AGMV_SetAudioDev(audio.data_ptr(), track[0], track[1], sample_rate, track[2])
        if rc:
            raise ValueError("AGMV_SetAudioDev refused the track (%d): %d samples in %d channels at %d Hz" % (rc, track[1], track[2], sample_rate))
    if palette_refine is not None:
        L.AGMV_SetPaletteRefine(palette_refine)
    if dither is not None:
        L.AGMV_SetDither(dither)
    if stabilise is not None:
        L.AGMV_SetStabilise(stabilise)
    try:
        if tensor is not None:
            rc = L.AGMV_EncodeFramesTensorDev(os.fsencode(path), frames.data_ptr(), v, tensor[4], tensor[5], n, w, h, fps, opt, quality, compression, schedule)
            if rc:
                raise ValueError("AGMV_EncodeFramesTensorDev refused its arguments (%d): %d frames of %dx%d, mean %r, std %r, opt %d, schedule %d"
                                 % (rc, n, w, h, mean, std, opt, schedule))
            return
        if rated is not None:
            filt, th, tw = target if target is not None else (0, 0, 0)
            rc = L.AGMV_EncodeViewRateDev(os.fsencode(path), frames.data_ptr(), v, n, w, h, C.byref(view) if view is not None else None, C.byref(rated), tw, th, filt,
                                          fps, opt, quality, compression, schedule)
            if rc:
                raise ValueError("AGMV_EncodeViewRateDev refused its arguments (%d): %d frames of %dx%d, rate %r (%s), select %r, crop %r, size %r (%s), opt %d, schedule %d"
                                 % (rc, n, w, h, tuple(rate), time, select, crop, size, scale, opt, schedule))
            return
        if view is not None:
            filt, th, tw = target if target is not None else (0, 0, 0)
            rc = L.AGMV_EncodeViewDev(os.fsencode(path), frames.data_ptr(), v, n, w, h, C.byref(view), tw, th, filt, fps, opt, quality, compression, schedule)
            if rc:
                raise ValueError("AGMV_EncodeViewDev refused its arguments (%d): %d frames of %dx%d, select %r, crop %r, size %r (%s), opt %d, schedule %d"
                                 % (rc, n, w, h, sel, crop, size, scale, opt, schedule))
            return
        if target is None:
            rc = L.AGMV_EncodeFramesFmtDev(os.fsencode(path), frames.data_ptr(), v, n, w, h, fps, opt, quality, compression, schedule)
            if rc:
                raise ValueError("AGMV_EncodeFramesFmtDev refused its arguments (%d): %d frames of %dx%d, opt %d, schedule %d" % (rc, n, w, h, opt, schedule))
            return
        filt, th, tw = target
        rc = L.AGMV_EncodeFramesScaledDev(os.fsencode(path), frames.data_ptr(), v, n, w, h, tw, th, filt, fps, opt, quality, compression, schedule)
        if rc:
            raise ValueError("AGMV_EncodeFramesScaledDev refused its arguments (%d): %d frames of %dx%d scaled (%s) to %dx%d, opt %d, schedule %d"
                             % (rc, n, w, h, scale, tw, th, opt, schedule))
    finally:
        if track is not None:
            L.AGMV_SetAudioDev(None, 0, 0, 0, 0)
        if palette_refine is not None:
            L.AGMV_SetPaletteRefine(0)
        if dither is not None:
            L.AGMV_SetDither(0)
        if stabilise is not None:
            L.AGMV_SetStabilise(0)


def stabilise_stats():
    """(examined, replaced) of the last sequence encode of this process (AGMV_GetStabiliseStats of include/agmv.h): the blocks of the
    P-frames that had their GOP's I-frame in their batch, and those the temporal stabilisation replaced; (0, 0) when it was off"""
    st = abi.AGMV_STABILISE_STATS()
    load_library().AGMV_GetStabiliseStats(C.byref(st))
    return int(st.examined), int(st.replaced)


def encode_view_stats():
    """(frames, clip_bytes, staging_bytes) of the last encode_frames(select= / crop= / fit=) of this process (AGMV_GetEncodeViewStats of
    include/agmv.h): the frames encoded, the bytes of the XRGB32 clip the call materialised (0 where the source was encoded in
    place) and of its staging batch (0 without one); all 0 behind a refused call"""
    st = abi.AGMV_ENCODE_VIEW_STATS()
    load_library().AGMV_GetEncodeViewStats(C.byref(st))
    return int(st.frames), int(st.clip_bytes), int(st.staging_bytes)


def encode_rate_stats():
    """(frames_in, frames_out, frame_reads) of the last encode_frames(rate=) of this process (AGMV_GetEncodeRateStats of include/agmv.h):
    the length of the view, the frames of the file, and the source frames read, one per tap with a weight above 0; all 0 behind a
    refused call"""
    st = abi.AGMV_ENCODE_RATE_STATS()
    load_library().AGMV_GetEncodeRateStats(C.byref(st))
    return int(st.frames_in), int(st.frames_out), int(st.frame_reads)


def _decode_target(size, scale):
    """(filter value, h, w) of decode_frames' size= and scale=, or None for size=None; touches neither the library nor the device"""
    if not isinstance(scale, str) or scale not in DECODE_SCALE:
        raise ValueError("decode_frames: scale %r is unknown: one of %s is needed" % (scale, ", ".join("\"%s\"" % k for k in sorted(DECODE_SCALE))))
    if size is None:
        if scale != "bilinear":
            raise ValueError("decode_frames: scale=%r needs size=(h, w): without a target size nothing is scaled" % (scale,))
        return None
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size)):
        raise ValueError("decode_frames: size must be (h, w), two positive ints, got %r" % (size,))
    return DECODE_SCALE[scale], size[0], size[1]


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _decode_selection(frames, crop, who="decode_frames", name="frames"):
    """decode_frames' frames= (encode_frames' select=) and crop= checked, in the name of the caller `who` -> (a range or a slice or None,
    crop); touches neither the library nor the device"""
    if isinstance(frames, tuple):
        if not (len(frames) == 3 and all(_is_int(v) for v in frames) and frames[2] >= 1):
            raise ValueError("%s: %s as a tuple must be (start, stop, step), three ints with step >= 1, got %r" % (who, name, frames))
        frames = range(*frames)
    if isinstance(frames, range):
        if frames.step < 1 or frames.start < 0:
            raise ValueError("%s: %s must start at 0 or later and step forwards, got %r" % (who, name, frames))
    elif isinstance(frames, slice):
        if not (all(v is None or _is_int(v) for v in (frames.start, frames.stop, frames.step)) and (frames.step is None or frames.step >= 1)):
            raise ValueError("%s: %s as a slice needs ints and a step >= 1, got %r" % (who, name, frames))
    elif frames is not None:
        raise ValueError("%s: %s must be a range, a slice or a tuple (start, stop, step), got %r" % (who, name, frames))
    if crop is not None and not (isinstance(crop, (tuple, list)) and len(crop) == 4 and all(_is_int(v) for v in crop)
                                 and crop[0] >= 0 and crop[1] >= 0 and crop[2] > 0 and crop[3] > 0):
        raise ValueError("%s: crop must be (top, left, height, width), four ints with a height and a width above 0, got %r" % (who, crop))
    return frames, crop


def _resolve_selection(sel, n):
    """a checked selection against a clip or file of n frames -> the range of the frames it takes"""
    return range(n) if sel is None else range(*sel.indices(n)) if isinstance(sel, slice) else range(sel.start, min(sel.stop, n), sel.step)


def fit_window(src_h, src_w, h, w):
    """(top, left, height, width) of the largest centred window of a src_h x src_w frame that has the aspect of an h x w target, in
    integers (`//` on non-negative ints): the full height where the source is the wider of the two, else the full width.  What
    encode_frames(fit="crop") takes; touches neither the library nor the device."""
    if not all(_is_int(v) and v > 0 for v in (src_h, src_w, h, w)):
        raise ValueError("fit_window: four positive ints are needed, got %r" % ((src_h, src_w, h, w),))
    if src_w * h >= src_h * w:
        ch, cw = src_h, src_h * w // h
    else:
        cw, ch = src_w, src_w * h // w
    if ch == 0 or cw == 0:
        raise ValueError("fit_window: a %d x %d frame holds no window of the aspect of %d x %d" % (src_w, src_h, w, h))
    return (src_h - ch) // 2, (src_w - cw) // 2, ch, cw


def _decode_view(path, v, tensor, target, scale, frames, crop, fmt):
    """decode_frames with frames= or crop=: AGMV_DecodeViewDev, or for a tensor clip (`tensor` of _tensor_clip) AGMV_DecodeViewTensorDev"""
    import torch
    L = load_library()
    info = AGMV_INFO()
    if tensor is not None:
        v, m, s = tensor[0], tensor[4], tensor[5]
        call, head = "AGMV_DecodeViewTensorDev", lambda dst, *rest: L.AGMV_DecodeViewTensorDev(os.fsencode(path), dst, v, m, s, *rest)
    else:
        call, head = "AGMV_DecodeViewDev", lambda dst, *rest: L.AGMV_DecodeViewDev(os.fsencode(path), dst, v, *rest)
    rc = head(None, 0, 0, 0, None, 0, C.byref(info))
    if rc < 0:
        raise (ValueError if rc == -1 else RuntimeError)("%s(%s): %s" % (call, path, "the normalisation is refused" if rc == -1 else "Error %d" % -rc))
    n, h, w = info.number_of_frames, info.height, info.width
    sel = _resolve_selection(frames, n)
    view = abi.AGMV_VIEW(sel.start if len(sel) else 0, len(sel), sel.step, 0, 0, 0, 0)
    if crop is not None:
        top, left, ch, cw = crop
        if top + ch > h or left + cw > w:
            raise ValueError("decode_frames: crop %r does not lie inside the %d x %d frames of %s" % (tuple(crop), w, h, path))
        view.x, view.y, view.width, view.height = left, top, cw, ch
        h, w = ch, cw
    filt, tw, th = 0, 0, 0
    if target is not None:
        filt, th, tw = target
        if filt == DECODE_SCALE["area"] and (th > h or tw > w):
            raise ValueError("decode_frames: scale=\"area\" only scales down, the frames taken from %s are %d x %d and size= asks for %d x %d" % (path, w, h, tw, th))
        h, w = th, tw
    if tensor is not None:
        shape, dtype = (len(sel), 3, h, w), _tensor_dtypes()[v]
    else:
        if v & 0xFF in YUVFMT.values() and (h % 2 or w % 2):
            raise ValueError("decode_frames: fmt %r needs frames of even width and height, got %d x %d" % (fmt, w, h))
        k = len(sel)
        shape = {1: (k, h, w), 2: (k, h, w, 3), 3: (k, h, w, 3), 4: (k, h, w, 4), 5: (k, 3, h, w), 16: (k, h * 3 // 2, w), 17: (k, h * 3 // 2, w)}[v & 0xFF]
        dtype = torch.int32 if v == 1 else torch.uint8
    out = torch.empty(shape, dtype=dtype, device=_device())
    if len(sel) == 0:
        return out, info
    rc = head(out.data_ptr(), tw, th, filt, C.byref(view), len(sel), None)
    if rc < 0:
        raise RuntimeError("%s(%s, frames %r, crop %r, %d x %d, scale %r): Error %d" % (call, path, sel, crop, w, h, scale, -rc))
    return out[:rc], info


@contextlib.contextmanager
def _deblock_for_this_call(who, deblock):
    """AGMV_SetDeblock(deblock) around one decode, reset in a finally; anything but None or an int from 1 to 64 raises before the
    library is touched"""
    if deblock is not None and not (isinstance(deblock, int) and not isinstance(deblock, bool) and 1 <= deblock <= 64):
        raise ValueError("%s: deblock must be None or an int from 1 to 64, got %r" % (who, deblock))
    if deblock is None:
        yield
        return
    L = load_library()
    L.AGMV_SetDeblock(deblock)
    try:
        yield
    finally:
        L.AGMV_SetDeblock(0)


def deblock_stats():
    """what the deblocking did in the last sequence decode of this process (AGMV_GetDeblockStats of include/agmv.h) as a dict:
    strength, frames filtered, lines examined, weak and strong lines; all zero when it was off"""
    st = abi.AGMV_DEBLOCK_STATS()
    load_library().AGMV_GetDeblockStats(C.byref(st))
    return {"strength": int(st.strength), "frames": int(st.frames), "lines": int(st.lines), "weak": int(st.weak), "strong": int(st.strong)}


def decode_frames(path, fmt="xrgb32", yuv=None, full_range=False, size=None, scale="bilinear", mean=None, std=None, frames=None, crop=None, deblock=None):
    """-> (CUDA tensor of the file's frames on the library's device in the layout `fmt`: int32 [n, h, w] of 0x00RRGGBB for "xrgb32",
    uint8 [n, h, w, 3] / [n, h, w, 4] / [n, 3, h, w] for the byte formats, uint8 [n, h * 3 / 2, w] for "nv12" and "i420" (a file
    of even width and height; yuv and full_range as for encode_frames); AGMV_INFO of the header).  size=(h, w), in tensor order,
    delivers the frames at that size instead of the file's (AGMV_DecodeFramesScaledDev of include/agmv.h, which defines the
    filters): scale "bilinear" (the default) and "nearest" take any size in either direction, "area" is the exact box filter and
    only scales down.  The tensor then has the layout's shape at (h, w) -- even h and w for the two YUV layouts, whatever the
    file's size -- and the AGMV_INFO still carries the file's own size.
    fmt "f32" / "f16" / "bf16" gives a model's input: a float32 / float16 / bfloat16 [n, 3, h, w] tensor, every byte v of channel
    c as (v / 255 - mean[c]) / std[c] (mean= and std=: a number or three; defaults 0 and 1), written by the sink in the same
    launch that scales (AGMV_DecodeFramesTensorDev of include/agmv.h: exact, through a table).
    frames= and crop= decode a view of the file (AGMV_DecodeViewDev / AGMV_DecodeViewTensorDev of include/agmv.h): frames is a range,
    a slice (resolved against the file's frame count) or a tuple (start, stop, step), steps >= 1 only; crop=(top, left, height, width),
    in tensor order, is a window of every frame, which must lie inside it.  Frame j of the result is the window of frame
    frames[j] of the full decode; layout, size=, scale= and the normalisation apply to the window as to a file of that size, and the
    tensor holds as many frames as the selection has inside the file -- none, without a decode, for an empty one.
    deblock=s, an int from 1 to 64, smooths the edges of the 4x4 block grid of every decoded frame with that strength before the
    layout, the view and the scaling see it (AGMV_SetDeblock of include/agmv.h, which holds the rule; set for this call only;
    deblock_stats() says what it did); None leaves the library's knob as it is."""
    with _deblock_for_this_call("decode_frames", deblock):
        return _decode_frames(path, fmt, yuv, full_range, size, scale, mean, std, frames, crop)


def _decode_frames(path, fmt, yuv, full_range, size, scale, mean, std, frames, crop):
    import torch
    target = _decode_target(size, scale)
    tensor = _tensor_clip(None, fmt, mean, std, "decode_frames")
    frames, crop = _decode_selection(frames, crop)
    if tensor is not None:
        if yuv is not None or full_range:
            raise ValueError("decode_frames: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (fmt,))
        if frames is not None or crop is not None:
            return _decode_view(path, None, tensor, target, scale, frames, crop, fmt)
        return _decode_tensor(path, tensor, target, scale)
    v = _fmt_value("decode_frames", fmt, yuv, full_range)
    if frames is not None or crop is not None:
        return _decode_view(path, v, None, target, scale, frames, crop, fmt)
    L = load_library()
    info = AGMV_INFO()
    rc = L.AGMV_DecodeFramesFmtDev(os.fsencode(path), None, v, 0, C.byref(info))
    if rc < 0:
        raise RuntimeError("AGMV_DecodeFramesFmtDev(%s): Error %d" % (path, -rc))
    n, h, w = info.number_of_frames, info.height, info.width
    if target is not None:
        filt, th, tw = target
        if filt == DECODE_SCALE["area"] and (th > h or tw > w):
            raise ValueError("decode_frames: scale=\"area\" only scales down, %s holds %d x %d and size= asks for %d x %d" % (path, w, h, tw, th))
        h, w = th, tw
    if v & 0xFF in YUVFMT.values() and (h % 2 or w % 2):
        raise ValueError("decode_frames: fmt %r needs %s of even width and height, %s %d x %d"
                         % (fmt, "a file" if target is None else "a target", ("%s holds" % path) if target is None else "size= asks for", w, h))
    shape = {1: (n, h, w), 2: (n, h, w, 3), 3: (n, h, w, 3), 4: (n, h, w, 4), 5: (n, 3, h, w), 16: (n, h * 3 // 2, w), 17: (n, h * 3 // 2, w)}[v & 0xFF]
    out = torch.empty(shape, dtype=torch.int32 if v == 1 else torch.uint8, device=_device())
    if target is None:
        rc = L.AGMV_DecodeFramesFmtDev(os.fsencode(path), out.data_ptr(), v, n, None)
        if rc < 0:
            raise RuntimeError("AGMV_DecodeFramesFmtDev(%s): Error %d" % (path, -rc))
        return out[:rc], info
    rc = L.AGMV_DecodeFramesScaledDev(os.fsencode(path), out.data_ptr(), v, w, h, filt, n, None)
    if rc < 0:
        raise RuntimeError("AGMV_DecodeFramesScaledDev(%s, %d x %d, scale %r): Error %d" % (path, w, h, scale, -rc))
    return out[:rc], info


def _decode_tensor(path, tensor, target, scale):
    """decode_frames for a tensor clip: (AGMV_TENSORFMT value, -, -, -, mean, std) of _tensor_clip, target of _decode_target"""
    import torch
    v, m, s = tensor[0], tensor[4], tensor[5]
    L = load_library()
    info = AGMV_INFO()
    rc = L.AGMV_DecodeFramesTensorDev(os.fsencode(path), None, v, m, s, 0, 0, 0, 0, C.byref(info))
    if rc < 0:
        raise (ValueError if rc == -1 else RuntimeError)("AGMV_DecodeFramesTensorDev(%s): %s" % (path, "the normalisation is refused" if rc == -1 else "Error %d" % -rc))
    n, h, w = info.number_of_frames, info.height, info.width
    filt, tw, th = 0, 0, 0
    if target is not None:
        filt, th, tw = target
        if filt == DECODE_SCALE["area"] and (th > h or tw > w):
            raise ValueError("decode_frames: scale=\"area\" only scales down, %s holds %d x %d and size= asks for %d x %d" % (path, w, h, tw, th))
        h, w = th, tw
    out = torch.empty((n, 3, h, w), dtype=_tensor_dtypes()[v], device=_device())
    rc = L.AGMV_DecodeFramesTensorDev(os.fsencode(path), out.data_ptr(), v, m, s, tw, th, filt, n, None)
    if rc < 0:
        raise RuntimeError("AGMV_DecodeFramesTensorDev(%s, %d x %d, scale %r): Error %d" % (path, w, h, scale, -rc))
    return out[:rc], info


class Reader:
    """A file opened once and read in pieces with the decoder's state kept (include/agmv_reader.h, which holds the contract): what
    decode_frames(path, ..., frames=range(p, p + n * step, step), crop=crop) returns for every read of n frames at position p, without
    the call's fixed cost and without the LZ stage from frame 0 each time.  fmt, yuv, full_range, size, scale, mean, std, crop and
    deblock are decode_frames' and are checked by the same code; step is the stride of the frames a read takes; index_bytes is the
    budget of the seek index (None: 64 MiB).  Everything the reader holds on the device is allocated here; a read allocates its
    result, or nothing with out=.
        with Reader(path, fmt="f16", crop=(0, 0, 224, 224)) as r:
            for batch in r.batches(16):
                ...
    len() is the file's frame count, .info its AGMV_INFO, .tell() the file frame the next read starts at, .seek(f) moves there,
    .stats() is AGMV_READER_STATS as a dict.  A closed reader raises ValueError."""

    def __init__(self, path, fmt="xrgb32", yuv=None, full_range=False, size=None, scale="bilinear", mean=None, std=None, step=1, crop=None,
                 deblock=None, index_bytes=None):
        self._h = None
        target = _decode_target(size, scale)
        tensor = _tensor_clip(None, fmt, mean, std, "Reader")
        _, crop = _decode_selection(None, crop, who="Reader")
        if not (_is_int(step) and step >= 1):
            raise ValueError("Reader: step must be an int >= 1, got %r" % (step,))
        if index_bytes is not None and not (_is_int(index_bytes) and index_bytes >= 1):
            raise ValueError("Reader: index_bytes must be None or an int >= 1, got %r" % (index_bytes,))
        d = abi.AGMV_READER_DESC(step=step, index_bytes=index_bytes or 0)
        if tensor is not None:
            if yuv is not None or full_range:
                raise ValueError("Reader: yuv= and full_range= belong to fmt \"nv12\" and \"i420\", not to fmt %r" % (fmt,))
            d.tensor, d.type, d.mean, d.std = 1, tensor[0], tensor[4], tensor[5]
        else:
            v = _fmt_value("Reader", fmt, yuv, full_range)
            d.fmt, d.yuv_flags = v & 0xFF, v & ~0xFF
        with _deblock_for_this_call("Reader", deblock):          # (the argument check; the strength itself travels in the description)
            pass
        d.deblock = deblock or 0
        if target is not None:
            d.filter, d.height, d.width = target
        if crop is not None:
            d.y, d.x, d.win_height, d.win_width = crop
        info, err = AGMV_INFO(), C.c_int(0)
        L = load_library()
        h = L.AGMV_OpenReaderDev(os.fsencode(path), C.byref(d), C.byref(info), C.byref(err))
        if not h:
            raise (ValueError if err.value in (-1, -4) else RuntimeError)(
                "AGMV_OpenReaderDev(%s, fmt %r, size %r (%s), step %d, crop %r): %s" % (path, fmt, size, scale, step, crop, {
                    -1: "the arguments are refused", -4: "the file's frames refuse the window or the target"}.get(err.value, "Error %d" % -err.value)))
        self._L, self._h, self.info, self.path = L, h, info, path
        fh, fw = (crop[2], crop[3]) if crop is not None else (info.height, info.width)
        if target is not None:
            fh, fw = target[1], target[2]
        if tensor is not None:
            self._frame, self._dtype = (3, fh, fw), _tensor_dtypes()[tensor[0]]
        else:
            import torch
            k = d.fmt
            self._frame = {1: (fh, fw), 2: (fh, fw, 3), 3: (fh, fw, 3), 4: (fh, fw, 4), 5: (3, fh, fw), 16: (fh * 3 // 2, fw), 17: (fh * 3 // 2, fw)}[k]
            self._dtype = torch.int32 if k == 1 else torch.uint8
        self.step = step

    def _handle(self):
        if self._h is None:
            raise ValueError("Reader: the reader is closed")
        return self._h

    def __len__(self):
        return int(self.info.number_of_frames)

    def tell(self):
        return int(self._L.AGMV_ReaderTell(self._handle()))

    def seek(self, frame):
        if not (_is_int(frame) and frame >= 0):
            raise ValueError("Reader.seek: a frame index, an int >= 0, is needed, got %r" % (frame,))
        self._L.AGMV_ReaderSeek(self._handle(), min(frame, 0xFFFFFFFF))

    def read(self, n, out=None):
        """the next (at most) n frames as a tensor of exactly the frames delivered, none at the file's end; out=, a contiguous tensor
        of the reader's dtype on the library's device whose frames have the reader's shape, receives them instead, and the slice
        of it that holds them is returned"""
        import torch
        h = self._handle()
        if not (_is_int(n) and n >= 0):
            raise ValueError("Reader.read: n must be an int >= 0, got %r" % (n,))
        left = len(range(min(self.tell(), len(self)), len(self), self.step))
        if out is None:
            n = min(n, left)
            out = torch.empty((n,) + self._frame, dtype=self._dtype, device=_device())
        else:
            if not (out.is_cuda and out.device == torch.device(_device()) and out.dtype == self._dtype and tuple(out.shape[1:]) == self._frame
                    and out.is_contiguous()):
                raise ValueError("Reader.read: out must be a contiguous %s tensor [n, %s] on %s, got %s %s on %s"
                                 % (self._dtype, ", ".join(map(str, self._frame)), _device(), out.dtype, tuple(out.shape), out.device))
            n = min(n, out.shape[0])
            torch.cuda.synchronize(out.device)         # the library works on streams of its own
        if n == 0:
            return out[:0]
        rc = self._L.AGMV_ReaderReadDev(h, out.data_ptr(), n)
        if rc < 0:
            raise RuntimeError("AGMV_ReaderReadDev(%s, %d frames at %d): Error %d" % (self.path, n, self.tell(), -rc))
        return out[:rc]

    def batches(self, n):
        """the reads of n frames from the current position to the file's end, one after the other"""
        while True:
            got = self.read(n)
            if got.shape[0] == 0:
                return
            yield got

    def stats(self):
        st = abi.AGMV_READER_STATS()
        self._L.AGMV_GetReaderStats(self._handle(), C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in abi.AGMV_READER_STATS._fields_}

    def close(self):
        if self._h is not None:
            self._L.AGMV_CloseReader(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class Writer:
    """A clip encoded in pieces into the file encode_frames writes for the whole of it (include/agmv_writer.h, which holds the contract):
    every frame is handed in twice, first to .analyse(frames), which counts it towards the palette, then to .write(frames), which
    encodes it; the pieces may have any sizes, may come from one reused buffer, and nothing of them is held after a call returns.
    height and width are those of the frames handed in; fps, opt, quality, compression, fmt, yuv, full_range, size, scale, mean and
    std are encode_frames' and are checked the same way (fmt is named, not inferred: there is no tensor to look at yet); schedule is
    SCHEDULE_FULL or SCHEDULE_PDIFS.  palette_refine, dither and stabilise are set for the open, where the writer reads them, and
    restored after it.  ring_frames is the staging capacity in frames (None: the library's choice; a request below the minimum is
    raised to it).  Analysing only a sample is legal: the palette is then the sample's.
        with Writer(path, 1080, 1920, fmt="nv12") as w:
            for chunk in source(): w.analyse(chunk)
            for chunk in source(): w.write(chunk)
    .close() finishes the file and returns the frames written (a with block closes); .stats() is AGMV_WRITER_STATS as a dict.  A closed
    writer raises ValueError."""

    def __init__(self, path, height, width, fps=24, opt=3, quality=3, compression=1, schedule=SCHEDULE_FULL, fmt="xrgb32", yuv=None, full_range=False,
                 size=None, scale="area", mean=None, std=None, palette_refine=None, dither=None, stabilise=None, ring_frames=None):
        self._h = None
        for name, v in (("palette_refine", palette_refine), ("dither", dither), ("stabilise", stabilise)):
            if v is not None and not (_is_int(v) and 1 <= v <= 64):
                raise ValueError("Writer: %s must be None or an int from 1 to 64, got %r" % (name, v))
        if not (_is_int(height) and _is_int(width) and height > 0 and width > 0):
            raise ValueError("Writer: height and width must be positive ints, got %r and %r" % (height, width))
        if ring_frames is not None and not (_is_int(ring_frames) and ring_frames >= 1):
            raise ValueError("Writer: ring_frames must be None or an int >= 1, got %r" % (ring_frames,))
        if schedule not in (SCHEDULE_FULL, SCHEDULE_PDIFS):
            raise ValueError("Writer: schedule must be SCHEDULE_FULL or SCHEDULE_PDIFS (SCHEDULE_ADAPTIVE compares frames a writer has not seen together), got %r" % (schedule,))
        target = _scale_target(size, scale)
        tensor = _tensor_clip(None, fmt, mean, std, "Writer")
        d = abi.AGMV_WRITER_DESC(src_width=width, src_height=height, frames_per_second=fps, opt=opt, quality=quality, compression=compression,
                                 schedule=schedule, ring_frames=ring_frames or 0)
        if tensor is not None:
            if yuv is not None or full_range or target is not None:
                raise ValueError("Writer: yuv=, full_range= and size= do not go with a tensor clip (fmt %r)" % (fmt,))
            d.tensor, d.type, d.mean, d.std = 1, tensor[0], tensor[4], tensor[5]
        else:
            v = _fmt_value("Writer", fmt, yuv, full_range)
            d.fmt, d.yuv_flags = v & 0xFF, v & ~0xFF
        if target is not None:
            d.filter, d.height, d.width = target
        self._fmt, self._yuv, self._full_range, self._mean, self._std, self._tensor = fmt, yuv, full_range, mean, std, tensor
        self._value, self._hw, self.path = (tensor[0] if tensor is not None else d.fmt | d.yuv_flags), (height, width), path
        L = load_library()
        err = C.c_int(0)
        knobs = ((L.AGMV_SetPaletteRefine, palette_refine), (L.AGMV_SetDither, dither), (L.AGMV_SetStabilise, stabilise))
        for call, v in knobs:
            if v is not None:
                call(v)
        try:
            h = L.AGMV_OpenWriterDev(os.fsencode(path), C.byref(d), C.byref(err))
        finally:
            for call, v in knobs:
                if v is not None:
                    call(0)
        if not h:
            raise ValueError("AGMV_OpenWriterDev refused its arguments (%d): frames of %dx%d, fmt %r, size %r (%s), opt %d, schedule %d"
                             % (err.value, width, height, fmt, size, scale, opt, schedule))
        self._L, self._h = L, h

    def _handle(self):
        if self._h is None:
            raise ValueError("Writer: the writer is closed")
        return self._h

    def _frames(self, who, frames):
        """the number of frames of a piece, checked against the writer's layout and size; the piece must be complete when called"""
        import torch
        h = self._handle()
        if self._tensor is not None:
            v, n, fh, fw = _tensor_clip(frames, self._fmt, self._mean, self._std, who)[:4]
        else:
            v, n, fh, fw = _clip_geometry(frames, self._fmt, self._yuv, self._full_range, who=who)
        if (v, fh, fw) != (self._value,) + self._hw:
            raise ValueError("%s: the writer takes frames of %dx%d in fmt %r, got %dx%d" % (who, self._hw[1], self._hw[0], self._fmt, fw, fh))
        if not (frames.is_cuda and frames.device == torch.device(_device())):
            raise ValueError("%s: the frames must be on %s, got %s" % (who, _device(), frames.device))
        torch.cuda.synchronize(frames.device)          # the library works on streams of its own
        return h, n

    def analyse(self, frames):
        """pass 1: these frames count towards the palette; refused once a write has frozen it"""
        h, n = self._frames("Writer.analyse", frames)
        rc = self._L.AGMV_WriterAnalyseDev(h, frames.data_ptr(), n)
        if rc:
            raise ValueError("AGMV_WriterAnalyseDev(%s, %d frames): %s" % (self.path, n, {-6: "the first write has frozen the palette"}.get(rc, "refused (%d)" % rc)))

    def write(self, frames):
        """pass 2: these frames are the next of the clip; returns once they are in the writer's staging"""
        h, n = self._frames("Writer.write", frames)
        rc = self._L.AGMV_WriterWriteDev(h, frames.data_ptr(), n)
        if rc:
            raise ValueError("AGMV_WriterWriteDev(%s, %d frames): %s" % (self.path, n, {-6: "nothing has been analysed: there is no palette"}.get(rc, "refused (%d)" % rc)))

    def stats(self):
        st = abi.AGMV_WRITER_STATS()
        self._L.AGMV_GetWriterStats(self._handle(), C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in abi.AGMV_WRITER_STATS._fields_}

    def close(self):
        """finishes the file and returns the frames written; a clip shorter than the schedule's first group (AGMV_CloseWriter's -2) leaves
        no file and raises ValueError.  A second close returns None."""
        if self._h is None:
            return None
        h, self._h = self._h, None
        written = C.c_ulong(0)
        rc = self._L.AGMV_CloseWriter(h, C.byref(written))
        if rc:
            raise ValueError("AGMV_CloseWriter(%s) refused the clip (%d): fewer frames were written than the schedule's first group reads; no file is left" % (self.path, rc))
        return int(written.value)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *exc):
        if exc_type is None:
            self.close()
            return
        with contextlib.suppress(ValueError):          # (the block's own exception is the one to report)
            self.close()

    def __del__(self):
        with contextlib.suppress(Exception):
            self.close()


def decode_audio(path, fmt="s16", cap_samples=None):
    """-> (CUDA tensor of the file's audio track on the library's device in the layout `fmt`: int16 [n, ch] for "s16" and float32
    [ch, n] for "f32p" (a 16-bit track), uint8 [n, ch] for "u8" (an 8-bit track); AGMV_INFO of the header).  n is what the file's
    chunks hold, at most audio_size / ch -- and at most cap_samples / ch where cap_samples, a count over all channels, is given.
    A file without a track gives n = 0.  No video is decoded."""
    import torch
    v = pcmfmt(fmt)
    L = load_library()
    info = AGMV_INFO()
    rc = L.AGMV_DecodeAudioDev(os.fsencode(path), None, v, 0, C.byref(info))
    if rc < 0:
        raise RuntimeError("AGMV_DecodeAudioDev(%s): Error %d" % (path, -rc))
    dtype = {1: torch.int16, 2: torch.uint8, 3: torch.float32}[v]
    ch = max(int(info.number_of_channels), 1)
    cap = int(info.audio_size) if info.total_audio_duration else 0
    if cap_samples is not None:
        cap = min(cap, int(cap_samples))
    buf = torch.empty(max(cap, 1), dtype=dtype, device=_device())
    got = 0
    if cap:
        got = L.AGMV_DecodeAudioDev(os.fsencode(path), buf.data_ptr(), v, cap, None)
        if got < 0:
            raise RuntimeError("AGMV_DecodeAudioDev(%s, fmt %r): Error %d (a 16-bit track decodes as \"s16\" or \"f32p\", an 8-bit track as \"u8\")"
                               % (path, fmt, -got))
    return (buf[:got].view(ch, got // ch) if v == 3 else buf[:got].view(got // ch, ch)), info


class Quality:
    """What AGMV_MeasureFramesDev / AGMV_MeasureFileDev report for n frames of width x height (include/agmv.h, "measuring a decoded
    clip"): sse, block_sse, max_err and ssim_sum as numpy int64 [n, 3], channel 0 = R; ssim_sum holds the Q20 sums over each frame's windows.
    The three figures are formed here, in float64, over all frames and channels."""

    def __init__(self, entries, n, width, height):
        import numpy as np
        raw = np.frombuffer(entries, dtype=np.int64, count=12 * n).reshape(n, 4, 3).copy() if n else np.zeros((0, 4, 3), np.int64)
        self.sse, self.block_sse, self.max_err, self.ssim_sum = (raw[:, k, :] for k in range(4))
        self.width, self.height = int(width), int(height)

    def __len__(self):
        return self.sse.shape[0]

    @property
    def windows(self):
        """SSIM windows per frame and channel"""
        return (self.width // 4 - 1) * (self.height // 4 - 1)

    @staticmethod
    def _psnr(mse):
        import math
        return math.inf if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)

    def psnr(self):
        """10 log10(255^2 / mean squared error) over all frames and channels; inf for zero error, nan for no frame"""
        count = 3 * len(self) * self.width * self.height
        return self._psnr(float(int(self.sse.sum())) / count) if count else float("nan")

    def block_psnr(self):
        """the same for the means of the 4x4 blocks: block_sse is 256 times their squared error"""
        count = 3 * len(self) * (self.width // 4) * (self.height // 4)
        return self._psnr(float(int(self.block_sse.sum())) / 256.0 / count) if count else float("nan")

    def ssim(self):
        """the mean SSIM over windows, frames and channels; nan where a frame has no window"""
        count = 3 * len(self) * self.windows
        return float(int(self.ssim_sum.sum())) / float(1 << 20) / count if count else float("nan")


def clip_quality(test, ref, fmt=None, yuv=None, full_range=False):
    """test: the decoded clip, a contiguous CUDA int32 / uint32 tensor [n, h, w] of 0x00RRGGBB on the library's device; ref: the
    clip it is measured against, n frames of the same size in the layout `fmt` (as for encode_frames: None = inferred from the
    tensor, never a YUV layout) -> Quality (AGMV_MeasureFramesDev).  Its four integer arrays are sse, block_sse, max_err and
    ssim_sum (the `ssim` words of AGMV_FRAME_QUALITY: ssim() is the method that forms the mean from them)."""
    import torch
    v, n, h, w = _clip_geometry(ref, fmt, yuv, full_range, who="clip_quality")
    _, tn, th, tw = _clip_geometry(test, "xrgb32", who="clip_quality")
    if (tn, th, tw) != (n, h, w):
        raise ValueError("clip_quality: the test clip holds %d frames of %dx%d, the reference %d frames of %dx%d" % (tn, tw, th, n, w, h))
    for name, t in (("test clip", test), ("reference", ref)):
        if not (t.is_cuda and t.device == torch.device(_device())):
            raise ValueError("clip_quality: the %s must be on %s, got %s" % (name, _device(), t.device))
    torch.cuda.synchronize(test.device)            # the library works on streams of its own
    entries = (AGMV_FRAME_QUALITY * max(n, 1))()
    rc = load_library().AGMV_MeasureFramesDev(test.data_ptr(), ref.data_ptr(), v, n, w, h, entries)
    if rc:
        raise ValueError("AGMV_MeasureFramesDev refused its arguments (%d): %d frames of %dx%d" % (rc, n, w, h))
    return Quality(entries, n, w, h)


def file_quality(path, ref, fmt=None, yuv=None, full_range=False, deblock=None):
    """the file at `path`, decoded batch by batch and never held as a clip, against ref: its frames before they were encoded, in
    the layout `fmt` (as for clip_quality) -> Quality of the frames measured (AGMV_MeasureFileDev).  The reference must hold
    exactly the header's number of frames, at the file's size.  deblock=s measures the frames as decode_frames(deblock=s)
    delivers them."""
    with _deblock_for_this_call("file_quality", deblock):
        return _file_quality(path, ref, fmt, yuv, full_range)


def _file_quality(path, ref, fmt, yuv, full_range):
    import torch
    v, n, h, w = _clip_geometry(ref, fmt, yuv, full_range, who="file_quality")
    if not (ref.is_cuda and ref.device == torch.device(_device())):
        raise ValueError("file_quality: the reference must be on %s, got %s" % (_device(), ref.device))
    L = load_library()
    info = AGMV_INFO()
    rc = L.AGMV_MeasureFileDev(os.fsencode(path), None, v, 0, None, C.byref(info))
    if rc < 0:
        raise RuntimeError("AGMV_MeasureFileDev(%s): Error %d" % (path, -rc))
    if (info.number_of_frames, info.height, info.width) != (n, h, w):
        raise ValueError("file_quality: %s holds %d frames of %dx%d, the reference %d frames of %dx%d"
                         % (path, info.number_of_frames, info.width, info.height, n, w, h))
    torch.cuda.synchronize(ref.device)
    entries = (AGMV_FRAME_QUALITY * max(n, 1))()
    rc = L.AGMV_MeasureFileDev(os.fsencode(path), ref.data_ptr(), v, n, entries, None)
    if rc < 0:
        raise RuntimeError("AGMV_MeasureFileDev(%s): Error %d" % (path, -rc))
    return Quality(entries, rc, w, h)
