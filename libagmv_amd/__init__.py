"""libagmv_amd -- MI355X-native hot path of the AGMV codec (libagmv drop-in for that path).

Layout
  csrc/agmv_hip.hip   hand-written gfx950 kernels of the encoder (table, encode, pack) + the core of the
                      C-ABI of include/agmv_hip.h (context, palette, streams, memory)
  csrc/agmv_decode_hip.hip  the decoder: the parsers, k_decode, k_fixup and the calls of that C-ABI that launch them
  csrc/agmv_clip_hip.hip  the clip front end of that C-ABI: synth, interp, histogram, similarity, gather, the views of decoded and of source clips, the temporal stabilisation, the deblocking of a decoded clip, the byte and
                      YUV 4:2:0 layouts, the area scale, the decoder's scaling sink, normalised float tensors
  csrc/agmv_lz*_hip.hip   the LZSS / LZ77 stages of encoder and decoder on the GPU
  csrc/agmv_audio_hip.hip  audio tracks: the compand / expand kernels (csrc/agmv_audio.h states the codec once, for host and device)
  csrc/*.c            host C: libagmv-compatible API (include/agmv.h), LZSS/LZ77, container,
                      BMP I/O, palette build, synthetic clip generator
  abi.py              the public C signatures, stated once: both libraries' ctypes tables and the structures (tests/test_abi.py holds them to the headers)
  hip.py              ctypes binding of the C-ABI for tests / bench (torch = device memory only)
  seq.py              ctypes calls of the memory-sequence entry points of include/agmv.h (.agmv file <-> CUDA tensor: five RGB layouts, NV12, I420; normalised float tensors; a scale to a target size before the encode and behind the decode; views of a file and of a clip; reader sessions, a file read in pieces with the decoder's state kept; writer sessions, a clip encoded in pieces into the one-shot call's file; a decoded clip or file measured against its reference)
  build.py            in-tree build of libagmv_hip.so / libagmv.so (hipcc, gcc)

There is no CPU fallback anywhere in this package: without the built HIP library, or
without a GPU, the hot-path calls raise.
"""
from .hip import PCMFMT, PIXFMT, TENSORFMT, YUVFMT, AgmvHip, HipUnavailable, lib_path, load_library  # noqa: F401
from .seq import DECODE_SCALE, SCALE, SCHEDULE_ADAPTIVE, SCHEDULE_FULL, SCHEDULE_PDIFS, Quality, Reader, Writer, clip_quality, deblock_stats, decode_audio, decode_frames, encode_frames, encode_rate_stats, encode_view_stats, file_quality, fit_window, stabilise_stats  # noqa: F401

__all__ = ["AgmvHip", "HipUnavailable", "lib_path", "load_library", "encode_frames", "decode_frames", "Reader", "Writer", "decode_audio",
           "clip_quality", "file_quality", "Quality", "stabilise_stats", "deblock_stats", "encode_view_stats", "encode_rate_stats", "fit_window",
           "SCHEDULE_FULL", "SCHEDULE_PDIFS", "SCHEDULE_ADAPTIVE", "PIXFMT", "YUVFMT", "PCMFMT", "TENSORFMT", "SCALE", "DECODE_SCALE"]
