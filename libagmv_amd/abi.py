"""The public C signatures, stated once: the structures of include/agmv.h that Python passes, every function of
include/agmv_hip.h (HIP), of include/agmv_hip_view.h (HIP_VIEW), of include/agmv_hip_view_source.h (HIP_VIEW_SOURCE), of
include/agmv_hip_stabilise.h (HIP_STABILISE), of include/agmv_hip_deblock.h (HIP_DEBLOCK) and of include/agmv_hip_time.h (HIP_TIME), every function of include/agmv.h that Python calls on libagmv.so (AGMV)
and every function of include/agmv_reader.h and include/agmv_writer.h, which the same library exports (READER, WRITER), as
name -> (restype, (argtypes...)).  bind() sets them on a loaded library.  tests/test_abi.py checks both tables and the
structures against the headers.  ctypes only, and no library is loaded here: the test children import this module the
way a C host would include the headers."""
from ctypes import (POINTER, Structure, c_char_p, c_float, c_int, c_longlong, c_size_t, c_ubyte, c_uint, c_uint32, c_uint64, c_ulong,
                    c_ulonglong, c_ushort, c_void_p)


class AGMV_ENTRY(Structure):
    _fields_ = [("pal_num", c_ubyte), ("index", c_ubyte), ("occurence", c_ulong)]


class AGMV_INFO(Structure):
    # (u32 is `unsigned long` in include/agmv.h)
    _fields_ = [("width", c_ulong), ("height", c_ulong), ("number_of_frames", c_ulong), ("version", c_ubyte),
                ("total_audio_duration", c_ulong), ("sample_rate", c_ulong), ("audio_size", c_ulong),
                ("number_of_channels", c_ushort), ("bits_per_sample", c_ushort)]


class AGMV_FRAME_QUALITY(Structure):
    # 96 bytes, the same on host and device
    _fields_ = [("sse", c_ulonglong * 3), ("block_sse", c_ulonglong * 3), ("max_err", c_ulonglong * 3), ("ssim", c_longlong * 3)]


class AGMV_VIEW(Structure):
    # plain 32-bit unsigned, not the header's u32
    _fields_ = [("first", c_uint), ("count", c_uint), ("step", c_uint), ("x", c_uint), ("y", c_uint), ("width", c_uint), ("height", c_uint)]


class AGMV_VIEW_STATS(Structure):
    _fields_ = [("lz_frames", c_uint), ("gpu_frames", c_uint), ("delivered", c_uint), ("restarts", c_uint)]


class AGMV_ENCODE_VIEW_STATS(Structure):
    _fields_ = [("frames", c_uint), ("clip_bytes", c_ulonglong), ("staging_bytes", c_ulonglong)]


class AGMV_RATE(Structure):
    _fields_ = [("src", c_uint), ("dst", c_uint), ("filter", c_uint)]


class AGMV_ENCODE_RATE_STATS(Structure):
    _fields_ = [("frames_in", c_uint), ("frames_out", c_uint), ("frame_reads", c_ulonglong)]


class AGMV_STABILISE_STATS(Structure):
    _fields_ = [("examined", c_ulonglong), ("replaced", c_ulonglong)]


class AGMV_DEBLOCK_STATS(Structure):
    _fields_ = [("strength", c_uint), ("frames", c_uint), ("lines", c_ulonglong), ("weak", c_ulonglong), ("strong", c_ulonglong)]


class AGMV_READER_DESC(Structure):
    # include/agmv_reader.h; the enums are c_int
    _fields_ = [("tensor", c_int), ("fmt", c_int), ("yuv_flags", c_int), ("type", c_int), ("mean", c_float * 3), ("std", c_float * 3),
                ("width", c_uint), ("height", c_uint), ("filter", c_int), ("step", c_uint), ("x", c_uint), ("y", c_uint),
                ("win_width", c_uint), ("win_height", c_uint), ("deblock", c_uint), ("index_bytes", c_size_t)]


class AGMV_READER_STATS(Structure):
    _fields_ = [("lz_frames", c_ulonglong), ("gpu_frames", c_ulonglong), ("delivered", c_ulonglong), ("reads", c_uint), ("seeks", c_uint),
                ("restarts", c_uint), ("checkpoints", c_uint), ("interval", c_uint)]


class AGMV_WRITER_DESC(Structure):
    # include/agmv_writer.h; the enums are c_int
    _fields_ = [("tensor", c_int), ("fmt", c_int), ("yuv_flags", c_int), ("type", c_int), ("mean", c_float * 3), ("std", c_float * 3),
                ("src_width", c_uint), ("src_height", c_uint), ("width", c_uint), ("height", c_uint), ("filter", c_int),
                ("frames_per_second", c_uint), ("opt", c_int), ("quality", c_int), ("compression", c_int), ("schedule", c_int),
                ("ring_frames", c_uint)]


class AGMV_WRITER_STATS(Structure):
    _fields_ = [("analysed", c_ulonglong), ("taken", c_ulonglong), ("written", c_ulonglong), ("writes", c_uint), ("batches", c_uint),
                ("waits", c_uint), ("ring_frames", c_uint)]


# vp: any pointer but the five below and `const char*`; ul: the header's u32; the enums and Bool are c_int
vp, sz, u32, u64, ul = c_void_p, c_size_t, c_uint32, c_uint64, c_ulong
INFO_P, QUALITY_P, ENTRY_P = POINTER(AGMV_INFO), POINTER(AGMV_FRAME_QUALITY), POINTER(AGMV_ENTRY)
VIEW_P, VIEW_STATS_P, STABILISE_STATS_P = POINTER(AGMV_VIEW), POINTER(AGMV_VIEW_STATS), POINTER(AGMV_STABILISE_STATS)
DEBLOCK_STATS_P = POINTER(AGMV_DEBLOCK_STATS)
ENCODE_VIEW_STATS_P = POINTER(AGMV_ENCODE_VIEW_STATS)
RATE_P, ENCODE_RATE_STATS_P = POINTER(AGMV_RATE), POINTER(AGMV_ENCODE_RATE_STATS)

HIP = {
    "agmv_hip_max_usize": (sz, (u32, u32, c_int)),
    "agmv_hip_device_count": (c_int, ()),
    "agmv_hip_create": (vp, (c_int,)),
    "agmv_hip_destroy": (None, (vp,)),
    "agmv_hip_last_error": (c_char_p, ()),
    "agmv_hip_set_palette": (c_int, (vp, vp, vp, c_int, vp)),
    "agmv_hip_quantise_dev": (c_int, (vp, vp, sz, vp, vp)),
    "agmv_hip_dither_frames_async": (c_int, (vp, u32, vp, u32, u32, u32, vp)),
    "agmv_hip_encode_frames_dev": (c_int, (vp, vp, u32, u32, u32, u32, vp, sz, vp, vp, vp)),
    "agmv_hip_encode_frames": (c_int, (vp, vp, u32, u32, u32, u32, vp, sz, vp, vp)),
    "agmv_hip_encode_entries_dev": (c_int, (vp, vp, u32, u32, u32, u32, vp, sz, vp, vp, vp)),
    "agmv_hip_encode_entries": (c_int, (vp, vp, u32, u32, u32, u32, vp, sz, vp, vp)),
    "agmv_hip_nearest": (c_int, (vp, vp, vp, c_int, vp, sz, vp)),
    "agmv_hip_within2_count": (c_int, (vp, vp, vp)),
    "agmv_hip_parse_frames_dev": (c_int, (vp, vp, sz, vp, u32, u32, u32, vp, vp, vp)),
    "agmv_hip_decode_frames_dev": (c_int, (vp, vp, sz, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp)),
    "agmv_hip_parse_fallback_frames": (c_int, (vp, vp)),
    "agmv_hip_parse_decode_frames_dev": (c_int, (vp, vp, sz, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp)),
    "agmv_hip_decode_bitstreams_dev": (c_int, (vp, vp, sz, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp)),
    "agmv_hip_decode_prior_dependent": (c_int, (vp, u32, u32, vp)),
    "agmv_hip_decode_frames": (c_int, (vp, vp, sz, vp, u32, u32, u32, u32, vp, vp, vp)),
    "agmv_hip_pack_frames_dev": (c_int, (vp, vp, sz, vp, u32, vp, vp, vp)),
    "agmv_hip_unpack_frames_dev": (c_int, (vp, vp, vp, u32, vp, sz, vp, vp)),
    "agmv_hip_lzss_max_csize": (sz, (sz,)),
    "agmv_hip_lzss_frames_dev": (c_int, (vp, vp, sz, vp, u32, vp, sz, vp, vp)),
    "agmv_hip_lzss_frames": (c_int, (vp, vp, sz, vp, u32, vp, sz, vp)),
    "agmv_hip_lz77_max_csize": (sz, (sz,)),
    "agmv_hip_lz77_peek_dev": (c_int, (vp, vp, sz, vp, u32, vp, sz, vp, vp)),
    "agmv_hip_lz77_frames_dev": (c_int, (vp, vp, sz, vp, u32, vp, vp, sz, vp, vp)),
    "agmv_hip_lz77_frames": (c_int, (vp, vp, sz, vp, u32, vp, sz, vp, sz, vp)),
    "agmv_hip_lz77_reparsed_segments": (c_int, (vp, vp)),
    "agmv_hip_lz_decode_frames_dev": (c_int, (vp, c_int, vp, vp, vp, vp, vp, u32, vp, sz, sz, vp, vp, vp)),
    "agmv_hip_lz_decode_frames_sized_dev": (c_int, (vp, c_int, vp, vp, vp, vp, vp, u32, vp, sz, sz, vp, vp, vp)),
    "agmv_hip_lz_decode_commit_dev": (c_int, (vp, vp, sz, vp, u32, vp, sz, vp)),
    "agmv_hip_lz_decode_fallback_frames": (c_int, (vp, vp)),
    "agmv_hip_lz_decode_frames": (c_int, (vp, c_int, vp, sz, vp, vp, vp, vp, u32, vp, sz, sz, vp, vp, vp)),
    "agmv_hip_synth_dev": (c_int, (vp, vp, u32, u32, u32, u32, u64, vp)),
    "agmv_hip_interp_dev": (c_int, (vp, vp, vp, vp, sz, vp)),
    "agmv_hip_histogram_dev": (c_int, (vp, vp, sz, c_int, vp, vp)),
    "agmv_hip_similarity_dev": (c_int, (vp, vp, u32, sz, vp, vp)),
    "agmv_hip_gather_dev": (c_int, (vp, vp, sz, u32, vp, sz, vp, vp)),
    "agmv_hip_pixfmt_frame_bytes": (sz, (c_int, sz)),
    "agmv_hip_pixels_to_xrgb_dev": (c_int, (vp, c_int, vp, sz, u32, sz, vp, vp)),
    "agmv_hip_pixels_from_xrgb_dev": (c_int, (vp, c_int, vp, u32, sz, vp, vp)),
    "agmv_hip_gather_fmt_dev": (c_int, (vp, c_int, vp, sz, u32, vp, sz, vp, vp)),
    "agmv_hip_histogram_fmt_dev": (c_int, (vp, c_int, vp, sz, u32, sz, c_int, vp, vp)),
    "agmv_hip_similarity_fmt_dev": (c_int, (vp, c_int, vp, u32, sz, vp, vp)),
    "agmv_hip_yuv_frame_bytes": (sz, (c_int, u32, u32)),
    "agmv_hip_yuv_to_xrgb_dev": (c_int, (vp, c_int, vp, u32, u32, u32, sz, vp, vp)),
    "agmv_hip_yuv_from_xrgb_dev": (c_int, (vp, c_int, vp, u32, u32, u32, vp, vp)),
    "agmv_hip_yuv_gather_dev": (c_int, (vp, c_int, vp, u32, u32, u32, vp, sz, vp, vp)),
    "agmv_hip_yuv_histogram_dev": (c_int, (vp, c_int, vp, u32, u32, u32, sz, c_int, vp, vp)),
    "agmv_hip_yuv_similarity_dev": (c_int, (vp, c_int, vp, u32, u32, u32, vp, vp)),
    "agmv_hip_scale_area_dev": (c_int, (vp, c_int, vp, u32, u32, u32, u32, u32, vp, vp)),
    "agmv_hip_scale_frames_async": (c_int, (vp, c_int, vp, u32, u32, u32, c_int, u32, u32, vp, vp)),
    "agmv_hip_tensor_frame_bytes": (sz, (c_int, sz)),
    "agmv_hip_tensor_table": (c_int, (c_int, vp, vp, vp)),
    "agmv_hip_tensor_from_xrgb_async": (c_int, (vp, c_int, vp, u32, u32, u32, c_int, u32, u32, vp, vp, vp)),
    "agmv_hip_tensor_to_xrgb_async": (c_int, (vp, c_int, vp, sz, u32, vp, vp, vp)),
    "agmv_hip_palette_refine_dev": (c_int, (vp, vp, c_int, vp, u32, u32, u32, vp, vp, vp)),
    "agmv_hip_audio_compand_async": (c_int, (vp, c_int, vp, u32, u64, vp, vp)),
    "agmv_hip_audio_expand_async": (c_int, (vp, c_int, vp, u32, u64, vp, vp)),
    "agmv_hip_measure_frames_async": (c_int, (vp, vp, c_int, vp, u32, u32, u32, vp, vp)),
    "agmv_hip_enable_timing": (c_int, (vp, c_int)),
    "agmv_hip_last_kernel_ms": (c_float, (vp, c_int)),
    "agmv_hip_check": (c_int, (vp, vp)),
    "agmv_hip_stream_create": (vp, (vp,)),
    "agmv_hip_stream_destroy": (None, (vp, vp)),
    "agmv_hip_stream_sync": (c_int, (vp, vp)),
    "agmv_hip_event_create": (vp, (vp,)),
    "agmv_hip_event_destroy": (None, (vp, vp)),
    "agmv_hip_event_record": (c_int, (vp, vp, vp)),
    "agmv_hip_stream_wait_event": (c_int, (vp, vp, vp)),
    "agmv_hip_host_alloc": (vp, (sz,)),
    "agmv_hip_host_free": (None, (vp,)),
    "agmv_hip_malloc_on": (vp, (vp, sz)),
    "agmv_hip_free_on": (None, (vp, vp)),
    "agmv_hip_memcpy_async": (c_int, (vp, vp, vp, sz, c_int, vp)),
    "agmv_hip_memset_async": (c_int, (vp, vp, c_int, sz, vp)),
    "agmv_hip_ctx_device": (c_int, (vp,)),
    "agmv_hip_malloc": (vp, (sz,)),
    "agmv_hip_free": (None, (vp,)),
    "agmv_hip_memcpy_h2d": (c_int, (vp, vp, sz)),
    "agmv_hip_memcpy_d2h": (c_int, (vp, vp, sz)),
    "agmv_hip_memset": (c_int, (vp, c_int, sz)),
    "agmv_hip_sync": (c_int, ()),
}

# include/agmv_hip_view.h, exported by the same library
HIP_VIEW = {
    "agmv_hip_view_frames_async": (c_int, (vp, vp, u32, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp)),
}

# include/agmv_hip_view_source.h, exported by the same library
HIP_VIEW_SOURCE = {
    "agmv_hip_view_source_async": (c_int, (vp, c_int, vp, u32, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp)),
}

# include/agmv_hip_stabilise.h, exported by the same library
HIP_STABILISE = {
    "agmv_hip_stabilise_frames_async": (c_int, (vp, u32, vp, u32, u32, u32, u32, vp, vp)),
}

# include/agmv_hip_deblock.h, exported by the same library
HIP_DEBLOCK = {
    "agmv_hip_deblock_frames_async": (c_int, (vp, u32, vp, u32, u32, u32, vp, vp, vp)),
}

# include/agmv_hip_time.h, exported by the same library
HIP_TIME = {
    "agmv_hip_time_frames_async": (c_int, (vp, c_int, vp, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, c_int, u32, u32, vp, vp)),
}

_SEQ = (c_char_p, c_char_p, c_char_p, c_ubyte, ul, ul, ul, ul, ul, c_int, c_int, c_int)     # the three BMP drivers, behind `agmv`
_CLIP = (ul, ul, ul, ul, c_int, c_int, c_int, c_int)                 # frames, width, height, fps, opt, quality, compression, schedule

AGMV = {
    "CreateAGMV": (vp, (ul, ul, ul, ul)),
    "DestroyAGMV": (None, (vp,)),
    "AGMV_SetICP0": (None, (vp, vp)),
    "AGMV_SetICP1": (None, (vp, vp)),
    "AGMV_SetTotalAudioDuration": (None, (vp, ul)),
    "AGMV_SetSampleRate": (None, (vp, ul)),
    "AGMV_SetNumberOfChannels": (None, (vp, c_ubyte)),
    "AGMV_SetAudioSize": (None, (vp, ul)),
    "AGMV_SetOPT": (None, (vp, c_int)),
    "AGMV_SetCompression": (None, (vp, c_int)),
    "AGMV_SetBitsPerSample": (None, (vp, c_ushort)),
    "AGMV_GetNumberOfFrames": (ul, (vp,)),
    "AGMV_GetTotalAudioDuration": (ul, (vp,)),
    "AGMV_GetSampleRate": (ul, (vp,)),
    "AGMV_GetNumberOfChannels": (c_ushort, (vp,)),
    "AGMV_GetAudioSize": (ul, (vp,)),
    "AGMV_GetBitsPerSample": (c_ushort, (vp,)),
    "AGMV_FindNextFrameChunk": (None, (vp,)),
    "AGMV_FindNextAudioChunk": (None, (vp,)),
    "AGMV_SkipFrameChunk": (None, (vp,)),
    "AGMV_ParseAGMV": (None, (vp, vp)),
    "AGMV_GetVersionFromOPT": (c_ubyte, (c_int, c_int)),
    "AGMV_SyncAudioTrack": (None, (vp, vp)),
    "AGMV_SignedToUnsignedPCM": (None, (vp, ul)),
    "AGMV_UnsigendToSignedPCM": (None, (vp, ul)),
    "AGMV_CalculateTotalAudioDuration": (ul, (ul, ul, c_ushort, c_ushort)),
    "AGMV_QuantizeColor": (ul, (ul, c_int)),
    "AGMV_ReverseQuantizeColor": (ul, (ul, c_int)),
    "AGMV_CompareFrameSimilarity": (c_float, (vp, vp, ul, ul)),
    "AGMV_BubbleSort": (None, (vp, vp, ul)),
    "AGMV_FindNearestColor": (c_ubyte, (vp, ul)),
    "AGMV_FindNearestEntry": (AGMV_ENTRY, (vp, vp, ul)),
    "AGMV_FindSmallestColor": (c_ubyte, (vp, ul)),
    "AGMV_FindSmallestEntry": (AGMV_ENTRY, (vp, vp, ul)),
    "AGMV_ComparePFrameBlock": (c_ubyte, (vp, ul, ul, ENTRY_P)),
    "AGMV_CompareIFrameBlock": (c_ubyte, (vp, ul, ul, ul, ENTRY_P)),
    "AGMV_AssembleIFrameBitstream": (None, (vp, ENTRY_P)),
    "AGMV_AssemblePFrameBitstream": (None, (vp, ENTRY_P)),
    "AGMV_EncodeHeader": (None, (vp, vp)),
    "AGMV_EncodeFrame": (None, (vp, vp, vp)),
    "AGMV_CompressAudio": (None, (vp,)),
    "AGMV_EncodeAudioChunk": (None, (vp, vp)),
    "AGMV_DecodeHeader": (c_int, (vp, vp)),
    "AGMV_DecodeFrameChunk": (c_int, (vp, vp)),
    "AGMV_DecodeAudioChunk": (c_int, (vp, vp)),
    "AGMV_EncodeVideo": (None, _SEQ),
    "AGMV_EncodeAGMV": (None, (vp,) + _SEQ),
    "AGMV_EncodeFullAGMV": (None, (vp,) + _SEQ),
    "AGMV_DecodeVideo": (c_int, (c_char_p, c_ubyte)),
    "AGMV_DecodeAGMV": (c_int, (c_char_p, c_ubyte, c_int)),
    "AGMV_WavToAudioTrack": (None, (c_char_p, vp)),
    "AGMV_RawSignedPCMToAudioTrack": (None, (c_char_p, vp, c_ubyte, ul)),
    "AGMV_Raw8PCMToAudioTrack": (None, (c_char_p, vp)),
    "AGMV_ExportAudioType": (None, (vp, vp, c_int)),
    "AGMV_DecodeAudio": (c_int, (c_char_p, c_int)),
    "AGMV_ResetVideo": (None, (vp, vp)),
    "AGMV_IsVideoDone": (c_int, (vp,)),
    "AGMV_SkipForwards": (None, (vp, vp, c_int)),
    "AGMV_SkipForwardsAndDecodeAudio": (None, (vp, vp, c_int)),
    "AGMV_SkipBackwards": (None, (vp, vp, c_int)),
    "AGMV_SkipTo": (None, (vp, vp, c_int)),
    "AGMV_PlayAGMV": (None, (vp, vp)),
    "PlotPixel": (None, (vp, c_int, c_int, c_int, c_int, ul)),
    "AGMV_DisplayFrame": (None, (vp, c_ushort, c_ushort, vp)),
    "AGMV_ExportAGMVToHeader": (None, (c_char_p,)),
    "AGMV_SetBatchFrames": (None, (c_uint,)),
    "AGMV_SetLZThreads": (None, (c_uint,)),
    "AGMV_SetDevices": (None, (c_uint,)),
    "AGMV_SynthFrame": (None, (vp, c_uint, c_uint, c_uint, u64)),
    "AGMV_BuildPalette": (None, (vp, c_int, c_int, vp, vp)),
    "AGMV_BuildPaletteRefined": (c_int, (vp, c_int, c_int, vp, vp, c_uint, vp)),
    "AGMV_SetPaletteRefine": (None, (c_uint,)),
    "AGMV_SetDither": (None, (c_uint,)),
    "AGMV_SetStabilise": (None, (c_uint,)),
    "AGMV_GetStabiliseStats": (None, (STABILISE_STATS_P,)),
    "AGMV_SetDeblock": (None, (c_uint,)),
    "AGMV_GetDeblockStats": (None, (DEBLOCK_STATS_P,)),
    "AGMV_EncodeFramesDev": (c_int, (c_char_p, vp) + _CLIP),
    "AGMV_DecodeFramesDev": (c_int, (c_char_p, vp, ul, INFO_P)),
    "AGMV_EncodeFramesFmtDev": (c_int, (c_char_p, vp, c_int) + _CLIP),
    "AGMV_DecodeFramesFmtDev": (c_int, (c_char_p, vp, c_int, ul, INFO_P)),
    "AGMV_EncodeFramesScaledDev": (c_int, (c_char_p, vp, c_int, ul, ul, ul, ul, ul, c_int, ul, c_int, c_int, c_int, c_int)),
    "AGMV_DecodeFramesScaledDev": (c_int, (c_char_p, vp, c_int, ul, ul, c_int, ul, INFO_P)),
    "AGMV_EncodeFramesTensorDev": (c_int, (c_char_p, vp, c_int, vp, vp) + _CLIP),
    "AGMV_DecodeFramesTensorDev": (c_int, (c_char_p, vp, c_int, vp, vp, ul, ul, c_int, ul, INFO_P)),
    "AGMV_DecodeViewDev": (c_int, (c_char_p, vp, c_int, ul, ul, c_int, VIEW_P, ul, INFO_P)),
    "AGMV_DecodeViewTensorDev": (c_int, (c_char_p, vp, c_int, vp, vp, ul, ul, c_int, VIEW_P, ul, INFO_P)),
    "AGMV_GetViewStats": (None, (VIEW_STATS_P,)),
    "AGMV_EncodeViewDev": (c_int, (c_char_p, vp, c_int, ul, ul, ul, VIEW_P, ul, ul, c_int, ul, c_int, c_int, c_int, c_int)),
    "AGMV_GetEncodeViewStats": (None, (ENCODE_VIEW_STATS_P,)),
    "AGMV_EncodeViewRateDev": (c_int, (c_char_p, vp, c_int, ul, ul, ul, VIEW_P, RATE_P, ul, ul, c_int, ul, c_int, c_int, c_int, c_int)),
    "AGMV_GetEncodeRateStats": (None, (ENCODE_RATE_STATS_P,)),
    "AGMV_SetAudioDev": (c_int, (vp, c_int, ul, ul, c_ushort)),
    "AGMV_DecodeAudioDev": (c_int, (c_char_p, vp, c_int, ul, INFO_P)),
    "AGMV_MeasureFramesDev": (c_int, (vp, vp, c_int, ul, ul, ul, QUALITY_P)),
    "AGMV_MeasureFileDev": (c_int, (c_char_p, vp, c_int, ul, QUALITY_P, INFO_P)),
}

# include/agmv_reader.h, exported by libagmv.so
READER = {
    "AGMV_OpenReaderDev": (vp, (c_char_p, POINTER(AGMV_READER_DESC), INFO_P, POINTER(c_int))),
    "AGMV_ReaderReadDev": (c_int, (vp, vp, ul)),
    "AGMV_ReaderSeek": (c_int, (vp, ul)),
    "AGMV_ReaderTell": (ul, (vp,)),
    "AGMV_GetReaderStats": (None, (vp, POINTER(AGMV_READER_STATS))),
    "AGMV_CloseReader": (None, (vp,)),
}

# include/agmv_writer.h, exported by libagmv.so
WRITER = {
    "AGMV_OpenWriterDev": (vp, (c_char_p, POINTER(AGMV_WRITER_DESC), POINTER(c_int))),
    "AGMV_WriterAnalyseDev": (c_int, (vp, vp, ul)),
    "AGMV_WriterWriteDev": (c_int, (vp, vp, ul)),
    "AGMV_CloseWriter": (c_int, (vp, POINTER(c_ulong))),
    "AGMV_GetWriterStats": (None, (vp, POINTER(AGMV_WRITER_STATS))),
}


def bind(lib, table, missing_ok=False):
    """set restype and argtypes of every function of `table` on the loaded library `lib`, and return it.  A symbol the
    library lacks raises AttributeError with its name, unless missing_ok (another build of the same source)."""
    for name, (restype, argtypes) in table.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            if missing_ok:
                continue
            raise AttributeError("%s does not export %s" % (getattr(lib, "_name", lib), name))
        f.restype, f.argtypes = restype, list(argtypes)
    return lib
