/*
 * include/agmv.h -- libagmv-compatible C API of the MI355X build (drop-in for the hot path).
 *
 * Same symbols, argument meaning, struct layouts and error behaviour as the reference's
 * public headers (reference include/agmv_defines.h, agmv_encode.h, agmv_decode.h,
 * agmv_utils.h, agmv_playback.h), so existing callers (README snippets, the example programs,
 * tools/agmvcli) compile and link unchanged against libagmv_amd/libagmv.so.
 * The per-frame work behind AGMV_EncodeFrame / AGMV_DecodeFrameChunk and the batch drivers
 * runs on the GPU through include/agmv_hip.h; LZSS/LZ77, the container, BMP I/O and the
 * palette build are host C (the opt-in refinement of the palette, AGMV_BuildPaletteRefined,
 * runs on the GPU).  There is no CPU fallback for the hot path: without a GPU the
 * encode/decode entry points abort with a message (the void encoders have no error channel,
 * reference src/agmv_encode.c:529).
 *
 * Out of scope in this build (declared by the reference, not provided here): the ten
 * non-BMP image formats, the AIFF / AIFC audio importers (AGMV_AIFFToAudioTrack, AGMV_AIFCToAudioTrack,
 * AGMV_80BitFloat), the Win32 player helpers.
 */
#ifndef AGMV_H
#define AGMV_H

#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scalar types (reference include/agmv_defines.h:20-30). NOTE u32 is `unsigned long`:
 * 8 bytes on LP64 -- frame buffers are 8 B/pixel at this boundary and are packed to 4 B/pixel
 * before they go to the GPU. */
typedef unsigned char  u8;
typedef unsigned short u16;
typedef unsigned long  u32;
typedef signed char    s8;
typedef signed short   s16;
typedef signed long    s32;
typedef float          f32;
typedef int            Bool;

#ifndef TRUE
#define TRUE  1
#define FALSE 0
#endif

typedef enum Error {                       /* reference include/agmv_defines.h:37-42 */
	NO_ERR = 0x0,
	INVALID_HEADER_FORMATTING_ERR = 0x1,
	FILE_NOT_FOUND_ERR = 0x2,
	MEMORY_CORRUPTION_ERR = 0x3,
} Error;

#define AGMV_MAX_CLR      524287
#define MAX_OFFSET_TABLE  40000

#define AGMV_FILL_FLAG    0x4E             /* block opcodes, reference include/agmv_defines.h:49-53 */
#define AGMV_NORMAL_FLAG  0x2f
#define AGMV_COPY_FLAG    0x5E
#define AGMV_FILL_COUNT   14
#define AGMV_COPY_COUNT   13

#define AGMV_GBA_W 120                     /* reference include/agmv_encode.h:21-24 */
#define AGMV_GBA_H  80
#define AGMV_NDS_W 128
#define AGMV_NDS_H  96

typedef enum AGMV_OPT {                    /* reference include/agmv_defines.h:56-65 */
	AGMV_OPT_I = 0x1,                      /* 512 colours, heavy PDIFS */
	AGMV_OPT_II = 0x2,                     /* 256 colours, light PDIFS */
	AGMV_OPT_III = 0x3,                    /* 512 colours, light PDIFS */
	AGMV_OPT_ANIM = 0x4,                   /* 256 colours, heavy PDIFS */
	AGMV_OPT_GBA_I = 0x5,                  /* 512 colours, heavy PDIFS, 120x80 */
	AGMV_OPT_GBA_II = 0x6,                 /* 256 colours, heavy PDIFS, 120x80 */
	AGMV_OPT_GBA_III = 0x7,                /* 512 colours, light PDIFS, 120x80 */
	AGMV_OPT_NDS = 0x8,                    /* 512 colours, light (BMP) PDIFS, 128x96 */
} AGMV_OPT;

typedef enum AGMV_QUALITY { AGMV_HIGH_QUALITY = 0x1, AGMV_MID_QUALITY = 0x2, AGMV_LOW_QUALITY = 0x3 } AGMV_QUALITY;
typedef enum AGMV_COMPRESSION { AGMV_LZSS_COMPRESSION = 0x1, AGMV_LZ77_COMPRESSION = 0x2 } AGMV_COMPRESSION;

typedef enum AGMV_IMG_TYPE {
	AGMV_IMG_BMP = 0x1, AGMV_IMG_TGA = 0x2, AGMV_IMG_TIM = 0x3, AGMV_IMG_PCX = 0x4, AGMV_IMG_LMP = 0x5,
	AGMV_IMG_PVR = 0x6, AGMV_IMG_GXT = 0x7, AGMV_IMG_BTI = 0x8, AGMV_IMG_3DF = 0x9, AGMV_IMG_PPM = 0x0A,
	AGMV_IMG_LBM = 0x0B,
} AGMV_IMG_TYPE;

typedef enum AGMV_AUDIO_TYPE { AGMV_AUDIO_WAV = 0x1, AGMV_AUDIO_AIFF = 0x2, AGMV_AUDIO_AIFC = 0x3, AGMV_AUDIO_RAW = 0x4 } AGMV_AUDIO_TYPE;

/* ---- records; member order and types fixed by the reference (include/agmv_defines.h:78-162) */
typedef struct AGMV_MAIN_HEADER {
	char fourcc[4];
	u32 num_of_frames;
	u32 width;
	u32 height;
	u8  fmt;
	u8  version;
	u32 frames_per_second;
	u32 total_audio_duration;
	u32 sample_rate;
	u32 audio_size;
	u16 num_of_channels;
	u16 bits_per_sample;
	u32 palette0[256];
	u32 palette1[256];
} AGMV_MAIN_HEADER;

typedef struct AGMV_FRAME_CHUNK { char fourcc[4]; u32 frame_num; u32 uncompressed_size; u32 compressed_size; } AGMV_FRAME_CHUNK;
typedef struct AGMV_AUDIO_CHUNK { char fourcc[4]; u32 size; u8* atsample; s8* satsample; } AGMV_AUDIO_CHUNK;
typedef struct AGMV_FRAME { u32 width; u32 height; u32* img_data; } AGMV_FRAME;
typedef struct AGMV_AUDIO_TRACK { u32 total_audio_duration; u32 start_point; u16* pcm; u8* pcm8; } AGMV_AUDIO_TRACK;
typedef struct AGMV_ENTRY { u8 pal_num; u8 index; u32 occurence; } AGMV_ENTRY;
typedef struct AGMV_INFO {
	u32 width; u32 height; u32 number_of_frames; u8 version; u32 total_audio_duration; u32 sample_rate;
	u32 audio_size; u16 number_of_channels; u16 bits_per_sample;
} AGMV_INFO;
typedef struct AGMV_BITSTREAM { u8* data; u32 len; u32 pos; } AGMV_BITSTREAM;

typedef struct AGMV {
	AGMV_MAIN_HEADER header;
	AGMV_FRAME_CHUNK* frame_chunk;
	AGMV_AUDIO_CHUNK* audio_chunk;
	AGMV_BITSTREAM* bitstream;
	AGMV_FRAME* frame;
	AGMV_FRAME* iframe;
	AGMV_AUDIO_TRACK* audio_track;
	AGMV_ENTRY* iframe_entries;
	AGMV_OPT opt;
	AGMV_COMPRESSION compression;
	u32 frame_count;
	f32 leniency;
	u32 offset_table[MAX_OFFSET_TABLE];
	Bool enable_audio;
	f32 volume;
} AGMV;

/* ---- object lifecycle + attributes (reference include/agmv_utils.h:53-92) */
AGMV* CreateAGMV(u32 num_of_frames, u32 width, u32 height, u32 frames_per_second);
void  DestroyAGMV(AGMV* agmv);

void AGMV_SetWidth(AGMV* agmv, u32 width);
void AGMV_SetHeight(AGMV* agmv, u32 height);
void AGMV_SetICP0(AGMV* agmv, u32 palette0[256]);
void AGMV_SetICP1(AGMV* agmv, u32 palette1[256]);
void AGMV_SetFramesPerSecond(AGMV* agmv, u32 frames_per_second);
void AGMV_SetNumberOfFrames(AGMV* agmv, u32 num_of_frames);
void AGMV_SetTotalAudioDuration(AGMV* agmv, u32 total_audio_duration);
void AGMV_SetSampleRate(AGMV* agmv, u32 sample_rate);
void AGMV_SetNumberOfChannels(AGMV* agmv, u8 num_of_channels);
void AGMV_SetAudioSize(AGMV* agmv, u32 size);
void AGMV_SetLeniency(AGMV* agmv, f32 leniency);
void AGMV_SetOPT(AGMV* agmv, AGMV_OPT opt);
void AGMV_SetVersion(AGMV* agmv, u8 version);
void AGMV_SetCompression(AGMV* agmv, AGMV_COMPRESSION compression);
void AGMV_SetAudioState(AGMV* agmv, Bool audio);
void AGMV_SetVolume(AGMV* agmv, f32 volume);
void AGMV_SetBitsPerSample(AGMV* agmv, u16 bits_per_sample);

u32 AGMV_GetWidth(AGMV* agmv);
u32 AGMV_GetHeight(AGMV* agmv);
u32 AGMV_GetFramesPerSecond(AGMV* agmv);
u32 AGMV_GetNumberOfFrames(AGMV* agmv);
u32 AGMV_GetTotalAudioDuration(AGMV* agmv);
u32 AGMV_GetSampleRate(AGMV* agmv);
u16 AGMV_GetNumberOfChannels(AGMV* agmv);
u32 AGMV_GetAudioSize(AGMV* agmv);
f32 AGMV_GetLeniency(AGMV* agmv);
u8  AGMV_GetVersion(AGMV* agmv);
AGMV_OPT AGMV_GetOPT(AGMV* agmv);
AGMV_COMPRESSION AGMV_GetCompression(AGMV* agmv);
Bool AGMV_GetAudioState(AGMV* agmv);
f32 AGMV_GetVolume(AGMV* agmv);
u16 AGMV_GetBitsPerSample(AGMV* agmv);
AGMV_INFO AGMV_GetVideoInfo(AGMV* agmv);

/* ---- FILE* byte / bit I/O and chunk scan (reference include/agmv_utils.h:23-49).
 * The bit reader and writer share one file-static state exactly like the reference
 * (src/agmv_utils.c:32-36): one encode or decode stream per process at a time. */
Bool AGMV_EOF(FILE* file);
u32  AGMV_ReadBits(FILE* file, u32 num_of_bits);
u8   AGMV_ReadByte(FILE* file);
u16  AGMV_ReadShort(FILE* file);
u32  AGMV_ReadLong(FILE* file);
void AGMV_ReadFourCC(FILE* file, char fourcc[4]);
void AGMV_WriteBits(FILE* file, u32 num, u16 num_of_bits);
void AGMV_WriteByte(FILE* file, u8 byte);
void AGMV_WriteShort(FILE* file, u16 word);
void AGMV_WriteLong(FILE* file, u32 dword);
void AGMV_WriteFourCC(FILE* file, char f, char o, char u, char r);
void AGMV_FlushReadBits(void);
void AGMV_FlushWriteBits(FILE* file);
void AGMV_FindNextFrameChunk(FILE* file);
void AGMV_FindNextAudioChunk(FILE* file);
void AGMV_SkipFrameChunk(FILE* file);
void AGMV_SkipAudioChunk(FILE* file);
void AGMV_ParseAGMV(FILE* file, AGMV* agmv);
Bool AGMV_IsCorrectFourCC(char fourcc[4], char f, char o, char u, char r);

/* ---- small utilities (reference include/agmv_utils.h:94-131) */
int  AGMV_NextIFrame(int n, int frame_count);
int  AGMV_PrevIFrame(int n, int frame_count);
int  AGMV_SkipToNearestIFrame(int n);
u8   AGMV_GetVersionFromOPT(AGMV_OPT opt, AGMV_COMPRESSION compression);
f32  AGMV_ClampVolume(f32 volume);
u16  AGMV_SwapShort(u16 word);
u32  AGMV_SwapLong(u32 dword);
void AGMV_CopyImageData(u32* dest, u32* src, u32 size);
void AGMV_SyncFrameAndImage(AGMV* agmv, u32* img_data);
void AGMV_SyncAudioTrack(AGMV* agmv, const void* pcm);
void AGMV_SignedToUnsignedPCM(u8* pcm, u32 size);
void AGMV_UnsigendToSignedPCM(u8* pcm, u32 size);
u32  AGMV_CalculateTotalAudioDuration(u32 size, u32 sample_rate, u16 num_of_channels, u16 bits_per_sample);
int  AGMV_Abs(int a);
int  AGMV_Min(int a, int b);
u8   AGMV_GetR(u32 color);
u8   AGMV_GetG(u32 color);
u8   AGMV_GetB(u32 color);
u8   AGMV_GetQuantizedR(u32 color, AGMV_QUALITY quality);
u8   AGMV_GetQuantizedG(u32 color, AGMV_QUALITY quality);
u8   AGMV_GetQuantizedB(u32 color, AGMV_QUALITY quality);
u32  AGMV_QuantizeColor(u32 color, AGMV_QUALITY quality);
u32  AGMV_ReverseQuantizeColor(u32 color, AGMV_QUALITY quality);
f32  AGMV_CompareFrameSimilarity(u32* frame1, u32* frame2, u32 width, u32 height);
void AGMV_InterpFrame(u32* interp, u32* frame1, u32* frame2, u32 width, u32 height);
void AGMV_BubbleSort(u32* data, u32* gram, u32 num_of_colors);
char* AGMV_Error2Str(Error error);
u32  AGMV_GetNumberOfBytesRead(u32 bits);
int  AGMV_ResetFrameRate(const char* filename, u32 frames_per_second);

/* ---- the hot path, per frame (reference include/agmv_encode.h:26-31, agmv_decode.h:22,
 * agmv_utils.h:114-116).  All of these run on the GPU. */
u8 AGMV_FindNearestColor(u32 palette[256], u32 color);
AGMV_ENTRY AGMV_FindNearestEntry(u32 palette0[256], u32 palette1[256], u32 color);
/* unused by the library itself (reference src/agmv_utils.c:818-849, :897-914): nearest colour among the first 200
   palette slots; the entry picks the palette with the smaller INDEX.  Host code, kept for API completeness. */
u8 AGMV_FindSmallestColor(u32 palette[256], u32 color);
AGMV_ENTRY AGMV_FindSmallestEntry(u32 palette0[256], u32 palette1[256], u32 color);
u8 AGMV_ComparePFrameBlock(AGMV* agmv, u32 x, u32 y, AGMV_ENTRY* entry);
u8 AGMV_CompareIFrameBlock(AGMV* agmv, u32 x, u32 y, u32 color, AGMV_ENTRY* img_entry);
void AGMV_AssembleIFrameBitstream(AGMV* agmv, AGMV_ENTRY* img_entry);
void AGMV_AssemblePFrameBitstream(AGMV* agmv, AGMV_ENTRY* img_entry);
void AGMV_EncodeHeader(FILE* file, AGMV* agmv);
void AGMV_EncodeFrame(FILE* file, AGMV* agmv, u32* img_data);
u32  AGMV_LZSS(FILE* file, AGMV_BITSTREAM* in);
u32  AGMV_LZ77(FILE* file, AGMV_BITSTREAM* in);
void AGMV_CompressAudio(AGMV* agmv);
void AGMV_EncodeAudioChunk(FILE* file, AGMV* agmv);
int  AGMV_DecodeHeader(FILE* file, AGMV* agmv);
int  AGMV_DecodeFrameChunk(FILE* file, AGMV* agmv);
int  AGMV_DecodeAudioChunk(FILE* file, AGMV* agmv);

/* ---- sequence drivers (reference include/agmv_encode.h:35-37, agmv_decode.h:24-26).
 * Like the reference, the three encoders call DestroyAGMV on `agmv` before returning
 * (src/agmv_encode.c:3625); only AGMV_IMG_BMP input is supported. */
void AGMV_EncodeVideo(const char* filename, const char* dir, const char* basename, u8 img_type, u32 start_frame,
                      u32 end_frame, u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt,
                      AGMV_QUALITY quality, AGMV_COMPRESSION compression);
void AGMV_EncodeAGMV(AGMV* agmv, const char* filename, const char* dir, const char* basename, u8 img_type,
                     u32 start_frame, u32 end_frame, u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt,
                     AGMV_QUALITY quality, AGMV_COMPRESSION compression);
void AGMV_EncodeFullAGMV(AGMV* agmv, const char* filename, const char* dir, const char* basename, u8 img_type,
                         u32 start_frame, u32 end_frame, u32 width, u32 height, u32 frames_per_second,
                         AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression);
int AGMV_DecodeVideo(const char* filename, u8 img_type);
int AGMV_DecodeAGMV(const char* filename, u8 img_type, AGMV_AUDIO_TYPE audio_type);

/* ---- audio tracks (reference include/agmv_encode.h:33, agmv_decode.h:25, agmv_utils.h:101-103, :118, :124-132).  Host C.
 * The format.  "Has audio" means header.total_audio_duration != 0, and the duration is in whole seconds: a track shorter than
 * one second is no track.  audio_size counts samples over all channels, in track order (interleaved).  A 16-bit track is u16
 * words holding the WAV samples' bit patterns (signed samples included); the file stores ONE code byte per sample.  With
 * k = floor(sqrt(s)) for a sample s in 0 .. 65535, in integers:
 *     e1 = k even ? k : (k + 1) & 255            r  = (s > k * k + k ? k + 1 : k) & 255
 *     e2 = r even ? r : (r + 1) & 255            e3 = (s >> 8) | 1
 *     d1 = |e1 * e1 - s|    d2 = |e2 * e2 - s|    d3 = |(e3 << 8) - s|    d = min(d1, d3)
 *     code = d == d1 ? e1 : d == d2 ? e2 : e3
 * (AGMV_CompressAudio, reference src/agmv_encode.c:636-705, with its quirks: the second minimum overwrites the first, rounding up
 * to even wraps from 255 to 0, a root of 256 is 0.)  A code c expands to c * c when even and to (c << 8) & 0xFFFF when odd
 * (src/agmv_decode.c:412-453); the worst round-trip error is 256.  An 8-bit track stores its bytes unchanged.
 * Every frame chunk is followed by 'AGAC', a 4-byte size and `size` codes from a running start_point.  The sequence encoders
 * write the same size into every chunk, (u32)(audio_size / (f32)d), with the reference's divisors: AGMV_EncodeAGMV (PDIFS) takes
 * d = its adjusted frame count, (end_frame - start_frame) / 2 for the heavy opts and * 0.75 for the light ones, and leaves the
 * tail audio_size - size * chunks unwritten; AGMV_EncodeFullAGMV takes d = end_frame - start_frame (src/agmv_encode.c:4024), one
 * less than the chunks it writes, so its chunks ask for more codes than audio_size holds and end in zeros here.  A decoder
 * reads each chunk's own size field.
 * Where the reference reads or leaves memory it never set, this build reads zeros and stays in bounds: AGMV_WavToAudioTrack takes
 * the RIFF size for the data size like the reference, so audio_size exceeds what the file holds by 18 samples (36 for 8 bits)
 * and those are 0; the decoders' track is 0 behind the last chunk; AGMV_EncodeAudioChunk writes 0 for samples past audio_size,
 * AGMV_DecodeAudioChunk drops them (start_point advances all the same).  A file that cannot be opened leaves the object as it
 * was.  AGMV_ExportAudioType writes the reference's bytes, its constant byte rate 75600 and its swapped form names (AGMV_AUDIO_AIFF
 * writes an 'AIFC' form, AGMV_AUDIO_AIFC an 'AIFF' form) included.  AGMV_DecodeAudio writes quick_export.wav / quick_export.aiff
 * into the working directory; AGMV_DecodeAGMV of this build writes no audio file, AGMV_DecodeAudio is the export. */
void AGMV_WavToAudioTrack(const char* filename, AGMV* agmv);
void AGMV_RawSignedPCMToAudioTrack(const char* filename, AGMV* agmv, u8 num_of_channels, u32 sample_rate);
void AGMV_Raw8PCMToAudioTrack(const char* filename, AGMV* agmv);
void AGMV_ExportAudioType(FILE* audio, AGMV* agmv, AGMV_AUDIO_TYPE audio_type);
int  AGMV_DecodeAudio(const char* filename, AGMV_AUDIO_TYPE audio_type);

/* ---- playback helpers (reference include/agmv_playback.h:23-31) */
void AGMV_ResetVideo(FILE* file, AGMV* agmv);
Bool AGMV_IsVideoDone(AGMV* agmv);
void AGMV_SkipForwards(FILE* file, AGMV* agmv, int n);
void AGMV_SkipForwardsAndDecodeAudio(FILE* file, AGMV* agmv, int n);
void AGMV_SkipBackwards(FILE* file, AGMV* agmv, int n);
void AGMV_SkipTo(FILE* file, AGMV* agmv, int n);
void AGMV_PlayAGMV(FILE* file, AGMV* agmv);
void PlotPixel(u32* vram, int x, int y, int w, int h, u32 color);
void AGMV_DisplayFrame(u32* vram, u16 width, u16 height, AGMV* agmv);
/* the finished file as a C array in ./agmv.h (reference src/agmv_utils.c:1577-1615) */
void AGMV_ExportAGMVToHeader(const char* filename);

/* ---- extensions of this build (not in the reference) -------------------------------------- */
/* frames per GPU batch of the sequence drivers (default 64; env AGMV_BATCH_FRAMES) and host
   threads for the LZ stage (default: online cores, env AGMV_LZ_THREADS) */
void AGMV_SetBatchFrames(unsigned frames);
void AGMV_SetLZThreads(unsigned threads);
/* GPUs the sequence encoders (AGMV_EncodeAGMV / EncodeFullAGMV / EncodeVideo) spread their GOP-aligned batches over, from this
   one host process (default 1; env AGMV_DEVICES); the output is the same file whatever the number */
void AGMV_SetDevices(unsigned devices);
/* canonical synthetic clip agmv_synth_v1: frame t as 4-byte 0x00RRGGBB pixels */
void AGMV_SynthFrame(unsigned* pix, unsigned w, unsigned h, unsigned t, unsigned long long seed);
/* palette build of the encoders (reference src/agmv_encode.c:2364-2656) from a 2^19-bin histogram
   of AGMV_QuantizeColor codes (the +1 initial count is added inside).  pal0/pal1: 256 words each. */
void AGMV_BuildPalette(const unsigned* hist, AGMV_QUALITY quality, AGMV_OPT opt, u32 pal0[256], u32 pal1[256]);

/* Palette refinement: the colours AGMV_BuildPalette picks, moved by weighted k-means (Lloyd's algorithm) over the histogram.
   Opt-in; the file format does not change, only the colours in the header's palettes do.  Everything is exact integer work:
     points     every AGMV_QuantizeColor code of the quality with hist[code] > 0 (the all-ones code included; bins above the
                quality's largest code are not read).  Its weight is w = hist[code], without the +1 AGMV_BuildPalette adds.  Its
                colour is the centre of its bin: the channels of AGMV_ReverseQuantizeColor(code) plus half a step,
                HIGH R +2, G +2, B +1;  MID R +4, G +2, B +2;  LOW R +4, G +2, B +4.
     centroids  k colours 0x00RRGGBB, c[0 .. k-1].  The first n_free move, the others are pinned.
     a round    1. every point goes to the j that minimises (r-cr)^2 + (g-cg)^2 + (b-cb)^2, the lowest j on a tie (the metric and
                   the tie rule of AGMV_FindNearestColor); pinned centroids take part;
                2. for every j < n_free whose points weigh W_j > 0 each channel of c[j] becomes (sum of w * channel + W_j div 2)
                   div W_j, in exact 64-bit unsigned sums.  A centroid with W_j = 0 and a pinned one keep their colour.
     stopping   at most `iterations` rounds, and none after the first round that changes no centroid.  rounds counts those
                that changed at least one.  sse[0] is the sum of w * (distance to the assigned centroid) over the points before
                the first round, sse[1] the same for the centroids returned, both modulo 2^64.
   AGMV_BuildPaletteRefined starts from the pick list of AGMV_BuildPalette (its picks before the slot map, as colours through
   AGMV_ReverseQuantizeColor): k = n_free = 256 for the 256-colour opts; k = 512, n_free = 511 for the others, with c[511] = 0
   pinned -- the reference drops pick 511, and palette0[126], which the slot map never fills, is a black the encoder can choose,
   so the pinned centroid stands for that slot.  The slot map then scatters c[0 .. 510] (c[0 .. 255]) as it scatters the picks.
   The refinement runs on the library's device (agmv_hip_palette_refine_dev of include/agmv_hip.h).  With iterations == 0 the
   call IS AGMV_BuildPalette and opens no device.  sse may be NULL.  Returns 0, or -1 for a NULL pointer or an unknown enum value;
   a GPU failure aborts with a message, as in the encoders.
   AGMV_SetPaletteRefine sets the rounds the sequence encoders (all three BMP drivers and every AGMV_EncodeFrames*Dev) ask for:
   0 = not set, then env AGMV_PALETTE_REFINE decides, and without it the refinement is off and every file is what it was
   without this knob; values above 64 count as 64.  With AGMV_TRACE in the environment the rounds, both distortions and the
   stage's time are printed. */
int AGMV_BuildPaletteRefined(const unsigned* hist, AGMV_QUALITY quality, AGMV_OPT opt, u32 pal0[256], u32 pal1[256], unsigned iterations,
                             unsigned long long sse[2]);
void AGMV_SetPaletteRefine(unsigned iterations);

/* Pattern dithering: every pixel of a clip replaced by one of 16 palette colours whose mean approaches it, before the encoder
   quantises it.  Opt-in; the file format does not change.  The dither is positional (a 4x4 threshold matrix, the size of the
   codec's blocks), never error diffusion: a pixel's result depends on its colour and on (x & 3, y & 3) alone, so content that
   does not move stays equal from frame to frame and the P-frames' COPY blocks survive.  Everything is integer work:
     px        the pixel (R, G, B); bits >= 24 are ignored.  (x, y) is its position inside its own frame.
     LUT       the exact nearest entry of a colour in the palette, by the rules of AGMV_FindNearestColor (256-colour opts) /
               AGMV_FindNearestEntry (512-colour opts); an entry is pal_num << 8 | index, col(e) its colour.
     s         the strength, 1 .. 64.
       acc = (0, 0, 0)                                   signed, per channel
       for i = 0 .. 15:
           a   = clamp(px + ((acc * s) >> 6), 0, 255)    per channel; >> is arithmetic (rounds down)
           e_i = LUT[a]
           acc = acc + px - col(e_i)
       key_i = (299 * R + 587 * G + 114 * B of col(e_i)) * 512 + e_i
       sort the 16 keys ascending;  t = B4[y & 3][x & 3]
       out(x, y) = col(entry of the t-th key)            as 0x00RRGGBB
     B4        has the rows  0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5.
   |acc| <= 16 * 255 and the keys stay below 2^27; equal keys are the same entry, so the sort needs no stability rule.  What
   follows: the output is always a palette colour with a zero high byte; a pixel whose colour is in the palette comes back as
   it is; the result never depends on the frame number or on a linear index.  agmv_hip_dither_frames_async of
   include/agmv_hip.h is the kernel.
   AGMV_SetDither sets the strength for the sequence encoders (all three BMP drivers and every AGMV_EncodeFrames*Dev, from every
   pixel layout and with a scale): 0 = not set, then env AGMV_DITHER decides (1 .. 64, anything else is off), and without it the
   dither is off and every file is what it was without this knob; values above 64 count as 64.  The knob is read when a sequence
   is opened.  What is dithered is exactly what the encoder would have seen, frame by frame, PDIFS midpoints included; the
   palette's histogram, the palette refinement and the adaptive schedule's similarity counts read the undithered source.
   AGMV_EncodeFrame (one frame, FILE*) is not affected.  With AGMV_TRACE in the environment the strength is printed. */
void AGMV_SetDither(unsigned strength);

/* Temporal stabilisation: blocks of a P-frame that differ from their GOP's I-frame by no more than the source's own noise receive
   the I-frame's pixels, before the encoder quantises them.  Opt-in; the file format does not change.  The encoder makes a block a
   one-byte COPY only when 13 of its 16 palette colours lie within +-2 of the I-frame's at the same pixel; a source whose pixels
   move by two or three levels from frame to frame (a camera, temporal dither, model output) loses that, and this gives it back.
   The rule acts on a batch of XRGB32 frames with frame counts fc = first_fc + k, in place, in integers only:
     anchor    of frame k is frame k - (fc & 3) of the same batch: the I-frame of its GOP, by the encoder's own frame_count % 4
               rule.  Frames with fc & 3 == 0 are never changed; frames whose anchor lies before the batch are never changed.
     block     4x4 pixels, aligned to the frame; w and h are multiples of 4.
     d         the 48 absolute channel differences between a block and the anchor's block at the same place, over bits 0 .. 23
               only.
     s         the strength, 1 .. 64.
       still     = max(d) <= s  and  sum(d) <= 12 * s          (a mean difference of at most s / 4)
       a still block receives the anchor's 16 pixels & 0x00FFFFFF;
       any other block keeps every bit it had, bits 24 .. 31 included.
   What follows: the result is idempotent (a replaced block differs by 0 and is replaced by the same words again); a replaced
   block is a COPY block whatever the palette; I-frames, and with them everything the palette is built from, are untouched; a GOP
   depends on nothing outside itself, so batches and devices need no exchange.  agmv_hip_stabilise_frames_async of
   include/agmv_hip_stabilise.h is the kernel.
   AGMV_SetStabilise sets the strength for the sequence encoders (all three BMP drivers and every AGMV_EncodeFrames*Dev, from every
   pixel layout and with a scale): 0 = not set, then env AGMV_STABILISE decides (1 .. 64, anything else is off), and without it the
   stabilisation is off and every file is what it was without this knob, launch for launch; values above 64 count as 64.  The knob
   is read when a sequence is opened.  What is stabilised is exactly what the encoder would have seen, frame by frame, PDIFS
   midpoints included, and BEFORE the dither: the dither is positional, so equal blocks stay equal and COPY survives both.  The
   palette's histogram, the palette refinement and the adaptive schedule's similarity counts read the source as it is.
   AGMV_EncodeFrame (one frame, FILE*) is not affected.
   AGMV_GetStabiliseStats reports the last sequence encode of this process: examined = the blocks of the P-frames that had
   their anchor in their batch, replaced = those that were replaced, summed over the GPU workers and devices (each worker owns one
   device counter, downloaded once when the sequence closes).  Both are zero when the knob was off.  With AGMV_TRACE in the
   environment the strength and the two counts are printed. */
typedef struct AGMV_STABILISE_STATS { unsigned long long examined, replaced; } AGMV_STABILISE_STATS;
void AGMV_SetStabilise(unsigned strength);
void AGMV_GetStabiliseStats(AGMV_STABILISE_STATS* out);

/* Sequences from and to frames in GPU memory: the .agmv files of the three BMP drivers without the BMPs.
   d_frames is device memory of the library's own device (env AGMV_DEVICE, default 0; AGMV_DEVICES is not consulted),
   [num_of_frames][height][width] pixels of 4 bytes, 0x00RRGGBB (bits >= 24 are ignored).
   The library works on streams of its own: the frames must be complete when AGMV_EncodeFramesDev is called, and the decoded
   frames are complete when AGMV_DecodeFramesDev returns.
   AGMV_EncodeFramesDev writes, byte for byte, the file the BMP driver of the schedule writes for f1.bmp .. f<n>.bmp holding the
   same frames: FULL = AGMV_EncodeFullAGMV, PDIFS = AGMV_EncodeAGMV (both on CreateAGMV(n, w, h, fps), frames 1 .. n),
   ADAPTIVE = AGMV_EncodeVideo(frames 1 .. n), with its CreateAGMV(n - 1, ...), per-opt leniency and header patch.  For the GBA
   and NDS opts width / height are the SOURCE size; GBA_GEN_AGMV.h is not written.  Returns 0, or -- before any file is
   created -- a negative value: -1 NULL pointer or unknown enum value, -2 fewer frames than the schedule's first group reads
   (4 light PDIFS / adaptive, 2 heavy, 1 FULL), -3 width or height that cannot be encoded (not a multiple of 4 for an opt that
   does not scale).  A GPU failure inside the encoder aborts with a message, as in the BMP drivers.
   AGMV_DecodeFramesDev is AGMV_DecodeAGMV with another destination: frame k of the file (0-based) lands at
   d_frames + k * width * height.  It decodes at most cap_frames frames and returns their number, or a negative Error.
   *info (may be NULL) receives the header's AGMV_INFO; with d_frames NULL nothing is decoded and only *info is filled, so the
   caller can size the buffer. */
typedef enum AGMV_SCHEDULE { AGMV_SCHEDULE_FULL = 0x1, AGMV_SCHEDULE_PDIFS = 0x2, AGMV_SCHEDULE_ADAPTIVE = 0x3 } AGMV_SCHEDULE;
int AGMV_EncodeFramesDev(const char* filename, const unsigned* d_frames, u32 num_of_frames, u32 width, u32 height,
                         u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression,
                         AGMV_SCHEDULE schedule);
int AGMV_DecodeFramesDev(const char* filename, unsigned* d_frames, u32 cap_frames, AGMV_INFO* info);

/* The same two calls on clips in the layouts that video readers, models and image decoders hold.  One frame is:
     AGMV_PIXFMT_XRGB32  [h][w] little-endian words 0x00RRGGBB; bits >= 24 ignored on input, 0 on output (the layout above)
     AGMV_PIXFMT_RGB24   [h][w][3] bytes R, G, B
     AGMV_PIXFMT_BGR24   [h][w][3] bytes B, G, R
     AGMV_PIXFMT_RGBA32  [h][w][4] bytes R, G, B, A; A ignored on input, 0xFF on output
     AGMV_PIXFMT_RGB8P   [3][h][w] bytes: plane R, plane G, plane B
   Frames of a clip lie back to back; no alignment is asked for beyond 1 byte (4 for XRGB32).  The kernels that touch the clip
   read and write it in that layout: no packed copy of more than one batch of frames exists on the device, and the files are
   the same bytes whatever the layout.  AGMV_EncodeFramesFmtDev / AGMV_DecodeFramesFmtDev take, mean and return what
   AGMV_EncodeFramesDev / AGMV_DecodeFramesDev do (which are the XRGB32 case); an unknown format is -1 before any file is
   created and before a device is opened.  Frame k of a decoded file lands agmv_hip_pixfmt_frame_bytes(fmt, width * height)
   * k bytes into d_frames (include/agmv_hip.h); frames behind cap_frames are not touched. */
typedef enum AGMV_PIXFMT {
	AGMV_PIXFMT_XRGB32 = 1, AGMV_PIXFMT_RGB24 = 2, AGMV_PIXFMT_BGR24 = 3, AGMV_PIXFMT_RGBA32 = 4, AGMV_PIXFMT_RGB8P = 5
} AGMV_PIXFMT;

/* 8-bit YUV 4:2:0, what video decoders deliver and video encoders take.  These two values continue AGMV_PIXFMT (6 stays an
   unknown format) and are passed in the same `fmt` argument, OR-ed with the two flags below.  A frame is w x h pixels, with
   cw = (w + 1) / 2 and ch = (h + 1) / 2 in integers; frames lie back to back, w * h + 2 * cw * ch bytes each
   (agmv_hip_yuv_frame_bytes of include/agmv_hip.h), and no alignment is required.
     AGMV_PIXFMT_NV12  [h][w] bytes Y, then [ch][cw][2] bytes U, V
     AGMV_PIXFMT_I420  [h][w] bytes Y, then [ch][cw] bytes U, then [ch][cw] bytes V
   Flags: AGMV_YUV_BT709 (default BT.601) and AGMV_YUV_FULL_RANGE (default limited range).  A flag on the formats 1 .. 5, any
   other bit above 0xFF and any other base value is an unknown format: -1 before a file is created or a device is opened.

   Reading.  Pixel (x, y) takes Y at (x, y) and U, V at (x >> 1, y >> 1): nearest chroma, no interpolation.  With
   C = ky * (Y - yo), D = U - 128, E = V - 128 in 32-bit signed integers and >> an arithmetic shift,
     R = clip8((C + rv * E + 128) >> 8),  G = clip8((C - gu * D - gv * E + 128) >> 8),  B = clip8((C + bu * D + 128) >> 8)
                        ky   yo   rv   gu   gv   bu
     BT.601 limited    298   16  409  100  208  516
     BT.709 limited    298   16  459   55  136  541
     BT.601 full       256    0  359   88  183  454
     BT.709 full       256    0  403   48  120  475
   Writing (the decoder's sink).  Y = clip8(((yr * R + yg * G + yb * B + 128) >> 8) + yo) per pixel.  For each chroma sample take
   the pixels of its 2 x 2 block that exist (cnt = 4, 2 or 1 at odd edges), average each of R, G, B over them as
   (sum + (cnt >> 1)) / cnt, then U = clip8(((ur * R + ug * G + ub * B + 128) >> 8) + 128), and V likewise.
                       yr  yg  yb   yo     ur   ug   ub     vr    vg   vb
     BT.601 limited    66 129  25   16    -38  -74  112    112   -94  -18
     BT.709 limited    47 157  16   16    -26  -86  112    112  -102  -10
     BT.601 full       77 150  29    0    -43  -85  128    128  -107  -21
     BT.709 full       54 183  19    0    -29  -99  128    128  -116  -12
   Every chroma row sums to 0, so greys stay at U = V = 128.  A YUV clip stands for the XRGB32 clip that this reading gives: the
   palette, the adaptive schedule's decisions, the GBA / NDS scaling and the encoded file are those of that clip, byte for byte,
   and a file decoded into a YUV sink is the XRGB32 decode with the writing rule applied. */
enum { AGMV_PIXFMT_NV12 = 16, AGMV_PIXFMT_I420 = 17, AGMV_YUV_BT709 = 0x100, AGMV_YUV_FULL_RANGE = 0x200 };
int AGMV_EncodeFramesFmtDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 width, u32 height,
                            u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression,
                            AGMV_SCHEDULE schedule);
int AGMV_DecodeFramesFmtDev(const char* filename, void* d_frames, AGMV_PIXFMT fmt, u32 cap_frames, AGMV_INFO* info);

/* A clip scaled to a target size, then encoded: 1080p or 720p frames of a GPU pipeline to the 320x240, 240x160 or 120x80 files
   this codec is for.  A source clip of sw x sh pixels per frame (src_width x src_height; need not be multiples of 4) in the layout
   `fmt` stands for the XRGB32 clip S of that size, by the reading the text above gives for every layout, YUV included.  The scale
   to dw x dh (width x height) with `filter` gives the XRGB32 clip D defined below, and the file is, byte for byte, the file
   AGMV_EncodeFramesDev writes for D: the palette (its histogram is that of D), the adaptive schedule's decisions, the PDIFS
   midpoints, the header and the chunks.  `div` is the integer quotient of non-negative integers.
     AGMV_SCALE_NEAREST  D(X, Y) = S(((2X + 1) * sw) div (2 * dw), ((2Y + 1) * sh) div (2 * dh)): the source pixel under the target
                         pixel's centre, in integers (64-bit on the host).  Any non-zero target size, upscales included.
     AGMV_SCALE_AREA     the exact box filter, downscale only (dw <= sw and dh <= sh).  On an axis source pixel i occupies
                         [i * dw, (i + 1) * dw) and target pixel X occupies [X * sw, (X + 1) * sw); wx(X, i) is the length of their
                         overlap, an integer in 0 .. dw, and the wx of one X sum to sw.  wy(Y, j) likewise from sh and dh.  Per
                         channel  D(X, Y) = (sum over j, i of wy(Y, j) * wx(X, i) * S(i, j) + (sw * sh) div 2) div (sw * sh).
                         The channels are averaged in RGB, never in YUV.  Hence: a scale to the same size is the identity; a scale by
                         an integer factor k is the mean of each k x k block, rounded half up; a source pixel contributes to at most
                         2 target columns and 2 target rows.  sw * sh <= 2^24 is required (3840 x 2160 fits): then
                         255 * sw * sh + (sw * sh) div 2 < 2^32 and every sum is exact in 32-bit unsigned arithmetic.
   D is materialised once on the library's device, 4 * width * height * num_of_frames bytes (1080p NV12 to 320x240: 0.3 MB per frame
   against 3.1 MB of source), freed before the call returns; the source is read once, in its own layout, and nothing of its size is
   allocated.  Returns 0, or a negative value.  -1, -2 and -3 come before a file is created, before d_frames is read and before a
   device is opened, and are looked for in this order:
     -1  NULL pointer; unknown enum value (the filter included); unknown format
     -3  width or height zero or not a multiple of 4; a zero source size (or one above 2^28 pixels); AGMV_SCALE_AREA with a target
         larger than the source in either axis, or with src_width * src_height > 2^24; a GBA / NDS opt
     -2  fewer frames than the schedule's first group reads (as for AGMV_EncodeFramesDev)
     -4  the scaled clip cannot be allocated: after the device is opened, still before a file is created
   The GBA / NDS opts bring their own nearest scaler, fixed target sizes and leniency: they stay on AGMV_EncodeFramesDev /
   AGMV_EncodeFramesFmtDev and are refused here.  AGMV_OPT_I / _II / _III with a 120 x 80 target write files of the same container
   version and palette mode as AGMV_OPT_GBA_I / _II / _III (AGMV_GetVersionFromOPT depends only on the colour count and the
   compression), and of the same PDIFS weight for _I and _III; AGMV_OPT_GBA_II is heavy where AGMV_OPT_II is light, its
   counterpart in weight is AGMV_OPT_ANIM. */
typedef enum AGMV_SCALE { AGMV_SCALE_NEAREST = 1, AGMV_SCALE_AREA = 2, AGMV_SCALE_BILINEAR = 3 } AGMV_SCALE;
int AGMV_EncodeFramesScaledDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height,
                               u32 width, u32 height, AGMV_SCALE filter, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality,
                               AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule);

/* A file decoded at a target size: the 120x80 .. 320x240 frames of this codec as the 1080p NV12 a video encoder takes, a model's
   input size, or thumbnails.  The file of sw x sh decodes to the XRGB32 clip S, which is what AGMV_DecodeFramesDev gives; a target
   size dw x dh (width x height) and `filter` give the XRGB32 clip D defined below, and d_frames receives D in the layout `fmt` by
   the writing rule the text above states for that layout -- NV12 / I420: luma per pixel of D, chroma from the pixels of D's 2 x 2
   block that exist.  Frame k lands k * (frame bytes of fmt at dw x dh) bytes into d_frames; frames behind cap_frames are not
   touched.  All integer: the same bytes from every run.  `div` and `mod` are the integer quotient and remainder of non-negative integers.
     AGMV_SCALE_NEAREST   the rule above.  Any non-zero target size.
     AGMV_SCALE_AREA      the rule above, under its conditions: dw <= sw, dh <= sh, sw * sh <= 2^24.
     AGMV_SCALE_BILINEAR  pixel centres aligned, edges clamped, 8-bit weights, one rounding.  Any non-zero target size in either
                          direction; a downscale reads four source pixels per target pixel whatever the ratio, so it aliases (use
                          AGMV_SCALE_AREA for that).  On an axis with source length s and target length d the taps of target
                          index X are: p = (2X + 1) * s - d, signed; if p < 0 then i0 = 0 and f = 0, otherwise i0 = p div 2d,
                          r = p mod 2d, f = (256 * r + d) div 2d, which lies in 0 .. 256; i1 = min(i0 + 1, s - 1).  With
                          (x0, x1, fx) from (sw, dw) and (y0, y1, fy) from (sh, dh), per channel
                            D(X, Y) = ((256 - fy) * ((256 - fx) * S(x0, y0) + fx * S(x1, y0))
                                       + fy * ((256 - fx) * S(x0, y1) + fx * S(x1, y1)) + 32768) >> 16
                          Every term fits 32-bit unsigned arithmetic: 255 * 65536 + 32768 < 2^32.  Hence: a scale to the same size
                          is the identity; a flat frame stays flat; every output lies between the smallest and the largest of its
                          four taps; the channels are interpolated in RGB, never in YUV.  AGMV_EncodeFramesScaledDev refuses
                          this filter (-1).
   The batches are decoded at the file's size; the decoder's state never leaves that size, and no XRGB32 copy of D exists for
   NEAREST and BILINEAR (AREA into a layout other than XRGB32 goes through one batch of D).  Returns the number of frames decoded, or
   a negative value; *info (may be NULL) receives the header's AGMV_INFO, with the file's own size.  The checks, in this order, all
   before a device is opened:
     -1        NULL filename; unknown format; unknown filter
     -4        width or height zero, or more than 2^28 target pixels
     -Error    the file cannot be opened or its header is bad (as AGMV_DecodeFramesFmtDev)
      0        d_frames NULL: only *info is filled
     -4        AGMV_SCALE_AREA with a target larger than the file's frame in either axis, or a file frame above 2^24 pixels */
int AGMV_DecodeFramesScaledDev(const char* filename, void* d_frames, AGMV_PIXFMT fmt, u32 width, u32 height, AGMV_SCALE filter, u32 cap_frames,
                               AGMV_INFO* info);

/* Normalised float tensors: what a model takes and gives.  A tensor clip is n frames of [3][h][w] elements -- planes R, G, B,
   back to back (NCHW) -- of the type an AGMV_TENSORFMT names, aligned to its element:
     AGMV_TENSOR_F32   IEEE binary32
     AGMV_TENSOR_F16   IEEE binary16
     AGMV_TENSOR_BF16  the upper 16 bits of a binary32
   It carries a normalisation mean[3], std[3] (float, channel 0 = R), and a byte v of channel c stands for
   (v / 255 - mean[c]) / std[c].  Bounds: 2^-32 <= |std[c]| <= 2^32 and |mean[c]| <= 2^32, both finite; anything else (and an
   unknown type) is -1 before a device is opened.  Inside these bounds no outcome depends on whether the device flushes subnormals:
   the table below is made on the host and only copied by the device, and where an input, the product or the sum of the reading
   rule is a float32 subnormal, t lies so close to 0 that the byte is 0 with and without the flush.

   Writing (the decoder's sink) is exact by construction, because it is a table.  T[c][v], 3 x 256 entries, is the float32
   nearest to the double ((double)v / 255.0 - (double)mean[c]) / (double)std[c]; for F16 / BF16 that float32 is rounded to
   nearest-even into the type, overflow giving an infinity of its sign.  The host builds the table in integers where it narrows
   (agmv_hip_tensor_table of include/agmv_hip.h) and the kernel only looks it up:
     out[k][c][y][x] = T[c][channel c of D(x, y)]
   where D is the XRGB32 decode, or with a target size the clip AGMV_DecodeFramesScaledDev defines for the filter.

   Reading (the encoder's source).  With a[c] = (float)(255.0 * (double)std[c]) and b[c] = (float)(255.0 * (double)mean[c]) an
   element x of channel c, converted exactly to float32, gives
     t = fl32(fl32(x * a[c]) + b[c])          two separately rounded float32 operations, never a fused one
     v = 0 for a NaN, else (int)rintf(fminf(fmaxf(t, 0), 255)), rounding half to even
   so -inf and everything below 0 give 0, +inf and everything above 255 give 255.  A tensor clip stands for the XRGB32 clip this
   reading gives: the palette, the schedules' decisions and the file are those of that clip, byte for byte.  For the usual
   normalisations reading what was written returns every v (tests/test_tensor_cpu.py).

   AGMV_DecodeFramesTensorDev is AGMV_DecodeFramesScaledDev into a tensor clip: width == height == 0 means the file's size, and
   `filter` is then ignored.  The batches are decoded at the file's size, the table is uploaded once per call, and the sink is
   one launch per batch (AGMV_SCALE_AREA goes through one batch of D).  Frame k lands k * 3 * width * height elements into
   d_tensor.  Returns and the order of the checks are AGMV_DecodeFramesScaledDev's, with -1 also for an unknown type or a refused
   normalisation; with d_tensor NULL only *info is filled.
   AGMV_EncodeFramesTensorDev materialises the XRGB32 clip of the reading rule on the library's device with one launch
   (agmv_hip_tensor_to_xrgb_async; 4 * width * height * num_of_frames bytes, a third to two thirds of the source), takes the path
   of AGMV_EncodeFramesDev on it and frees it before it returns.  It returns what AGMV_EncodeFramesDev returns for that clip
   (-1, also for an unknown type or a refused normalisation, -5, -2, -3), all before a device is opened, and -4 when the clip
   cannot be allocated.  A pending AGMV_SetAudioDev track, the dither and the palette refinement apply as for the other
   AGMV_EncodeFrames*Dev; the track is consumed whatever the call returns. */
typedef enum AGMV_TENSORFMT { AGMV_TENSOR_F32 = 1, AGMV_TENSOR_F16 = 2, AGMV_TENSOR_BF16 = 3 } AGMV_TENSORFMT;
int AGMV_DecodeFramesTensorDev(const char* filename, void* d_tensor, AGMV_TENSORFMT type, const float mean[3], const float std[3], u32 width,
                               u32 height, AGMV_SCALE filter, u32 cap_frames, AGMV_INFO* info);
int AGMV_EncodeFramesTensorDev(const char* filename, const void* d_tensor, AGMV_TENSORFMT type, const float mean[3], const float std[3],
                               u32 num_of_frames, u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality,
                               AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule);

/* A view of a file: 16 frames at stride 4 from somewhere inside it, a 224 x 224 window of them, as a model takes them -- without
   a tensor that holds the whole file.  A view selects the frames first, first + step, first + 2 * step, ... of the file and of
   each the window [x, x + width) x [y, y + height) of its pixels.  The contract, for every file, damaged ones included:
     frame j of a view is the window of frame first + j * step of the full decode (AGMV_DecodeFramesDev).
   Everything behind the selection applies to the window as to a file of that size: the layout `fmt`, a target size and its
   filter (AGMV_DecodeFramesScaledDev), the normalisation of a tensor clip (AGMV_DecodeFramesTensorDev).  The fields are plain
   32-bit `unsigned` (u32 is `unsigned long` here):
     view == NULL            the whole file
     step                    >= 1
     count                   0 means "to the end of the file"; a selection that runs past the file's last frame is cut there;
                             `first` at or behind the end delivers 0 frames and writes nothing
     width == height == 0    the full frame; x and y must then be 0.  Otherwise the window must lie inside the file's frame
   A target width == height == 0 means no scaling, and `filter` is not read, as in AGMV_DecodeFramesTensorDev.  cap_frames counts
   frames of the view; frame j lands j * (frame bytes of the layout at the target's, else the window's, size) bytes into the
   destination, and frames behind cap_frames are not touched.  Returns the number of view frames delivered, or a negative value;
   *info (may be NULL) receives the header's AGMV_INFO as always.  The checks, in this order, all before a device is opened:
     -1        NULL filename; unknown format, type or normalisation; unknown filter when a target is given; step == 0; exactly one
               of view->width, view->height zero; x or y not zero with a zero window
     -4        a target with a width or height of zero, or more than 2^28 target pixels
     -Error    the file cannot be opened or its header is bad (as AGMV_DecodeFramesFmtDev)
      0        the destination is NULL: only *info is filled
     -4        the window does not lie inside the frame; AGMV_SCALE_AREA with a target larger than the window in either axis, or a
               file frame above 2^24 pixels; NV12 / I420 without a target size over a window of odd width or height
   How it runs.  The view that selects everything (first 0, step 1, the full frame) is the decode without a view, launch for
   launch, of as many frames as it delivers.  Any other view ends behind the last frame it needs.  The LZ stage runs for every
   frame from 0 up to there, in order: bytes [bpos, bpos + 16) of a frame's row come from the ONE persistent buffer of the
   reference's decoder, which only the LZ output of all earlier frames makes right.  The GPU stage -- parse, reconstruct, I-frame
   snapshot, sink -- starts at the GOP that holds `first`, frame g0 = first & ~3, from the state of a fresh decoder.  When g0 > 0 the
   decoder is asked once, behind the first batch it decoded, whether a pixel of that batch derives from the state before it
   (agmv_hip_decode_prior_dependent of include/agmv_hip.h: exact, per pixel); if so -- a COPY in the I-frame, a stream that ends
   early, a file of width 4 -- the call is run again with the GPU stage from frame 0 and writes the same destinations.  Every later
   batch follows from the first by the decoder's own state hand-over.  The selected windows of a batch are packed by one copy
   launch (agmv_hip_view_frames_async of include/agmv_hip_view.h) into a buffer of one batch of windows, which the sink reads as it reads a batch of a file of
   the window's size; a packed XRGB32 destination without a target receives that copy directly, and consecutive full frames go to
   the sink from where they were decoded.  A batch without a selected frame runs no sink launch.
   AGMV_GetViewStats reports what the last AGMV_DecodeViewDev / AGMV_DecodeViewTensorDev of this process did -- of a restarted
   call, what the run that delivered did: lz_frames = frames through the LZ stage, gpu_frames = frames through the GPU stage,
   delivered = the call's return value (0 for a negative one), restarts = 0 or 1.  All zero behind a call that did not reach the decode. */
typedef struct AGMV_VIEW { unsigned first, count, step; unsigned x, y, width, height; } AGMV_VIEW;
typedef struct AGMV_VIEW_STATS { unsigned lz_frames, gpu_frames, delivered, restarts; } AGMV_VIEW_STATS;
int AGMV_DecodeViewDev(const char* filename, void* d_frames, AGMV_PIXFMT fmt, u32 width, u32 height, AGMV_SCALE filter, const AGMV_VIEW* view,
                       u32 cap_frames, AGMV_INFO* info);
int AGMV_DecodeViewTensorDev(const char* filename, void* d_tensor, AGMV_TENSORFMT type, const float mean[3], const float std[3], u32 width,
                             u32 height, AGMV_SCALE filter, const AGMV_VIEW* view, u32 cap_frames, AGMV_INFO* info);
void AGMV_GetViewStats(AGMV_VIEW_STATS* out);

/* Deblocking: the edges of the 4x4 block grid of a decoded clip smoothed between reconstruction and the sink.  Opt-in; the decoder's
   own state is never filtered.  What a file decodes to is dominated by flat FILL blocks, a gradient comes back as a staircase of
   squares, and a scaling sink magnifies every step; this is the decoder's counterpart of the encoder's dither.  The rule, in
   integers only, which tests/deblock_cases.py states in numpy:
     frames    w x h packed XRGB32 pixels, w and h multiples of 4.  Channels are the three low bytes; bits 24 .. 31 of every pixel
               are copied from the source.
     s         the strength, 1 .. 64.
     stage 1   vertical edges: for every row y and every x = 4, 8, ..., w - 4 the line p1 p0 | q0 q1 = columns x-2, x-1, x, x+1 of
               the decoded frame.
     stage 2   horizontal edges: for every column x and every y = 4, 8, ..., h - 4 the line p1 p0 | q0 q1 = rows y-2, y-1, y, y+1 of
               stage 1's result.  Each stage is a function of its input only.
     decision  per line, over R, G and B together:  step = max_c |p0_c - q0_c|,  side = max_c max(|p1_c - p0_c|, |q1_c - q0_c|).
               A line with step = 0 or step > s is left as it is; any other line is STRONG when side <= s >> 2, else WEAK.
     weak      per channel  p0' = (p1 + 2 p0 + q0 + 2) >> 2,  q0' = (p0 + 2 q0 + q1 + 2) >> 2;  p1 and q1 are kept.
     strong    per channel, with a = p1 + p0 and b = q0 + q1:
               p1' = (7a + b + 8) >> 4,  p0' = (5a + 3b + 8) >> 4,  q0' = (3a + 5b + 8) >> 4,  q1' = (a + 7b + 8) >> 4
               (two flat blocks A | B become the ramp 7:1, 5:3, 3:5, 1:7).
     counters  the weak and the strong lines of both stages, two 64-bit counts; the same clip gives the same counts on every run.
   What follows: every result lies in 0 .. 255; a frame without a step across a block edge comes back unchanged; every pixel
   belongs to exactly one line per stage, so the 4x4 cell around a block corner (pixels 4i-2 .. 4i+1 x 4j-2 .. 4j+1, clipped at
   the rim) depends on its own 16 pixels alone and the rule needs no halo.  agmv_hip_deblock_frames_async of
   include/agmv_hip_deblock.h is the kernel.
   AGMV_SetDeblock sets the strength for the sequence decoders -- AGMV_DecodeFramesDev, ...FmtDev, ...ScaledDev, ...TensorDev,
   AGMV_DecodeViewDev, ...ViewTensorDev, AGMV_MeasureFileDev and the BMP export of AGMV_DecodeAGMV / AGMV_DecodeVideo: 0 = not set,
   then env AGMV_DEBLOCK decides (a decimal number 1 .. 64 and nothing else in the value; anything else is off), and without it the filter is off and every decode is what it was
   without this knob, launch for launch; values above 64 count as 64.  The knob is read when a decode is opened.  Each batch is
   filtered once, whole frames at the file's size, behind the decoder's I-frame snapshot and in front of the sink: before a view's
   window and stride and before any scaling, so frame j of a deblocked view is the window of frame first + j * step of the
   deblocked full decode.  The last frame and the I-frame snapshot that the next batch decodes from stay unfiltered.
   AGMV_DecodeFrameChunk (one frame, FILE*, state in the AGMV object) is NOT covered.
   AGMV_GetDeblockStats reports the last sequence decode of this process (zeroed when it opens, set when it closes): the
   strength, the frames filtered (for a view: those from the GOP it starts at), lines = frames * ((w/4 - 1) * h + (h/4 - 1) * w)
   examined, and the weak and strong counts.  All zero when the knob was off.  With AGMV_TRACE in the environment the strength is
   printed at open and the counts at close. */
typedef struct AGMV_DEBLOCK_STATS { unsigned strength, frames; unsigned long long lines, weak, strong; } AGMV_DEBLOCK_STATS;
void AGMV_SetDeblock(unsigned strength);
void AGMV_GetDeblockStats(AGMV_DEBLOCK_STATS* out);

/* A view of a clip encoded: 1080p60 NV12 from a capture as the 240 x 160, 15 fps file of this codec -- every 4th frame, the centred
   1440 x 1080 window of each, scaled -- without a copy of the selection.  The view is the AGMV_VIEW above with the same field rules,
   now resolved against the clip of num_of_frames frames of src_width x src_height in the layout `fmt`: view == NULL is the whole
   clip, count == 0 means "to the end", a selection that runs past the last frame is cut there, width == height == 0 is the full
   frame.  Let S be the XRGB32 clip the source stands for by its reading rule and V the XRGB32 clip of the selected windows,
     V[j][r][c] = S[first + j * step][y + r][x + c]
   (an NV12 / I420 pixel keeps the chroma sample of its 2 x 2 cell of the source frame, so a window may start and end anywhere).
     width == height == 0   the file is, byte for byte, what AGMV_EncodeFramesDev writes for V; `filter` is not read
     otherwise              the file is, byte for byte, what AGMV_EncodeFramesScaledDev writes for V as an XRGB32 source with this
                            target and filter; only AGMV_SCALE_NEAREST and AGMV_SCALE_AREA are accepted
   The palette, the schedule's decisions, the PDIFS midpoints, the header and the chunks are those of V.  frames_per_second is
   written as given (divide by step to keep the clip's speed).  The dither, the stabilisation, the palette refinement and a pending
   AGMV_SetAudioDev track apply as for the other AGMV_EncodeFrames*Dev; the track is consumed whatever the call returns.
   Returns 0, or a negative value; the checks, in this order, all before a device is opened and before a file is created:
     -1  NULL filename or frames; unknown format or enum value; with a target a filter other than NEAREST and AREA; step == 0;
         exactly one of view->width, view->height zero; x or y not zero with a zero window
     -5  AGMV_SCHEDULE_ADAPTIVE with a pending track
     -3  a source size AGMV_EncodeFramesScaledDev refuses (zero, or above 2^28 pixels); a window that does not lie inside the frame;
         an NV12 / I420 source of odd width or height, unless the view is consecutive full frames; without a target a window
         (or full frame) whose size AGMV_EncodeFramesDev refuses for this opt; with a target everything
         AGMV_EncodeFramesScaledDev refuses for a source of the window's size: a target that is zero or no multiple of 4, a GBA /
         NDS opt, AGMV_SCALE_AREA with a target above the window in either axis or with a window above 2^24 pixels
     -2  the view's length -- the frames first, first + step, ... below num_of_frames, at most count of them; 0 for a `first` at or
         behind the end -- is below what the schedule's first group reads
     -4  the clip or the staging batch cannot be allocated: after the device is opened, still before a file is created
   How it runs.  The selection that takes everything is AGMV_EncodeFramesFmtDev / AGMV_EncodeFramesScaledDev, launch for launch.
   Consecutive full frames (step == 1, no window) are the same call on d_frames + first * frame bytes: nothing is copied.  Any
   other view without a target materialises V once on the library's device, 4 * window width * window height * length bytes, with
   one launch (agmv_hip_view_source_async of include/agmv_hip_view_source.h), and takes the path of AGMV_EncodeFramesDev on it.
   With a target only D, the clip at the target's size, is materialised: V exists one staging batch at a time -- as many windows
   as fit 256 MiB, and at least one -- which agmv_hip_view_source_async writes and the box filter / the nearest gather then reads as
   an XRGB32 source into that batch's frames of D; every frame of D is a function of its own window alone, so D is what the scale
   of the whole of V gives.  256 MiB is the size of the memory-side cache and bounds the memory; it is not a tuned value.
   AGMV_VIEW_STAGE_FRAMES=n in the environment (read per call, a test aid) forces batches of n windows.  The source is read once,
   in its own layout, and nothing of its size is allocated; everything is freed before the call returns.
   AGMV_GetEncodeViewStats reports what the last AGMV_EncodeViewDev of this process did: frames = the frames encoded (the view's
   length), clip_bytes = the bytes of the XRGB32 clip it materialised (V, with a target D; 0 where the source was encoded in place),
   staging_bytes = the bytes of the staging batch (0 without one).  All zero behind a call that returned a negative value. */
typedef struct AGMV_ENCODE_VIEW_STATS { unsigned frames; unsigned long long clip_bytes, staging_bytes; } AGMV_ENCODE_VIEW_STATS;
int AGMV_EncodeViewDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height,
                       const AGMV_VIEW* view, u32 width, u32 height, AGMV_SCALE filter, u32 frames_per_second, AGMV_OPT opt,
                       AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule);
void AGMV_GetEncodeViewStats(AGMV_ENCODE_VIEW_STATS* out);

/* A view of a clip encoded at another frame rate: 60 -> 24, 30 -> 24, 25 -> 15, 50 -> 12, with an exact box filter in time, where
   the view's step can only drop frames and only at integer ratios.  Integers only; div is the quotient of non-negative integers.
   Let V be the XRGB32 clip of the view exactly as AGMV_EncodeViewDev defines it above, nv its length (view == NULL: the whole
   clip).  A rate src : dst reads "src frames of V become dst frames of the result"; both are divided by their gcd first, giving
   sn : dn, which must both be <= 65535.  The result R has m = (nv * dn) div sn frames (64-bit): the target intervals that lie
   entirely inside V.
     AGMV_TIME_AREA     needs dn <= sn.  Frame k of V occupies [k * dn, (k + 1) * dn), frame j of R occupies [j * sn, (j + 1) * sn);
                        wt(j, k) is the length of their overlap, 0 .. dn, and the wt of one j sum to sn.  Per channel and pixel
                          R[j] = (sum over k of wt(j, k) * V[k] + sn div 2) div sn
                        255 * 65535 + 32767 < 2^32, so every sum is exact in 32-bit unsigned arithmetic.  The channels are averaged
                        in RGB, after the layout's reading rule, never in YUV (as for AGMV_SCALE_AREA).
     AGMV_TIME_NEAREST  any ratio, duplication (dn > sn) included: R[j] = V[((2j + 1) * sn) div (2 * dn)], the frame under the
                        target interval's centre.
   Bits 24 .. 31 of every pixel of R are 0, under either filter.  What follows from the rule: 1 : 1 is the identity; k : 1 AREA is the
   mean of each group of k frames, rounded half up; k : 1 NEAREST is frame j * k + k div 2; under AREA a frame of V has weight in
   at most two frames of R, a pixel that does not change over the taps keeps its value, and under either filter every output lies
   between the smallest and the largest of its taps.
   AGMV_EncodeViewRateDev writes, byte for byte, the file AGMV_EncodeFramesDev writes for R when no target is given
   (width == height == 0), and with a target the file AGMV_EncodeFramesScaledDev writes for R as an XRGB32 source with that target
   and filter.  The palette, the schedule's decisions (AGMV_SCHEDULE_ADAPTIVE's skipping included), the PDIFS midpoints, the header
   and the chunks are those of R; frames_per_second is written as given; the dither, the stabilisation, the palette refinement and a
   pending AGMV_SetAudioDev track apply as for every other AGMV_EncodeFrames*Dev.  rate == NULL, or a rate that reduces to 1 : 1
   (its filter must still be known), is AGMV_EncodeViewDev, launch for launch and byte for byte.
   Returns 0, or a negative value: the refusals of AGMV_EncodeViewDev, in its order, all before a device is opened and before a
   file is created, with these additions:
     -1  also: rate->src or rate->dst zero; an unknown time filter; a reduced src or dst above 65535; AGMV_TIME_AREA with dst > src
     -3  also: for a rate other than 1 : 1 an NV12 / I420 source of odd width or height, consecutive full frames included (nothing
         is encoded in place then)
     -2  is judged on m, not on nv: an m of 0 is -2
   How it runs.  Without a target R is materialised once, 4 * window width * window height * m bytes, with one launch
   (agmv_hip_time_frames_async of include/agmv_hip_time.h), and takes the path of AGMV_EncodeFramesDev.  With a target R exists one
   staging batch at a time, of the size AGMV_EncodeViewDev gives its batches of V (AGMV_VIEW_STAGE_FRAMES still forces it): the
   same entry point writes the batch, the box filter / the nearest gather read it as an XRGB32 source, and every frame of D is a
   function of its own frame of R.  The source is read in its own layout and nothing of its size is allocated.
   AGMV_GetEncodeRateStats reports the last AGMV_EncodeViewRateDev of this process: frames_in = nv, frames_out = m, frame_reads =
   the sum over j of the taps with a weight above 0 (under AREA at most nv + m - 1), counted on the host.  All zero behind a call
   that returned a negative value.  AGMV_GetEncodeViewStats reports the same call too, with frames = m.
   The writer sessions of include/agmv_writer.h take no rate: a group of taps may straddle two pieces. */
typedef enum AGMV_TIME { AGMV_TIME_NEAREST = 1, AGMV_TIME_AREA = 2 } AGMV_TIME;
typedef struct AGMV_RATE { unsigned src, dst, filter; } AGMV_RATE;
typedef struct AGMV_ENCODE_RATE_STATS { unsigned frames_in, frames_out; unsigned long long frame_reads; } AGMV_ENCODE_RATE_STATS;
int AGMV_EncodeViewRateDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height,
                           const AGMV_VIEW* view, const AGMV_RATE* rate, u32 width, u32 height, AGMV_SCALE filter, u32 frames_per_second,
                           AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule);
void AGMV_GetEncodeRateStats(AGMV_ENCODE_RATE_STATS* out);

/* Audio tracks from and to GPU memory.  An AGMV_PCMFMT names the layout of PCM in device memory:
     AGMV_PCM_S16   [samples][channels] 16-bit words, bits unchanged (int16 WAV samples as they are); for 16-bit tracks
     AGMV_PCM_U8    [samples][channels] unsigned bytes; for 8-bit tracks; a copy
     AGMV_PCM_F32P  [channels][samples] float, 1 .. 8 channels (torchaudio's planar layout); for 16-bit tracks.  Into the track:
                    q = (int)rintf(fminf(fmaxf(x, -1), 1) * 32767.0f), rounding half to even, NaN gives 0, and the track's u16 is
                    the bit pattern of (int16)q.  Out of the track: (float)(int16)u / 32768.0f.
   AGMV_SetAudioDev attaches a track in the memory of the library's device to the NEXT AGMV_EncodeFrames*Dev call, which consumes
   it whatever that call returns; NULL clears it.  The memory must stay valid and complete until that call returns.  Returns 0,
   or a negative value and attaches nothing: -1 unknown format, -2 zero channels, more than 255, or more than 8 planar ones, -3 a sample rate
   of 0, -4 a length of less than one second (samples_per_channel / sample_rate == 0: no track), -5 more than 2^32 - 1 samples
   over all channels.  The encode call sets the header as the WAV importer would for that PCM (16 or 8 bits per sample,
   audio_size = samples_per_channel * channels, duration = samples_per_channel / sample_rate), compands the whole track in one
   kernel (agmv_hip_audio_compand_async of include/agmv_hip.h) on the library's device, downloads the codes and lets the drivers
   interleave the chunks: byte for byte the file of the BMP driver on an object that holds the same track.
   AGMV_SCHEDULE_ADAPTIVE with a pending track returns -5 before any file is created (AGMV_EncodeVideo has no audio).
   AGMV_DecodeAudioDev mirrors AGMV_DecodeFramesFmtDev: *info (may be NULL) receives the header's AGMV_INFO; with d_pcm NULL
   nothing else happens.  Otherwise the chunks' payloads are gathered as AGMV_DecodeAudio walks them, uploaded once and expanded
   by one kernel into the layout `fmt`.  Returns the samples decoded over all channels: the sum of the chunks' sizes, at most
   audio_size and at most cap_samples, rounded down to whole sample frames; 0 for a file without a track.  F32P planes hold
   (return value / channels) samples each and lie back to back from d_pcm.  A negative return is an Error, negated; -1 also for
   an unknown format, a format that does not fit the track's bits per sample, zero channels and more than 8 planar ones.  No
   video is decoded. */
typedef enum AGMV_PCMFMT { AGMV_PCM_S16 = 1, AGMV_PCM_U8 = 2, AGMV_PCM_F32P = 3 } AGMV_PCMFMT;
int AGMV_SetAudioDev(const void* d_pcm, AGMV_PCMFMT fmt, u32 samples_per_channel, u32 sample_rate, u16 channels);
int AGMV_DecodeAudioDev(const char* filename, void* d_pcm, AGMV_PCMFMT fmt, u32 cap_samples, AGMV_INFO* info);

/* Measuring a decoded clip: what a lossy knob (the quality level, the palette refinement, the dither, the stabilisation, a scale) did to the pixels,
   computed where the frames are.  Two clips of n frames of w x h pixels, w and h multiples of 4: the TEST clip is packed XRGB32
   (what the decoder produces; bits >= 24 are ignored), the REFERENCE clip is in any AGMV_PIXFMT layout, YUV flags included; a YUV
   reference is compared as the XRGB32 clip it stands for by the reading rule above.  Per frame and per channel c (0 = R, 1 = G,
   2 = B), with a the test channel and b the reference channel of a pixel:
     sse[c]        the sum over the pixels of (a - b)^2
     block_sse[c]  the sum over the 4x4 blocks of the codec's grid of (sum of a over the block - sum of b over the block)^2: 256
                   times the squared error of the block means
     max_err[c]    the largest |a - b|
     ssim[c]       the sum over the windows of the window's SSIM in Q20, signed
   A window is 2 x 2 blocks (8 x 8 pixels) at every block position (bx, by) with bx < w/4 - 1 and by < h/4 - 1: overlapping windows at
   stride 4, (w/4 - 1) * (h/4 - 1) per frame, none when w = 4 or h = 4.  Over the 64 pixels of a window
     s1 = sum a    s2 = sum b    ss = sum a^2 + sum b^2    s12 = sum a*b
     vars = 64 * ss - s1^2 - s2^2                cov = 64 * s12 - s1 * s2
     num = (2 * s1 * s2 + C1) * (2 * cov + C2)     den = (s1^2 + s2^2 + C1) * (vars + C2)
     C1 = 26634 = floor(0.01^2 * 255^2 * 64^2 + 0.5)       C2 = 235963 = floor(0.03^2 * 255^2 * 64 * 63 + 0.5)
   and the window's value is floor(num * 2^20 / den), the floor towards minus infinity.  den > 0 and |num| <= den < 2^58, so 20
   shift-and-subtract steps on 64-bit magnitudes give the quotient, and for a negative num the value is -q - (remainder != 0).
   Equal windows give exactly 2^20.  Everything is integer: the sums do not depend on the order of accumulation, and the same
   clips give the same words from run to run.  PSNR and the mean SSIM are the caller's to form: over a set of frames and channels
   PSNR = 10 * log10(255^2 * pixels * channels / sum of sse), mean SSIM = sum of ssim / 2^20 / (windows * channels).
   AGMV_MeasureFramesDev measures two clips in the memory of the library's device (agmv_hip_measure_frames_async of
   include/agmv_hip.h is the kernel) into `quality`, host memory of num_of_frames entries.  Returns 0, or a negative value before a
   device is opened: -1 NULL pointer or unknown format, -3 width or height zero, not a multiple of 4, more than 2^28 pixels, or more than 2^31 - 1 frames.
   num_of_frames == 0 is 0 and touches nothing.  A GPU failure aborts with a message, as in the encoders.
   AGMV_MeasureFileDev decodes the file and measures frame k of it against frame k of the reference clip d_ref (num_of_frames
   frames of the file's size in the layout ref_fmt), batch by batch, without ever holding the decoded clip: a batch is decoded
   into the decoder's double buffer, measured there, and its entries are downloaded once at the end.  Returns the number of
   frames measured; entries behind that number are not written.  *info (may be NULL) receives the header's AGMV_INFO; with
   `quality` NULL nothing else happens and the return is 0.  Negative returns: -1 unknown format or NULL d_ref, -3 num_of_frames
   differs from the header's count or the file's size cannot hold the layout (odd width or height for YUV), else an Error,
   negated.  File and clip correspond frame for frame when the file was written with AGMV_SCHEDULE_FULL; the other schedules
   drop frames, and the header's count says so. */
typedef struct AGMV_FRAME_QUALITY {            /* 96 bytes, the same on host and device */
	unsigned long long sse[3], block_sse[3], max_err[3];
	long long ssim[3];
} AGMV_FRAME_QUALITY;
int AGMV_MeasureFramesDev(const unsigned* d_test, const void* d_ref, AGMV_PIXFMT ref_fmt, u32 num_of_frames, u32 width, u32 height,
                          AGMV_FRAME_QUALITY* quality /* host, num_of_frames entries */);
int AGMV_MeasureFileDev(const char* filename, const void* d_ref, AGMV_PIXFMT ref_fmt, u32 num_of_frames,
                        AGMV_FRAME_QUALITY* quality /* host */, AGMV_INFO* info);

#ifdef __cplusplus
}
#endif
#endif
