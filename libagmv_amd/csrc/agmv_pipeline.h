/* libagmv_amd/csrc/agmv_pipeline.h -- the pipelined sequence engine (agmv_pipeline.c), internal to the host library */
#ifndef AGMV_PIPELINE_H
#define AGMV_PIPELINE_H

#include <stdio.h>

#include "agmv_hip.h"
#include "agmv_internal.h"

typedef struct agmv_pool agmv_pool;
agmv_pool* agmv_pool_start(unsigned threads);
void agmv_pool_submit(agmv_pool* p, void (*fn)(void*), void* arg);
void agmv_pool_stop(agmv_pool* p);                       /* runs what is queued, then joins */

void agmv_frame_path(char* out, size_t cap, const char* dir, const char* base, long idx);
uint32_t* agmv_source_index(uint32_t sw, uint32_t sh, int scale_w, int scale_h, uint32_t w, uint32_t h);
uint32_t* agmv_scale_index(uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh);
void agmv_load_source(const char* dir, const char* base, long idx, int scale_w, int scale_h, uint32_t w, uint32_t h, uint32_t* dst);

/* where the frames of a sequence encode come from: the numbered BMP files dir/base<idx>.bmp, or (d_frames != NULL) a clip of
   n_frames frames of src_w x src_h pixels in the layout `fmt` (an AGMV_PIXFMT, for NV12 / I420 with the AGMV_YUV_ flags) in the
   memory of device `device`, its first frame numbered `first` */
typedef struct agmv_source {
	const char *dir, *base;
	const void* d_frames;
	int fmt;
	uint32_t src_w, src_h, n_frames;
	long first;
	int device;
} agmv_source;

/* a YUV 4:2:0 layout (its frames are addressed by w and h, not by a pixel count), and the bytes of one frame of any layout */
#define AGMV_FMT_IS_YUV(fmt) (((fmt) & 0xFF) >= AGMV_PIXFMT_NV12)
static inline size_t agmv_fmt_frame_bytes(int fmt, uint32_t w, uint32_t h)
{
	return AGMV_FMT_IS_YUV(fmt) ? agmv_hip_yuv_frame_bytes(fmt, w, h) : agmv_hip_pixfmt_frame_bytes(fmt, (size_t)w * h);
}

/* one open sequence encode: frames are pushed in order (plain, or the PDIFS midpoint of two sources) and leave as AGFC
   (+ AGAC) chunks in `file`, strictly in order; batches of `cap` frames (whole GOPs) go round-robin over two workers per
   device; a device source is encoded by two workers on its own device, which read it in place (no load tasks, no pinned
   staging).  `pal` = palette0 | palette1.  agmv_seq_close returns the number of frames written. */
typedef struct agmv_seq agmv_seq;
agmv_seq* agmv_seq_open(AGMV* a, FILE* file, const agmv_source* src, int scale_w, int scale_h, int mode512, int lz77,
                        int audio_chunks, int use_interp, unsigned cap, unsigned devices, unsigned threads, const uint32_t pal[512]);
void agmv_seq_push(agmv_seq* s, long a, long b);
u32  agmv_seq_close(agmv_seq* s);

void agmv_histogram_frames(agmv_hip_ctx* ctx, const agmv_source* src, u32 start, u32 end, u32 size, int quality,
                           unsigned threads, uint32_t* hist);

/* a target for the decoder's sink: the frames land in d_dst at w x h, scaled with `filter` (an AGMV_SCALE of include/agmv.h).
   tensor != 0 (an AGMV_TENSORFMT): d_dst is a tensor clip of that type instead of a clip in `fmt`, written through `table` (host
   memory, the 768 elements of agmv_hip_tensor_table); filter 0 then means the file's size, and w, h are not read */
typedef struct agmv_scale { uint32_t w, h; int filter, tensor; const void* table; } agmv_scale;

int agmv_decode_stream(agmv_hip_ctx* ctx, const u8* file, size_t len, size_t pos, uint32_t w, uint32_t h, uint32_t nframes, int ver,
                       int has_audio, unsigned cap_frames, unsigned threads, void* d_dst, int fmt, const agmv_scale* scale, void* d_quality,
                       unsigned long* export_count);

/* the AGAC payloads of a file image (its first chunk at or behind pos) back to back, at most cap bytes; returns their number */
size_t agmv_gather_audio(const u8* file, size_t len, size_t pos, uint32_t nframes, u8* out, size_t cap);

/* agmv_codec.c */
void agmv_write_frame_chunk(FILE* f, u32 frame_no, u32 usize, u32 csize, const u8* payload);

#endif
