/* libagmv_amd/csrc/agmv_pipeline.h -- the pipelined sequence engine (agmv_pipeline.c), internal to the host library */
#ifndef AGMV_PIPELINE_H
#define AGMV_PIPELINE_H

#include <stdio.h>

#include "agmv_hip.h"
#include "agmv_hip_deblock.h"
#include "agmv_hip_stabilise.h"
#include "agmv_hip_view.h"
#include "agmv_hip_view_source.h"
#include "agmv_hip_time.h"
#include "agmv_internal.h"
#include "agmv_reader.h"

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
   memory of device `device`, its first frame numbered `first`.  ring_frames != 0 is the ring form of such a clip (a writer session's staging): d_frames holds
   ring_frames frames, frame idx of the clip lies at (idx - first) % ring_frames, n_frames is not read, and whoever fills the ring waits for
   agmv_seq_sources_free before it overwrites a frame */
typedef struct agmv_source {
	const char *dir, *base;
	const void* d_frames;
	int fmt;
	uint32_t src_w, src_h, n_frames;
	long first;
	int device;
	uint32_t ring_frames;
} agmv_source;
/* the table of agmv_source_index for such a clip on the device of context c, uploaded on `stream`; *h_index: the host's table, the caller's to free
   behind its next synchronisation of that stream.  NULL on failure. */
uint32_t* agmv_source_index_dev(agmv_hip_ctx* c, void* stream, const agmv_source* src, int scale_w, int scale_h, uint32_t w, uint32_t h, uint32_t** h_index);

/* The one place that knows the two families of layouts: a YUV 4:2:0 clip is addressed by w and h, a byte layout by a pixel count.
   The bytes of one frame, and the device calls that read or write a clip of w x h frames in the layout `fmt`. */
#define AGMV_FMT_IS_YUV(fmt) (((fmt) & 0xFF) >= AGMV_PIXFMT_NV12)
static inline size_t agmv_fmt_frame_bytes(int fmt, uint32_t w, uint32_t h)
{
	return AGMV_FMT_IS_YUV(fmt) ? agmv_hip_yuv_frame_bytes(fmt, w, h) : agmv_hip_pixfmt_frame_bytes(fmt, (size_t)w * h);
}
static inline int agmv_fmt_to_xrgb(agmv_hip_ctx* c, int fmt, uint32_t w, uint32_t h, const void* d_src, uint32_t n, size_t n_pixels, uint32_t* d_dst, void* stream)
{
	return AGMV_FMT_IS_YUV(fmt) ? agmv_hip_yuv_to_xrgb_dev(c, fmt, d_src, w, h, n, n_pixels, d_dst, stream)
	                            : agmv_hip_pixels_to_xrgb_dev(c, fmt, d_src, (size_t)w * h, n, n_pixels, d_dst, stream);
}
static inline int agmv_fmt_from_xrgb(agmv_hip_ctx* c, int fmt, uint32_t w, uint32_t h, const uint32_t* d_src, uint32_t n, void* d_dst, void* stream)
{
	return AGMV_FMT_IS_YUV(fmt) ? agmv_hip_yuv_from_xrgb_dev(c, fmt, d_src, w, h, n, d_dst, stream)
	                            : agmv_hip_pixels_from_xrgb_dev(c, fmt, d_src, n, (size_t)w * h, d_dst, stream);
}
static inline int agmv_fmt_gather(agmv_hip_ctx* c, int fmt, uint32_t w, uint32_t h, const void* d_src, uint32_t n, const uint32_t* d_index, size_t n_out, uint32_t* d_dst, void* stream)
{
	return AGMV_FMT_IS_YUV(fmt) ? agmv_hip_yuv_gather_dev(c, fmt, d_src, w, h, n, d_index, n_out, d_dst, stream)
	                            : agmv_hip_gather_fmt_dev(c, fmt, d_src, (size_t)w * h, n, d_index, n_out, d_dst, stream);
}
static inline int agmv_fmt_histogram(agmv_hip_ctx* c, int fmt, uint32_t w, uint32_t h, const void* d_src, uint32_t n, size_t n_pixels, int quality, uint32_t* d_hist, void* stream)
{
	return AGMV_FMT_IS_YUV(fmt) ? agmv_hip_yuv_histogram_dev(c, fmt, d_src, w, h, n, n_pixels, quality, d_hist, stream)
	                            : agmv_hip_histogram_fmt_dev(c, fmt, d_src, (size_t)w * h, n, n_pixels, quality, d_hist, stream);
}
static inline int agmv_fmt_similarity(agmv_hip_ctx* c, int fmt, uint32_t w, uint32_t h, const void* d_src, uint32_t n, uint32_t* d_counts, void* stream)
{
	return AGMV_FMT_IS_YUV(fmt) ? agmv_hip_yuv_similarity_dev(c, fmt, d_src, w, h, n, d_counts, stream)
	                            : agmv_hip_similarity_fmt_dev(c, fmt, d_src, n, (size_t)w * h, d_counts, stream);
}

/* one open sequence encode: frames are pushed in order (plain, or the PDIFS midpoint of two sources) and leave as AGFC
   (+ AGAC) chunks in `file`, strictly in order; batches of `cap` frames (whole GOPs) go round-robin over two workers per
   device; a device source is encoded by two workers on its own device, which read it in place (no load tasks, no pinned
   staging).  agmv_seq_close returns the number of frames written. */
typedef struct agmv_seq agmv_seq;
typedef struct agmv_seq_opts {
	int scale_w, scale_h;                  /* the size a GBA / NDS opt scales every source frame to, 0 x 0: the frames as they are */
	int mode512, lz77;                     /* two palettes; LZ77 instead of LZSS */
	int audio_chunks, use_interp;          /* an AGAC chunk behind every frame chunk; frames may be PDIFS midpoints */
	unsigned cap, devices, threads;        /* frames per batch (rounded up to whole GOPs), devices asked for, host pool threads */
	const uint32_t* pal;                   /* [512] palette0 | palette1 */
} agmv_seq_opts;
agmv_seq* agmv_seq_open(AGMV* a, FILE* file, const agmv_source* src, const agmv_seq_opts* opts);
void agmv_seq_push(agmv_seq* s, long a, long b);
u32  agmv_seq_close(agmv_seq* s);
/* A sequence may be opened before its palette and file exist (opts->pal NULL, file NULL: a writer session allocates everything at its open):
   agmv_seq_start hands both over before the first push.  A ring source is given back in batch order, when a batch's bitstreams are ready
   (`bits_ready`: the worker has synchronised its stream behind the batch, so nothing reads its sources any more): agmv_seq_sources_free is the number
   of sources, counted from the clip's first, that no batch reads any more; agmv_seq_wait_sources_free returns once it is at least `want`, which the
   batches submitted so far must cover.  agmv_seq_counts: the batches submitted and the frames whose chunks are in the file. */
void agmv_seq_start(agmv_seq* s, FILE* file, const uint32_t* pal, int mode512);
unsigned long agmv_seq_sources_free(agmv_seq* s);
unsigned long agmv_seq_wait_sources_free(agmv_seq* s, unsigned long want);
void agmv_seq_counts(agmv_seq* s, unsigned* batches, unsigned long long* frames_written);

/* The PDIFS schedule of a clip whose end is not known (a writer session), stated once.  encode_sequence's loop over n frames emits its first group
   whatever n is (it reads 4 sources for a light opt, 2 for a heavy one: fewer frames are refused) and a later group, starting at 0-based source
   j = 4k (light) or 2k (heavy), exactly when its `i + 4 >= end_frame` did not break before it: when frame j + 5 exists.  Returns the groups that are
   decided once n frames have arrived.  Frames that arrive later only add groups, so closing decides nothing more: the sources behind the last decided
   group are the ones the loop never encodes, and `closed` changes nothing (the test holds both values to the loop). */
uint32_t agmv_writer_groups(uint32_t n, int heavy, int closed);

void agmv_histogram_frames(agmv_hip_ctx* ctx, const agmv_source* src, u32 start, u32 end, u32 size, int quality,
                           unsigned threads, uint32_t* hist);

/* Where the decoder's frames go, frame k of the file to its place in device memory of the decoder's device; *count advances by the
   frames decoded.  EXPORT: quick_export_<*count + 1 ...>.bmp, *count being the running export counter.  FRAMES: a clip in the AGMV_PIXFMT fmt.
   TENSOR: a tensor clip of the AGMV_TENSORFMT type, written through `table` (host, the 768 elements of agmv_hip_tensor_table).  MEASURE:
   nowhere; frame k is measured against frame k of the clip d_ref in fmt, which is only read, and its AGMV_FRAME_QUALITY lands in d_quality[k].
   A target with a filter (an AGMV_SCALE) scales every frame to w x h on its way; filter 0 is the file's size, and w, h are not read. */
typedef struct agmv_target { uint32_t w, h; int filter; } agmv_target;
/* A FRAMES or TENSOR sink with `viewed` set takes a view of the file (AGMV_VIEW of include/agmv.h), resolved against the header:
   view.count >= 1 is the number of frames it delivers, view.width x view.height the window's own size.  Frame j of the view goes
   where frame j of a file goes; target, layout and normalisation apply to the window as to a file of that size; *count advances by
   the frames delivered.  Without `viewed` nothing of `view` is read and the sink is what it was before views existed. */
typedef struct agmv_sink {
	enum { AGMV_SINK_EXPORT, AGMV_SINK_FRAMES, AGMV_SINK_TENSOR, AGMV_SINK_MEASURE } kind;
	unsigned long* count;
	union {
		struct { void* d_dst; int fmt; agmv_target to; } frames;
		struct { void* d_dst; int type; const void* table; agmv_target to; } tensor;
		struct { const void* d_ref; int fmt; void* d_quality; } measure;
	};
	int viewed;
	AGMV_VIEW view;
} agmv_sink;

/* The frames of a view in a file of nframes frames: first, first + step, ... below nframes, at most `count` of them (0: no bound). */
uint32_t agmv_view_length(uint32_t first, uint32_t step, uint32_t count, uint32_t nframes);
/* The one statement of which frames of a batch belong to a view.  The frames [batch_first, batch_first + batch_n) of the file that
   are frames first + j * step of the view, j < count (count 0: no bound), are an arithmetic progression of difference `step`:
   returns its length, and for a length above 0 *row = the index in the batch of its first frame and *index = that frame's j. */
uint32_t agmv_view_in_batch(uint32_t first, uint32_t step, uint32_t count, uint32_t batch_first, uint32_t batch_n, uint32_t* row, uint32_t* index);

/* the target of a sink that scales, else NULL */
static inline const agmv_target* agmv_sink_target(const agmv_sink* s)
{
	const agmv_target* t = s->kind == AGMV_SINK_FRAMES ? &s->frames.to : s->kind == AGMV_SINK_TENSOR ? &s->tensor.to : NULL;
	return t && t->filter ? t : NULL;
}

int agmv_decode_stream(agmv_hip_ctx* ctx, const u8* file, size_t len, size_t pos, uint32_t w, uint32_t h, uint32_t nframes, int ver,
                       int has_audio, unsigned cap_frames, unsigned threads, const agmv_sink* sink, AGMV_VIEW_STATS* stats);

/* A file image as the decode drivers read it: len bytes with 16 zero bytes behind them, pos = the first byte behind the header, w x h frames,
   nframes of them at most, the header's version, whether an AGAC chunk follows every frame chunk. */
typedef struct agmv_dfile { const u8* image; size_t len, pos; uint32_t w, h, nframes; int ver, has_audio; } agmv_dfile;

/* A reader session (include/agmv_reader.h has the contract): what agmv_decode_stream opens, kept open.  The image must outlive the reader.  `sink` is a
   FRAMES or TENSOR sink with `viewed` set and the view resolved against the header (step, window; first and count are each read's own), its destination
   and count are not read; deblock is the strength, 0 = off; index_bytes the budget of the seek index.  agmv_dreader_read returns the frames delivered
   or a negative Error. */
typedef struct agmv_dreader agmv_dreader;
agmv_dreader* agmv_dreader_open(agmv_hip_ctx* ctx, const agmv_dfile* f, unsigned cap_frames, unsigned threads, const agmv_sink* sink, unsigned deblock, size_t index_bytes);
int agmv_dreader_read(agmv_dreader* r, void* d_dst, uint32_t n);
void agmv_dreader_seek(agmv_dreader* r, uint32_t frame);
uint32_t agmv_dreader_tell(const agmv_dreader* r);
void agmv_dreader_stats(const agmv_dreader* r, AGMV_READER_STATS* out);
void agmv_dreader_close(agmv_dreader* r);

/* The arithmetic of a reader's seek index, stated once.  *interval (may be NULL) = the distance of its checkpoints in a file of nframes frames whose
   persistent buffer has lz_cap bytes, under a budget of index_bytes: the smallest multiple of 4, at least 4, with ceil(nframes / interval) * lz_cap <=
   index_bytes -- and for a budget below one lz_cap the smallest multiple of 4 that is >= nframes: checkpoint 0 alone, the zero buffer, which costs
   nothing.  Returns the frame the LZ stage starts at for a seek to frame f: the greatest recorded checkpoint <= f & ~3, where bit k of `recorded`
   (32 per word; NULL: none) says that checkpoint k * interval is recorded; checkpoint 0 always is. */
uint32_t agmv_reader_checkpoint(uint32_t nframes, size_t lz_cap, size_t index_bytes, uint32_t f, const uint32_t* recorded, uint32_t* interval);

/* the AGAC payloads of a file image (its first chunk at or behind pos) back to back, at most cap bytes; returns their number */
size_t agmv_gather_audio(const u8* file, size_t len, size_t pos, uint32_t nframes, u8* out, size_t cap);

/* agmv_codec.c */
void agmv_write_frame_chunk(FILE* f, u32 frame_no, u32 usize, u32 csize, const u8* payload);

#endif
