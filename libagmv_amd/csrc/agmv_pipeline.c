/*
 * libagmv_amd/csrc/agmv_pipeline.c -- the pipelined sequence engine behind AGMV_EncodeAGMV / AGMV_EncodeFullAGMV /
 * AGMV_EncodeVideo and AGMV_DecodeAGMV / AGMV_DecodeVideo (reference src/agmv_encode.c:719-4407 BMP branch,
 * src/agmv_decode.c:455-647).  The reference runs load -> encode -> compress -> write one frame after the other on one
 * thread; here the stages of DIFFERENT batches overlap (SURVEY.md section 7 "pipeline shape"):
 *
 *   encode   host cores: BMP parse (+ GBA/NDS nearest scale) of batch b+1 into pinned staging
 *            GPU worker threads (two per device, devices = AGMV_DEVICES): H2D -> PDIFS midpoint -> (opt-in, AGMV_SetStabilise /
 *              AGMV_STABILISE: k_stabilise, in place) -> (opt-in, AGMV_SetDither /
 *              AGMV_DITHER: k_dither, in place) -> k_encode -> D2H of batch b, each worker on its own stream and context; batches are whole GOPs, so they are independent given
 *              the palette and go round-robin over the workers / devices (multi-GPU sharding by GOP range, no exchange)
 *            host cores: exact LZSS / LZ77 of batch b-1, one task per frame -- or, opt-in (AGMV_LZ_DEVICE for LZSS,
 *              AGMV_LZ77_DEVICE for LZ77 on one device), the same stage on the GPU worker's stream behind k_encode: the
 *              payloads are downloaded instead of the bitstreams
 *            calling thread: chunks written strictly in frame order
 *   decode   calling thread: chunks located, LZ stage on the host cores into pinned batch slabs, with ONE persistent buffer
 *            for the stale-tail semantics -- or, opt-in (AGMV_LZ_DECODE_DEVICE), on the GPU into device rows, the buffer
 *            on the device; GPU worker: (H2D ->) parse -> reconstruct -> (opt-in, AGMV_SetDeblock / AGMV_DEBLOCK: k_deblock,
 *            into a copy) -> D2H with the decoder state (last frame, I-frame snapshot) kept on the device, unfiltered;
 *            host cores: BMP export, one task per frame
 *
 * Both pipelines have a second end for frames that live in GPU memory (AGMV_EncodeFramesDev / AGMV_DecodeFramesDev): a device
 * SOURCE of the encoder (agmv_source: no BMP parse, no pinned staging, no upload -- the workers copy, gather or interpolate
 * from the caller's clip) and a device SINK of the decoder (the worker decodes into the caller's buffer: no D2H, no BMP export).
 * Both ends carry a pixel format (AGMV_PIXFMT): the kernels that touch the caller's clip read or write it in that layout, and
 * only the worker's batch buffers hold packed 0x00RRGGBB pixels.  Everything between the two ends is the same code.
 *
 * Plain C + pthreads; everything that touches the GPU goes through include/agmv_hip.h.  No CPU fallback: a GPU failure in
 * the void encoders aborts with a message, in the int-returning decoders it is returned.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "agmv_hip.h"
#include "agmv_internal.h"
#include "agmv_pipeline.h"

#include <time.h>
static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
/* host allocations of the drivers: the void encoders have no error channel (reference src/agmv_encode.c:529), so a failed
   allocation ends the process with a message instead of a NULL dereference in some pool thread */
static void* xmalloc(size_t n) { void* p = malloc(n ? n : 1); if (!p) agmv_die("out of host memory"); return p; }
static void* xcalloc(size_t n, size_t m) { void* p = calloc(n ? n : 1, m ? m : 1); if (!p) agmv_die("out of host memory"); return p; }
/* ... and their pinned and device allocations likewise */
static void* pinned(size_t n) { void* p = agmv_hip_host_alloc(n); if (!p) agmv_die("pinned allocation"); return p; }
static void* on_device(agmv_hip_ctx* c, size_t n) { void* p = agmv_hip_malloc_on(c, n); if (!p) agmv_die("device allocation"); return p; }
static void* zeroed_on_device(agmv_hip_ctx* c, size_t n, void* stream)       /* (complete on return) */
{
	void* p = on_device(c, n);
	if (agmv_hip_memset_async(c, p, 0, n, stream) || agmv_hip_stream_sync(c, stream)) agmv_die("device allocation");
	return p;
}

static int tracing(void) { static int v = -1; if (v < 0) v = getenv("AGMV_TRACE") != NULL; return v; }
#define TRACE(...) do { if (tracing()) fprintf(stderr, "agmv trace: " __VA_ARGS__); } while (0)
/* the opt-in knobs of the encoder are on for any non-zero integer */
static int env_nonzero(const char* name) { const char* v = getenv(name); return v && atoi(v) != 0; }

/* ------------------------------------------------------------------------------------------
 * a small task pool
 * ------------------------------------------------------------------------------------------ */
typedef struct task { void (*fn)(void*); void* arg; struct task* next; } task;

struct agmv_pool {
	pthread_t th[64];
	unsigned nth;
	task *head, *tail;
	pthread_mutex_t mu;
	pthread_cond_t cv;
	int stop;
};

static void* pool_main(void* arg)
{
	agmv_pool* p = (agmv_pool*)arg;
	for (;;) {
		task* t;
		pthread_mutex_lock(&p->mu);
		while (!p->head && !p->stop) pthread_cond_wait(&p->cv, &p->mu);
		t = p->head;
		if (t) { p->head = t->next; if (!p->head) p->tail = NULL; }
		pthread_mutex_unlock(&p->mu);
		if (!t) break;                                    /* stop and drained */
		t->fn(t->arg);
		free(t);
	}
	return NULL;
}

agmv_pool* agmv_pool_start(unsigned threads)
{
	agmv_pool* p = (agmv_pool*)xcalloc(1, sizeof(*p));
	unsigned i;
	if (threads < 1) threads = 1;
	if (threads > 64) threads = 64;
	pthread_mutex_init(&p->mu, NULL);
	pthread_cond_init(&p->cv, NULL);
	p->nth = 0;
	for (i = 0; i < threads; i++) {                            /* only threads that exist are joined later */
		if (pthread_create(&p->th[p->nth], NULL, pool_main, p) == 0) p->nth++;
	}
	if (p->nth == 0) agmv_die("cannot start a host worker thread");
	return p;
}

void agmv_pool_submit(agmv_pool* p, void (*fn)(void*), void* arg)
{
	task* t = (task*)xmalloc(sizeof(*t));
	t->fn = fn; t->arg = arg; t->next = NULL;
	pthread_mutex_lock(&p->mu);
	if (p->tail) p->tail->next = t; else p->head = t;
	p->tail = t;
	pthread_cond_signal(&p->cv);
	pthread_mutex_unlock(&p->mu);
}

void agmv_pool_stop(agmv_pool* p)
{
	unsigned i;
	if (!p) return;
	pthread_mutex_lock(&p->mu);
	p->stop = 1;
	pthread_cond_broadcast(&p->cv);
	pthread_mutex_unlock(&p->mu);
	for (i = 0; i < p->nth; i++) pthread_join(p->th[i], NULL);
	pthread_mutex_destroy(&p->mu);
	pthread_cond_destroy(&p->cv);
	free(p);
}

/* ------------------------------------------------------------------------------------------
 * source frames
 * ------------------------------------------------------------------------------------------ */
static void die_unreadable(const char* path) { fprintf(stderr, "libagmv(amd): cannot read frame %s\n", path); abort(); }

void agmv_frame_path(char* out, size_t cap, const char* dir, const char* base, long idx)
{
	if (dir[0] != 'c' || dir[1] != 'u' || dir[2] != 'r') snprintf(out, cap, "%s/%s%ld.bmp", dir, base, idx);
	else snprintf(out, cap, "%s%ld.bmp", base, idx);                /* "cur..." = current directory, src/agmv_encode.c:2373-2378 */
}

/* the GBA/NDS path from a source frame of sw x sh pixels to the w x h frame the encoder sees, as a table of w*h source
   positions (AGMV_NO_SOURCE: the pixel is 0): the nearest scale to scale_w x scale_h as the reference asks for it, then the
   first w*h pixels of the scaled image read linearly (the reference reads a 121x81 scaled image as 120x80) and
   zeros behind a scaled image that is shorter.  Every quirk of the scaled source lives here: the BMP source applies the table
   on the host, the device source hands it to agmv_hip_gather_dev. */
uint32_t* agmv_source_index(uint32_t sw, uint32_t sh, int scale_w, int scale_h, uint32_t w, uint32_t h)
{
	uint32_t nw, nh;
	uint32_t* sc = agmv_scale_nearest_index(sw, sh, ((float)scale_w / sw) + 0.001f, ((float)scale_h / sh) + 0.001f, &nw, &nh);
	const size_t need = (size_t)w * h, have = (size_t)nw * nh;
	uint32_t* idx = (uint32_t*)xmalloc(need * sizeof(uint32_t));
	size_t k;
	if (!sc) agmv_die("out of host memory");
	for (k = 0; k < need; k++) idx[k] = k < have ? sc[k] : AGMV_NO_SOURCE;
	free(sc);
	return idx;
}

/* that table for the clip of a device source, on the device of context c: allocated there and uploaded on `stream`.  *h_index is the host's table, which
   the copy reads: the caller frees it behind its next synchronisation of the stream.  NULL without device memory or when the copy is refused. */
uint32_t* agmv_source_index_dev(agmv_hip_ctx* c, void* stream, const agmv_source* src, int scale_w, int scale_h, uint32_t w, uint32_t h, uint32_t** h_index)
{
	const size_t bytes = (size_t)w * h * sizeof(uint32_t);
	uint32_t* d_index = (uint32_t*)agmv_hip_malloc_on(c, bytes);
	*h_index = agmv_source_index(src->src_w, src->src_h, scale_w, scale_h, w, h);
	if (d_index && agmv_hip_memcpy_async(c, d_index, *h_index, bytes, 0, stream)) { agmv_hip_free_on(c, d_index); d_index = NULL; }
	return d_index;
}

/* AGMV_SCALE_NEAREST of include/agmv.h as such a table: target pixel (X, Y) of the dw x dh frame reads the source pixel under
   its centre, (((2X + 1) * sw) / (2 * dw), ((2Y + 1) * sh) / (2 * dh)) in integers.  NULL without memory. */
uint32_t* agmv_scale_index(uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh)
{
	uint32_t* idx = (uint32_t*)malloc((size_t)dw * dh * sizeof(uint32_t));
	uint32_t* col = (uint32_t*)malloc((size_t)dw * sizeof(uint32_t));
	uint32_t x, y;
	if (!idx || !col) { free(idx); free(col); return NULL; }
	for (x = 0; x < dw; x++) col[x] = (uint32_t)(((2ull * x + 1) * sw) / (2ull * dw));
	for (y = 0; y < dh; y++) {
		const uint32_t row = (uint32_t)(((2ull * y + 1) * sh) / (2ull * dh)) * sw;
		for (x = 0; x < dw; x++) idx[(size_t)y * dw + x] = row + col[x];
	}
	free(col);
	return idx;
}

/* source frame `idx` as the encoder sees it: BMP -> 0x00RRGGBB, optional GBA/NDS nearest scale (agmv_source_index) */
void agmv_load_source(const char* dir, const char* base, long idx, int scale_w, int scale_h, uint32_t w, uint32_t h, uint32_t* dst)
{
	char path[4096];
	uint32_t *pix = NULL, *index, sw = 0, sh = 0;
	size_t need = (size_t)w * h, have, k;
	agmv_frame_path(path, sizeof(path), dir, base, idx);
	if (!scale_w) {                                        /* straight into the caller's (pinned) buffer */
		if (agmv_bmp_load_into(path, dst, need, &sw, &sh) != NO_ERR) die_unreadable(path);
		have = (size_t)sw * sh;
		if (have < need) memset(dst + have, 0, (need - have) * 4);
		return;
	}
	if (agmv_bmp_load(path, &pix, &sw, &sh) != NO_ERR) die_unreadable(path);
	index = agmv_source_index(sw, sh, scale_w, scale_h, w, h);
	for (k = 0; k < need; k++) dst[k] = index[k] == AGMV_NO_SOURCE ? 0 : pix[index[k]];
	free(index);
	free(pix);
}

/* ------------------------------------------------------------------------------------------
 * encode pipeline
 * ------------------------------------------------------------------------------------------ */
typedef struct lzjob { const u8* in; uint32_t n; u8* out; u32 csize; } lzjob;

typedef struct ebatch {
	unsigned id, n; u32 first_fc;
	unsigned long src_end;                 /* the sources of this batch lie before source src_end of the clip, counted from its first (submit_batch) */
	long *srcA, *srcB;                     /* source frame numbers; srcB < 0: plain frame, else PDIFS midpoint of A and B */
	uint32_t* h_pix;                       /* BMP source, pinned: frame k at [k * per], its second source at [k * per + npx] */
	unsigned loads_left, lz_left; int loaded, bits_ready;
	uint32_t *sizes, *csizes;              /* pinned [cap]: the usize of each frame and, lz_dev, its csize */
	u8* h_bits; size_t h_bits_cap, *boff;  /* pinned, rows packed back to back by download_rows, row k at boff[k] */
	lzjob* jobs; u8* comp; size_t comp_cap;
} ebatch;

typedef struct eworker {
	struct agmv_seq* s; unsigned idx; pthread_t th;
	agmv_hip_ctx* ctx; void* stream;
	uint32_t *d_frames, *d_sizes, *d_tmp[2]; uint8_t* d_out; uint16_t* d_ient;
	uint8_t* d_lz; uint32_t* d_csize;      /* lz_dev: payload rows [cap][LZSS: lz_stride, LZ77: lz77_stride] and their csize */
	size_t lz77_stride; uint8_t* d_peek;   /* lz_dev, LZ77: stride of the rows d_lz holds now (grown on demand); [cap] the byte behind each stream */
	unsigned long long* d_replaced;        /* stabilise: this worker's count of replaced blocks on its device, downloaded by eworker_close */
	unsigned long long examined;           /* stabilise: P-frame blocks of this worker's batches that had their anchor in the batch */
} eworker;

typedef struct eplan { int device_src, scaled, packs, direct, midpoints, lz_dev, lz77; unsigned devices; } eplan;

struct agmv_seq {
	AGMV* a; FILE* file; agmv_source src;
	eplan plan;                            /* what the engine branches on (eplan_of) */
	int scale_w, scale_h, audio_chunks;
	unsigned stabilise, dither;            /* strengths, 0 = off, of the temporal stabilisation of every batch (AGMV_SetStabilise / AGMV_STABILISE) and, behind it, of
	                                          its pattern dithering (AGMV_SetDither / AGMV_DITHER), both before its encode */
	uint32_t* d_index;                     /* plan.scaled: the table of agmv_source_index on the device; this and d_persist are shared by the workers (eshared_open) */
	uint8_t* d_persist;                    /* lz_dev, LZ77: `persist` on the device (persist_len bytes, zero-initialised) */
	unsigned peek_turn;                    /* lz_dev, LZ77: the batch whose peek call comes next (under mu) */
	uint32_t w, h; size_t npx, per, stride, lz_stride;
	unsigned cap, nslots, nworkers; ebatch* slot; eworker* wk; agmv_pool* pool;
	pthread_mutex_t mu; pthread_cond_t cv;
	unsigned nsubmitted, next_prep, next_write; int closing;
	unsigned next_free; unsigned long src_free;           /* a ring source: the batches before next_free have handed over, in order, and read nothing before source src_free any more */
	ebatch* cur;                           /* batch being described by agmv_seq_push */
	u32 fc0, frames_written;
	u8* persist; size_t persist_len;       /* emulation of agmv->bitstream->data for LZ77's one-past-the-end read */
	double t_open, t_load, t_lz, t_gpu, t_write;          /* AGMV_TRACE: summed task times */
};

/* The plan of a sequence encode: what open, the worker, submit, push and close branch on, derived here alone (the environment is read here, once per open).
   device_src: the frames are resident in device memory: no pinned h_pix, no load tasks, and one device, the clip's own.
   devices: the devices the batches go round, as asked for (at most the cards there are, or oversubscribed); 1 for a device source.
   scaled: a device source under a GBA / NDS opt: its frames are gathered through d_index, which exists for them alone (a BMP source is scaled on the host).
   direct: a device source of XRGB32 frames without a scale: a midpoint interpolates straight from the clip.
   packs: every other source: a midpoint's two sources are put into the worker's two temporaries as packed pixels first.
   midpoints: the sequence was opened with interpolation: frames may be PDIFS midpoints, h_pix has room for two sources per frame and the temporaries exist.
   lz77: the file's compression is LZ77, not LZSS.  lz_dev: the LZ stage runs on the GPU workers, in the form lz77 chooses (d_csize; LZSS: d_lz up front; LZ77: d_peek,
   d_persist and the turn-taking), opt-in: AGMV_LZ_DEVICE for LZSS sequences only, AGMV_LZ77_DEVICE for LZ77 ones on ONE device, where their persistent buffer then lives. */
static eplan eplan_of(const agmv_source* src, int scale_w, int use_interp, int lz77, unsigned devices)
{
	eplan p = {.device_src = src->d_frames != NULL, .midpoints = use_interp, .lz77 = lz77};
	p.devices = p.device_src ? 1 : devices;
	p.scaled = p.device_src && scale_w;
	p.direct = p.device_src && !p.scaled && src->fmt == AGMV_PIXFMT_XRGB32;
	p.packs = !p.direct;
	p.lz_dev = lz77 ? p.devices == 1 && env_nonzero("AGMV_LZ77_DEVICE") : env_nonzero("AGMV_LZ_DEVICE");
	return p;
}

typedef struct loadarg { agmv_seq* s; ebatch* b; unsigned k; int which; } loadarg;
typedef struct lzarg { agmv_seq* s; ebatch* b; unsigned k; } lzarg;

static void load_task(void* p)
{
	loadarg* la = (loadarg*)p;
	agmv_seq* s = la->s;
	ebatch* b = la->b;
	const double t0 = now_s();
	agmv_load_source(s->src.dir, s->src.base, la->which ? b->srcB[la->k] : b->srcA[la->k], s->scale_w, s->scale_h, s->w, s->h,
	                 b->h_pix + (size_t)la->k * s->per + (la->which ? s->npx : 0));
	pthread_mutex_lock(&s->mu);
	s->t_load += now_s() - t0;
	if (--b->loads_left == 0) { b->loaded = 1; pthread_cond_broadcast(&s->cv); }
	pthread_mutex_unlock(&s->mu);
	free(la);
}

static void lz_task(void* p)
{
	lzarg* za = (lzarg*)p;
	agmv_seq* s = za->s;
	lzjob* j = &za->b->jobs[za->k];
	const double t0 = now_s();
	j->csize = s->plan.lz77 ? agmv_lz77_mem(j->in, j->n, j->out) : agmv_lzss_mem(j->in, j->n, j->out);
	pthread_mutex_lock(&s->mu);
	s->t_lz += now_s() - t0;
	if (--za->b->lz_left == 0) pthread_cond_broadcast(&s->cv);
	pthread_mutex_unlock(&s->mu);
	free(za);
}

/* lz_dev, LZ77: payload rows for batch b, whose sizes are on the host: 4 bytes per byte of the largest stream (the
   worst case, 4 * stride, is 17.5 MB per 1080p frame), grown on demand.  Returns the stride of the rows. */
static size_t lz77_rows(eworker* wk, const ebatch* b)
{
	agmv_seq* s = wk->s;
	size_t top = 0, need;
	unsigned k;
	for (k = 0; k < b->n; k++) if (b->sizes[k] > top) top = b->sizes[k];
	need = (agmv_hip_lz77_max_csize(top) + 256) & ~(size_t)255;
	if (need > wk->lz77_stride) {
		agmv_hip_free_on(wk->ctx, wk->d_lz);
		wk->lz77_stride = (need + need / 4 + 255) & ~(size_t)255;
		wk->d_lz = (uint8_t*)agmv_hip_malloc_on(wk->ctx, wk->lz77_stride * s->cap);
		if (!wk->d_lz) agmv_die("device allocation");
	}
	return wk->lz77_stride;
}

/* the LZ stage of batch b on the worker's stream, for a sequence with lz_dev: the payload rows into wk->d_lz, their csize
   into b->csizes (complete on return).  The one place that knows the two device forms.  Returns the stride of the rows. */
static size_t lz_stage_dev(eworker* wk, ebatch* b)
{
	agmv_seq* s = wk->s;
	const size_t lz_stride = s->plan.lz77 ? lz77_rows(wk, b) : s->lz_stride;
	int rc;
	if (s->plan.lz77) {
		/* the persistent buffer is shared by the two workers and has to see the batches in order: the peek calls take
		   turns, and the turn is passed on once this one's writes are complete on the device */
		pthread_mutex_lock(&s->mu);
		while (s->peek_turn != b->id) pthread_cond_wait(&s->cv, &s->mu);
		pthread_mutex_unlock(&s->mu);
		if (agmv_hip_lz77_peek_dev(wk->ctx, wk->d_out, s->stride, wk->d_sizes, b->n, s->d_persist, s->persist_len, wk->d_peek, wk->stream) ||
		    agmv_hip_stream_sync(wk->ctx, wk->stream))
			agmv_die("batch LZ77 peek");
		pthread_mutex_lock(&s->mu);
		s->peek_turn = b->id + 1;
		pthread_cond_broadcast(&s->cv);
		pthread_mutex_unlock(&s->mu);
		rc = agmv_hip_lz77_frames_dev(wk->ctx, wk->d_out, s->stride, wk->d_sizes, b->n, wk->d_peek, wk->d_lz, lz_stride, wk->d_csize, wk->stream);
	} else
		rc = agmv_hip_lzss_frames_dev(wk->ctx, wk->d_out, s->stride, wk->d_sizes, b->n, wk->d_lz, lz_stride, wk->d_csize, wk->stream);
	if (rc || agmv_hip_memcpy_async(wk->ctx, b->csizes, wk->d_csize, 4 * (size_t)b->n, 1, wk->stream) || agmv_hip_stream_sync(wk->ctx, wk->stream))
		agmv_die(s->plan.lz77 ? "batch LZ77" : "batch LZSS");
	return lz_stride;
}

/* batch b's rows to the host, packed back to back in b->h_bits: row k is len[k] bytes at d_rows + k * row_stride and lands at
   b->boff[k], with `pad` more bytes reserved behind it (1 for raw bitstreams headed for the host LZ stage, 0 for payloads).
   Complete on return. */
static void download_rows(eworker* wk, ebatch* b, const uint8_t* d_rows, size_t row_stride, const uint32_t* len, size_t pad)
{
	size_t total = 0;
	unsigned k;
	for (k = 0; k < b->n; k++) { b->boff[k] = total; total += (size_t)len[k] + pad; }
	if (total + 16 > b->h_bits_cap) {
		agmv_hip_host_free(b->h_bits);
		b->h_bits_cap = total + total / 4 + 4096;
		b->h_bits = (u8*)agmv_hip_host_alloc(b->h_bits_cap);
		if (!b->h_bits) agmv_die("pinned allocation");
	}
	for (k = 0; k < b->n; k++)
		if (len[k] && agmv_hip_memcpy_async(wk->ctx, b->h_bits + b->boff[k], d_rows + (size_t)k * row_stride, len[k], 1, wk->stream))
			agmv_die("row download");
	if (agmv_hip_stream_sync(wk->ctx, wk->stream)) agmv_die("row download");
}

/* a device source: where its frame `idx` is -- in a flat clip at its index, in a ring of ring_frames frames at its index modulo the ring's length.
   The one place that knows the two forms. */
static const void* src_frame(const agmv_seq* s, long idx)
{
	size_t k = (size_t)(idx - s->src.first);
	if (s->src.ring_frames) k %= s->src.ring_frames;
	return (const u8*)s->src.d_frames + k * agmv_fmt_frame_bytes(s->src.fmt, s->src.src_w, s->src.src_h);
}

/* The one put: the source of batch b's slot k (which = 1: its second source) into dst as packed XRGB32, as the encoder sees it, on the worker's stream.
   A BMP source: the upload of what the load task left in h_pix.  A device source: converted from the clip's layout (XRGB32: a copy), or gathered through the scale's table. */
static int put_frame(eworker* wk, const ebatch* b, unsigned k, int which, uint32_t* dst)
{
	agmv_seq* s = wk->s;
	const void* at;
	if (!s->plan.device_src) return agmv_hip_memcpy_async(wk->ctx, dst, b->h_pix + (size_t)k * s->per + (which ? s->npx : 0), s->npx * 4, 0, wk->stream);
	at = src_frame(s, which ? b->srcB[k] : b->srcA[k]);
	if (s->plan.scaled) return agmv_fmt_gather(wk->ctx, s->src.fmt, s->src.src_w, s->src.src_h, at, 1, s->d_index, s->npx, dst, wk->stream);
	return agmv_fmt_to_xrgb(wk->ctx, s->src.fmt, s->src.src_w, s->src.src_h, at, 1, s->npx, dst, wk->stream);
}

/* the P-frames of a batch of n frames from frame count first_fc on whose I-frame (frame_count % 4 == 0) lies in the batch */
static unsigned stabilise_examined_frames(unsigned n, u32 first_fc)
{
	const unsigned lead = (4u - (unsigned)(first_fc & 3u)) & 3u;
	return n > lead ? (n - lead) - (n - lead + 3u) / 4u : 0;
}

/* the last sequence encode's AGMV_STABILISE_STATS: zeroed by agmv_seq_open, set by agmv_seq_close */
static AGMV_STABILISE_STATS g_stabilise_stats;
void AGMV_GetStabiliseStats(AGMV_STABILISE_STATS* out) { if (out) *out = g_stabilise_stats; }

/* The worker, by step.  Take: batch id once it is submitted and loaded; NULL when the sequence closes with none left. */
static ebatch* eworker_take(agmv_seq* s, unsigned id)
{
	ebatch* b = &s->slot[id % s->nslots];
	pthread_mutex_lock(&s->mu);
	while (!(id < s->nsubmitted && b->id == id && b->loaded) && !(s->closing && id >= s->nsubmitted)) pthread_cond_wait(&s->cv, &s->mu);
	if (id >= s->nsubmitted) b = NULL;
	pthread_mutex_unlock(&s->mu);
	return b;
}

/* Fill: the batch's frames into d_frames.  A plain frame is put; a midpoint (AGMV_InterpFrame on the GPU, src/agmv_utils.c:949-969) interpolates
   straight from the clip where the plan says `direct`, else from its two sources put into the temporaries. */
static void eworker_fill(eworker* wk, const ebatch* b)
{
	agmv_seq* s = wk->s;
	const int dev = s->plan.device_src;
	unsigned k;
	for (k = 0; k < b->n; k++) {
		uint32_t* dst = wk->d_frames + (size_t)k * s->npx;
		if (b->srcB[k] < 0) {
			if (put_frame(wk, b, k, 0, dst)) agmv_die(dev ? "frame copy" : "frame upload");
		} else if (s->plan.direct) {
			if (agmv_hip_interp_dev(wk->ctx, dst, (const uint32_t*)src_frame(s, b->srcA[k]), (const uint32_t*)src_frame(s, b->srcB[k]), s->npx, wk->stream))
				agmv_die("frame interp");
		} else if (put_frame(wk, b, k, 0, wk->d_tmp[0]) || put_frame(wk, b, k, 1, wk->d_tmp[1]) ||
		           agmv_hip_interp_dev(wk->ctx, dst, wk->d_tmp[0], wk->d_tmp[1], s->npx, wk->stream))
			agmv_die(dev ? "frame gather / interp" : "frame upload / interp");
	}
}

/* The caller's entry plane, for a first batch that completes a GOP the caller began (first_fc & 3): its I-frame entries to d_ient, behind the fill */
static void eworker_entry_plane(eworker* wk)
{
	agmv_seq* s = wk->s;
	uint16_t* e = (uint16_t*)xmalloc(s->npx * 2); size_t i;
	for (i = 0; i < s->npx; i++) e[i] = (uint16_t)((s->a->iframe_entries[i].pal_num & 1u) << 8 | s->a->iframe_entries[i].index);
	if (agmv_hip_stream_sync(wk->ctx, wk->stream) || agmv_hip_memcpy_async(wk->ctx, wk->d_ient, e, s->npx * 2, 0, wk->stream) ||
	    agmv_hip_stream_sync(wk->ctx, wk->stream))
		agmv_die("entry plane upload");
	free(e);
}

/* Encode: the frames are what k_encode would have seen, midpoints included: stabilised against the batch's own I-frames, then dithered, in place,
   on the same stream; then the bitstreams into d_out and their sizes to the host, complete on return */
static void eworker_encode(eworker* wk, ebatch* b)
{
	agmv_seq* s = wk->s;
	if (s->stabilise) {
		if (agmv_hip_stabilise_frames_async(wk->ctx, s->stabilise, wk->d_frames, s->w, s->h, b->n, b->first_fc, wk->d_replaced, wk->stream))
			agmv_die("batch stabilisation");
		wk->examined += (unsigned long long)stabilise_examined_frames(b->n, b->first_fc) * (s->npx / 16);
	}
	if (s->dither && agmv_hip_dither_frames_async(wk->ctx, s->dither, wk->d_frames, s->w, s->h, b->n, wk->stream)) agmv_die("batch dither");
	if (agmv_hip_encode_frames_dev(wk->ctx, wk->d_frames, b->n, s->w, s->h, b->first_fc, wk->d_out, s->stride, wk->d_sizes, wk->d_ient, wk->stream) ||
	    agmv_hip_memcpy_async(wk->ctx, b->sizes, wk->d_sizes, 4 * (size_t)b->n, 1, wk->stream) || agmv_hip_check(wk->ctx, wk->stream))
		agmv_die("batch encode");
}

/* Hand over: the rows to the host and the batch to the calling thread.  With the LZ stage on the GPU the payloads travel instead of the bitstreams and the time
   from here on is the trace's LZ slot; else the bitstreams, +1 byte each: prepare_batch sets the byte behind each stream.  t_taken: when the worker took the batch. */
static void eworker_hand_over(eworker* wk, ebatch* b, double t_taken)
{
	agmv_seq* s = wk->s;
	const double t_lz = now_s(); unsigned k;
	if (s->plan.lz_dev) {
		const size_t lz_stride = lz_stage_dev(wk, b);
		download_rows(wk, b, wk->d_lz, lz_stride, b->csizes, 0);
		for (k = 0; k < b->n; k++) { b->jobs[k].out = b->h_bits + b->boff[k]; b->jobs[k].csize = b->csizes[k]; }
	} else download_rows(wk, b, wk->d_out, s->stride, b->sizes, 1);
	pthread_mutex_lock(&s->mu);
	s->t_gpu += now_s() - t_taken;
	if (s->plan.lz_dev) s->t_lz += now_s() - t_lz;
	b->bits_ready = 1;
	/* the stream is synchronised: nothing reads this batch's sources any more.  Batches hand over in any order, a ring is given back in theirs */
	while (s->next_free < s->nsubmitted && s->slot[s->next_free % s->nslots].id == s->next_free && s->slot[s->next_free % s->nslots].bits_ready)
		s->src_free = s->slot[s->next_free++ % s->nslots].src_end;
	pthread_cond_broadcast(&s->cv);
	pthread_mutex_unlock(&s->mu);
}

/* one GPU worker: its batches are id = idx, idx + nworkers, ... in order */
static void* eworker_main(void* p)
{
	eworker* wk = (eworker*)p;
	unsigned id; ebatch* b;
	for (id = wk->idx; (b = eworker_take(wk->s, id)) != NULL; id += wk->s->nworkers) {
		const double t_taken = now_s();
		eworker_fill(wk, b);
		if (b->first_fc & 3u) eworker_entry_plane(wk);
		eworker_encode(wk, b);
		eworker_hand_over(wk, b, t_taken);
	}
	return NULL;
}

/* LZ stage of batch b: in frame order the byte behind each stream is set to what the reference's persistent buffer holds
   there (an earlier, longer frame's byte; LZ77 reads it, src/agmv_encode.c:222), then one task per frame */
static void prepare_batch(agmv_seq* s, ebatch* b)
{
	size_t need = 0, coff = 0;
	unsigned k;
	if (s->plan.lz_dev) return;     /* the GPU worker left the payloads (LZ77 with the byte past the end from d_persist); lz_left is 0 since begin_batch */
	for (k = 0; k < b->n; k++) need += (size_t)b->sizes[k] * (s->plan.lz77 ? 4 : 2) + 64;
	if (need > b->comp_cap) { free(b->comp); b->comp_cap = need + need / 4; b->comp = (u8*)xmalloc(b->comp_cap); }
	for (k = 0; k < b->n; k++) {
		u8* raw = b->h_bits + b->boff[k];
		const size_t n = b->sizes[k];
		raw[n] = n < s->persist_len ? s->persist[n] : 0;
		memcpy(s->persist, raw, n < s->persist_len ? n : s->persist_len);
		b->jobs[k].in = raw; b->jobs[k].n = (uint32_t)n; b->jobs[k].out = b->comp + coff;
		coff += n * (s->plan.lz77 ? 4 : 2) + 64;
	}
	pthread_mutex_lock(&s->mu);
	b->lz_left = b->n;
	pthread_mutex_unlock(&s->mu);
	for (k = 0; k < b->n; k++) {
		lzarg* za = (lzarg*)xmalloc(sizeof(*za));
		za->s = s; za->b = b; za->k = k;
		agmv_pool_submit(s->pool, lz_task, za);
	}
}

static void write_batch(agmv_seq* s, ebatch* b)
{
	unsigned k;
	const double t0 = now_s();
	for (k = 0; k < b->n; k++) {
		agmv_write_frame_chunk(s->file, s->a->frame_count + 1, b->sizes[k], b->jobs[k].csize, b->jobs[k].out);
		if (s->audio_chunks) AGMV_EncodeAudioChunk(s->file, s->a);
		s->a->frame_count++;
		s->frames_written++;
	}
	s->t_write += now_s() - t0;
}

/* the calling thread's share: prepare and write finished batches in order.  Returns when batch slot `want` is free
   (UNTIL_SLOT, want = the id about to be described), when everything submitted has been written (UNTIL_DRAINED) or when the
   batches that read a source before `want` have handed over (UNTIL_FREED, a ring source). */
enum { UNTIL_SLOT, UNTIL_DRAINED, UNTIL_FREED };
static void seq_progress(agmv_seq* s, unsigned long want, int until)
{
	pthread_mutex_lock(&s->mu);
	for (;;) {
		if (s->next_prep < s->nsubmitted) {
			ebatch* b = &s->slot[s->next_prep % s->nslots];
			if (b->id == s->next_prep && b->bits_ready) {
				pthread_mutex_unlock(&s->mu);
				prepare_batch(s, b);
				pthread_mutex_lock(&s->mu);
				s->next_prep++;
				continue;
			}
		}
		if (s->next_write < s->next_prep) {
			ebatch* b = &s->slot[s->next_write % s->nslots];
			if (b->lz_left == 0) {
				pthread_mutex_unlock(&s->mu);
				write_batch(s, b);
				pthread_mutex_lock(&s->mu);
				s->next_write++;
				pthread_cond_broadcast(&s->cv);
				continue;
			}
		}
		if (until == UNTIL_DRAINED ? s->next_write >= s->nsubmitted : until == UNTIL_SLOT ? want < s->next_write + s->nslots : s->src_free >= want) break;
		pthread_cond_wait(&s->cv, &s->mu);
	}
	pthread_mutex_unlock(&s->mu);
}

static void begin_batch(agmv_seq* s)
{
	const unsigned id = s->nsubmitted;
	ebatch* b;
	seq_progress(s, id, UNTIL_SLOT);                       /* until the slot of batch id - nslots has been written */
	b = &s->slot[id % s->nslots];
	b->id = id; b->n = 0; b->loaded = 0; b->bits_ready = 0; b->lz_left = 0;
	b->first_fc = s->fc0 + (id ? ((s->fc0 & 3u) ? (4u - (s->fc0 & 3u)) + (id - 1) * s->cap : id * s->cap) : 0);
	s->cur = b;
}

static unsigned batch_limit(const agmv_seq* s, const ebatch* b)
{
	return (b->id == 0 && (s->fc0 & 3u)) ? 4u - (s->fc0 & 3u) : s->cap;     /* a first batch that only completes the caller's GOP */
}

static void submit_batch(agmv_seq* s)
{
	ebatch* b = s->cur;
	unsigned k, tasks = 0;
	if (!b || !b->n) return;
	if (!s->plan.device_src) for (k = 0; k < b->n; k++) tasks += b->srcB[k] < 0 ? 1 : 2;
	b->src_end = (unsigned long)((b->srcB[b->n - 1] < 0 ? b->srcA[b->n - 1] : b->srcB[b->n - 1]) + 1 - s->src.first);     /* (the schedules push their sources in ascending order) */
	pthread_mutex_lock(&s->mu);
	b->loads_left = tasks;
	if (!tasks) b->loaded = 1;                             /* a device source: nothing to load, the batch is the worker's at once */
	s->nsubmitted++;
	pthread_cond_broadcast(&s->cv);
	pthread_mutex_unlock(&s->mu);
	for (k = 0; tasks && k < b->n; k++) {
		int which;
		for (which = 0; which < (b->srcB[k] < 0 ? 1 : 2); which++) {
			loadarg* la = (loadarg*)xmalloc(sizeof(*la));
			la->s = s; la->b = b; la->k = k; la->which = which;
			agmv_pool_submit(s->pool, load_task, la);
		}
	}
	s->cur = NULL;
}

/* Open and close, in pairs.  Every allocation is checked where it is made (xmalloc, pinned, on_device), what the plan does not call for stays NULL,
   and the closes free whatever is there.  One batch slot: h_pix only for a BMP source. */
static void eslot_open(const agmv_seq* s, ebatch* b)
{
	b->id = ~0u;
	b->srcA = (long*)xmalloc(sizeof(long) * s->cap); b->srcB = (long*)xmalloc(sizeof(long) * s->cap);
	b->boff = (size_t*)xmalloc(sizeof(size_t) * s->cap); b->jobs = (lzjob*)xcalloc(s->cap, sizeof(lzjob));
	if (!s->plan.device_src) b->h_pix = (uint32_t*)pinned(s->per * 4 * s->cap);
	b->sizes = (uint32_t*)pinned(4 * (size_t)s->cap + 64); b->csizes = (uint32_t*)pinned(4 * (size_t)s->cap + 64);
}

static void eslot_close(ebatch* b)
{
	free(b->srcA); free(b->srcB); free(b->boff); free(b->jobs); free(b->comp);
	agmv_hip_host_free(b->h_pix); agmv_hip_host_free(b->sizes); agmv_hip_host_free(b->csizes); agmv_hip_host_free(b->h_bits);
}

/* One worker: its context on `device` with the palette's tables, its stream and its buffers, sized by the plan (LZ77's payload rows: lz77_rows) */
static void eworker_open(agmv_seq* s, unsigned i, int device, const agmv_seq_opts* o)
{
	eworker* wk = &s->wk[i]; const eplan* p = &s->plan;
	agmv_hip_ctx* c = wk->ctx = agmv_hip_create(device);
	wk->s = s; wk->idx = i;
	if (!c) agmv_die("cannot open the GPU");
	if (o->pal && (agmv_hip_set_palette(c, o->pal, o->pal + 256, o->mode512, NULL) || agmv_hip_sync())) agmv_die("palette upload");
	if (!(wk->stream = agmv_hip_stream_create(c))) agmv_die("device allocation");
	wk->d_frames = (uint32_t*)on_device(c, s->npx * 4 * s->cap); wk->d_out = (uint8_t*)on_device(c, s->stride * s->cap);
	wk->d_sizes = (uint32_t*)on_device(c, 4 * (size_t)s->cap); wk->d_ient = (uint16_t*)on_device(c, s->npx * 2);
	if (p->midpoints && p->packs) { wk->d_tmp[0] = (uint32_t*)on_device(c, s->npx * 4); wk->d_tmp[1] = (uint32_t*)on_device(c, s->npx * 4); }
	if (p->lz_dev) wk->d_csize = (uint32_t*)on_device(c, 4 * (size_t)s->cap);
	if (p->lz_dev && !p->lz77) wk->d_lz = (uint8_t*)on_device(c, s->lz_stride * s->cap);
	if (p->lz_dev && p->lz77) wk->d_peek = (uint8_t*)on_device(c, s->cap);
	if (s->stabilise) wk->d_replaced = (unsigned long long*)zeroed_on_device(c, sizeof(unsigned long long), wk->stream);
}

/* ... behind its thread's join: the stabilisation's count joins the statistics (the worker synchronised its stream behind its last batch) */
static void eworker_close(eworker* wk)
{
	agmv_hip_ctx* c = wk->ctx; unsigned long long replaced = 0;
	if (wk->s->stabilise) {
		if (agmv_hip_memcpy_async(c, &replaced, wk->d_replaced, sizeof(replaced), 1, wk->stream) || agmv_hip_stream_sync(c, wk->stream)) agmv_die("stabilisation count download");
		g_stabilise_stats.examined += wk->examined; g_stabilise_stats.replaced += replaced;
	}
	agmv_hip_free_on(c, wk->d_replaced); agmv_hip_free_on(c, wk->d_frames); agmv_hip_free_on(c, wk->d_out); agmv_hip_free_on(c, wk->d_sizes); agmv_hip_free_on(c, wk->d_ient);
	agmv_hip_free_on(c, wk->d_tmp[0]); agmv_hip_free_on(c, wk->d_tmp[1]); agmv_hip_free_on(c, wk->d_lz); agmv_hip_free_on(c, wk->d_csize); agmv_hip_free_on(c, wk->d_peek);
	agmv_hip_stream_destroy(c, wk->stream); agmv_hip_destroy(c);
}

/* What all workers share, once, on worker 0's context and stream: a scaled device source's table, LZ77's persistent buffer (agmv_seq_close frees both) */
static void eshared_open(agmv_seq* s)
{
	eworker* wk = &s->wk[0]; uint32_t* index = NULL;
	if (s->plan.scaled) {
		s->d_index = agmv_source_index_dev(wk->ctx, wk->stream, &s->src, s->scale_w, s->scale_h, s->w, s->h, &index);
		if (!s->d_index || agmv_hip_stream_sync(wk->ctx, wk->stream)) agmv_die("scale table upload");
		free(index);
	}
	if (s->plan.lz_dev && s->plan.lz77) s->d_persist = (uint8_t*)zeroed_on_device(wk->ctx, s->persist_len, wk->stream);
}

agmv_seq* agmv_seq_open(AGMV* a, FILE* file, const agmv_source* src, const agmv_seq_opts* o)
{
	agmv_seq* s = (agmv_seq*)xcalloc(1, sizeof(*s));
	unsigned i, devices = o->devices < 1 ? 1 : o->devices;
	const unsigned ndev = (unsigned)agmv_hip_device_count();
	const double t0 = now_s(); double t1;
	if (ndev < 1) agmv_die("cannot open the GPU");
	/* AGMV_DEVICES_OVERSUBSCRIBE=1: more "devices" than cards -- worker pair d runs on card d % ndev.  The round-robin of batches over
	   devices, the in-order chunk writer and the per-device tables are then exercised on a one-GPU box. */
	if (devices > ndev && !env_nonzero("AGMV_DEVICES_OVERSUBSCRIBE")) devices = ndev;
	s->plan = eplan_of(src, o->scale_w, o->use_interp, o->lz77, devices);
	s->a = a; s->file = file; s->src = *src; s->scale_w = o->scale_w; s->scale_h = o->scale_h; s->audio_chunks = o->audio_chunks;
	s->w = (uint32_t)AGMV_GetWidth(a); s->h = (uint32_t)AGMV_GetHeight(a); s->fc0 = (u32)a->frame_count;
	s->npx = (size_t)s->w * s->h; s->per = s->npx * (s->plan.midpoints ? 2 : 1); s->stride = agmv_hip_max_usize(s->w, s->h, 1);
	s->lz_stride = (agmv_hip_lzss_max_csize(s->stride) + 255) & ~(size_t)255;
	s->stabilise = agmv_stabilise_strength(); s->dither = agmv_dither_strength();
	memset(&g_stabilise_stats, 0, sizeof(g_stabilise_stats));
	if (s->stabilise) TRACE("seq_open: temporal stabilisation of every batch before its dither and encode, strength %u\n", s->stabilise);
	if (s->dither) TRACE("seq_open: pattern dithering of every batch before its encode, strength %u\n", s->dither);
	s->cap = (o->cap + 3u) & ~3u; s->nworkers = s->plan.devices * 2; s->nslots = s->nworkers + 2;
	pthread_mutex_init(&s->mu, NULL); pthread_cond_init(&s->cv, NULL);
	s->pool = agmv_pool_start(o->threads); s->persist_len = s->stride + 64; s->persist = (u8*)xcalloc(s->persist_len, 1);
	s->slot = (ebatch*)xcalloc(s->nslots, sizeof(ebatch)); s->wk = (eworker*)xcalloc(s->nworkers, sizeof(eworker));
	for (i = 0; i < s->nslots; i++) eslot_open(s, &s->slot[i]);
	t1 = now_s();
	TRACE("seq_open: pool + %u pinned slots of %.1f MB in %.3f s\n", s->nslots, s->plan.device_src ? 0.0 : s->per * 4.0 * s->cap / 1e6, t1 - t0);
	for (i = 0; i < s->nworkers; i++)                          /* a device source is encoded where it lives */
		eworker_open(s, i, s->plan.device_src ? src->device : (int)((i % s->plan.devices) % ndev), o);
	eshared_open(s);
	for (i = 0; i < s->nworkers; i++)
		if (pthread_create(&s->wk[i].th, NULL, eworker_main, &s->wk[i])) agmv_die("cannot start a GPU worker thread");
	TRACE("seq_open: %u GPU workers (context + table + buffers) in %.3f s\n", s->nworkers, now_s() - t1);
	s->t_open = now_s();
	return s;
}

/* a sequence opened without a palette and a file (opts.pal NULL, file NULL) receives both here, before its first push: the workers exist and wait */
void agmv_seq_start(agmv_seq* s, FILE* file, const uint32_t* pal, int mode512)
{
	unsigned i;
	for (i = 0; i < s->nworkers; i++)
		if (agmv_hip_set_palette(s->wk[i].ctx, pal, pal + 256, mode512, NULL) || agmv_hip_sync()) agmv_die("palette upload");
	s->file = file;
}

/* a ring source: the sources before this one (counted from the clip's first) are read by no batch any more: their places in the ring are free */
unsigned long agmv_seq_sources_free(agmv_seq* s)
{
	unsigned long v;
	pthread_mutex_lock(&s->mu);
	v = s->src_free;
	pthread_mutex_unlock(&s->mu);
	return v;
}

/* ... the same once it has reached `want`, which a submitted batch must cover; the calling thread prepares and writes batches meanwhile */
unsigned long agmv_seq_wait_sources_free(agmv_seq* s, unsigned long want)
{
	seq_progress(s, want, UNTIL_FREED);
	return agmv_seq_sources_free(s);
}

void agmv_seq_counts(agmv_seq* s, unsigned* batches, unsigned long long* frames_written) { *batches = s->nsubmitted; *frames_written = s->frames_written; }

/* append one encoded frame: source `a`, or the PDIFS midpoint of sources a and b (b >= 0) */
void agmv_seq_push(agmv_seq* s, long a, long b)
{
	const long first = s->src.ring_frames ? s->src.first + (long)agmv_seq_sources_free(s) : s->src.first;    /* a ring holds ring_frames sources from the first that is not free */
	const long end = first + (long)(s->src.ring_frames ? s->src.ring_frames : s->src.n_frames);
	if (!s->cur) begin_batch(s);
	if (b >= 0 && !s->plan.midpoints) agmv_die("internal: midpoint frame on a sequence opened without interpolation");
	if (s->plan.device_src && (a < first || a >= end || b >= end || (b >= 0 && b < first))) agmv_die("internal: frame outside the device clip");
	s->cur->srcA[s->cur->n] = a; s->cur->srcB[s->cur->n] = b;
	if (++s->cur->n == batch_limit(s, s->cur)) submit_batch(s);
}

u32 agmv_seq_close(agmv_seq* s)
{
	unsigned i; u32 written; double t0;
	submit_batch(s);
	pthread_mutex_lock(&s->mu);
	s->closing = 1;
	pthread_cond_broadcast(&s->cv);
	pthread_mutex_unlock(&s->mu);
	seq_progress(s, 0, UNTIL_DRAINED);
	TRACE("pipeline: %u frames in %u batches, %.3f s from open to last chunk written; summed over the threads: BMP parse %.3f s, GPU workers "
	      "(upload + kernels + download) %.3f s, LZ (%s) %.3f s, chunk writes %.3f s\n", (unsigned)s->frames_written, s->nsubmitted, now_s() - s->t_open,
	      s->t_load, s->t_gpu, s->plan.lz_dev ? "device" : "host", s->t_lz, s->t_write);
	t0 = now_s();
	for (i = 0; i < s->nworkers; i++) pthread_join(s->wk[i].th, NULL);
	agmv_hip_free_on(s->wk[0].ctx, s->d_index); agmv_hip_free_on(s->wk[0].ctx, s->d_persist);       /* (eshared_open; every worker has been joined) */
	for (i = 0; i < s->nworkers; i++) eworker_close(&s->wk[i]);
	agmv_pool_stop(s->pool);
	for (i = 0; i < s->nslots; i++) eslot_close(&s->slot[i]);
	written = s->frames_written;
	if (s->stabilise)
		TRACE("seq_close: temporal stabilisation, strength %u: %llu of %llu P-frame blocks with their I-frame in the batch replaced\n", s->stabilise,
		      g_stabilise_stats.replaced, g_stabilise_stats.examined);
	TRACE("seq_close: teardown %.3f s\n", now_s() - t0);
	free(s->slot); free(s->wk); free(s->persist);
	pthread_mutex_destroy(&s->mu); pthread_cond_destroy(&s->cv);
	free(s);
	return written;
}

uint32_t agmv_writer_groups(uint32_t n, int heavy, int closed)
{
	const uint32_t step = heavy ? 2u : 4u;
	(void)closed;
	if (n < step) return 0;                                    /* (the first group reads `step` sources) */
	return n < 6 ? 1 : 1 + (n - 6) / step;                     /* group k >= 1 starts at k * step and needs k * step + 5 < n */
}

/* ------------------------------------------------------------------------------------------
 * pass 1 of the palette build: histogram of AGMV_QuantizeColor codes of every source frame at its ORIGINAL size (the
 * reference histograms before scaling, src/agmv_encode.c:2371-2397).  BMP parsing on the host cores, a window of frames
 * ahead of the GPU, which histograms them in order.
 * ------------------------------------------------------------------------------------------ */
typedef struct hframe { uint32_t w, h; int done; } hframe;
typedef struct hctx { pthread_mutex_t mu; pthread_cond_t cv; hframe* fr; uint32_t** ring; size_t ring_px; unsigned window; const char *dir, *base; u32 start; } hctx;
typedef struct harg { hctx* c; u32 i; } harg;

static void hist_load_task(void* p)
{
	harg* ha = (harg*)p;
	hctx* c = ha->c;
	hframe* f = &c->fr[ha->i];
	char path[4096];
	agmv_frame_path(path, sizeof(path), c->dir, c->base, (long)(c->start + ha->i));
	if (agmv_bmp_load_into(path, c->ring[ha->i % c->window], c->ring_px, &f->w, &f->h) != NO_ERR) die_unreadable(path);
	pthread_mutex_lock(&c->mu);
	f->done = 1;
	pthread_cond_broadcast(&c->cv);
	pthread_mutex_unlock(&c->mu);
	free(ha);
}

/* the clip is resident: no parse, no ring, no upload, one call over the n frames from `start` */
static void hist_resident(agmv_hip_ctx* ctx, const agmv_source* src, u32 start, u32 n, u32 size, int quality, uint32_t* d_hist, void* stream)
{
	const size_t fpx = (size_t)src->src_w * src->src_h, px = fpx < size ? fpx : size;
	const u8* d_first = (const u8*)src->d_frames + (size_t)((long)start - src->first) * agmv_fmt_frame_bytes(src->fmt, src->src_w, src->src_h);
	if ((long)start < src->first || (long)start + (long)n > src->first + (long)src->n_frames) agmv_die("internal: frame outside the device clip");
	if (agmv_fmt_histogram(ctx, src->fmt, src->src_w, src->src_h, d_first, n, px, quality, d_hist, stream)) agmv_die("histogram");
}

/* BMP files: a ring of pinned frames, parsed ahead of the GPU by the host cores; only the first `size` pixels of a frame count
   (the reference histograms img[0 .. width*height) of the size it was told, src/agmv_encode.c:2390-2394) */
static void hist_bmp_ring(agmv_hip_ctx* ctx, const agmv_source* src, u32 start, u32 n, u32 size, int quality, unsigned threads, uint32_t* d_hist, void* stream)
{
	agmv_pool* pool = agmv_pool_start(threads);
	hctx c = {.fr = (hframe*)xcalloc(n, sizeof(hframe)), .dir = src->dir, .base = src->base, .start = start, .ring_px = size, .window = threads + 2 < n ? threads + 2 : n};
	uint32_t* d_pix = (uint32_t*)on_device(ctx, c.ring_px * 4);
	u32 i, issued = 0;
	pthread_mutex_init(&c.mu, NULL);
	pthread_cond_init(&c.cv, NULL);
	c.ring = (uint32_t**)xcalloc(c.window, sizeof(uint32_t*));
	for (i = 0; i < c.window; i++) c.ring[i] = (uint32_t*)pinned(c.ring_px * 4);
	for (i = 0; i < n; i++) {
		hframe* f = &c.fr[i];
		size_t px;
		while (issued < n && issued < i + c.window) {      /* slot issued % window was consumed with frame issued - window */
			harg* ha = (harg*)xmalloc(sizeof(*ha));
			ha->c = &c; ha->i = issued++;
			agmv_pool_submit(pool, hist_load_task, ha);
		}
		pthread_mutex_lock(&c.mu);
		while (!f->done) pthread_cond_wait(&c.cv, &c.mu);
		pthread_mutex_unlock(&c.mu);
		px = (size_t)f->w * f->h < size ? (size_t)f->w * f->h : size;
		if (agmv_hip_memcpy_async(ctx, d_pix, c.ring[i % c.window], px * 4, 0, stream) || agmv_hip_histogram_dev(ctx, d_pix, px, quality, d_hist, stream) ||
		    agmv_hip_stream_sync(ctx, stream))
			agmv_die("histogram");
	}
	agmv_pool_stop(pool);
	for (i = 0; i < c.window; i++) agmv_hip_host_free(c.ring[i]);
	agmv_hip_free_on(ctx, d_pix);
	free(c.ring); free(c.fr);
	pthread_mutex_destroy(&c.mu);
	pthread_cond_destroy(&c.cv);
}

void agmv_histogram_frames(agmv_hip_ctx* ctx, const agmv_source* src, u32 start, u32 end, u32 size, int quality,
                           unsigned threads, uint32_t* hist /* 2^19 bins */)
{
	const u32 n = end >= start ? end - start + 1 : 0;
	const int resident = src->d_frames != NULL;
	const double t0 = now_s();
	uint32_t* d_hist;
	void* stream;
	if (n == 0) {                                              /* the reference's `for (i = start; i <= end; i++)` does not run (src/agmv_encode.c:2371-2397) */
		memset(hist, 0, 4u << 19);
		return;
	}
	d_hist = (uint32_t*)agmv_hip_malloc_on(ctx, 4u << 19);
	stream = agmv_hip_stream_create(ctx);
	if (!d_hist || !stream) agmv_die(resident ? "histogram" : "device allocation");
	if (agmv_hip_memset_async(ctx, d_hist, 0, 4u << 19, stream)) agmv_die("histogram");
	if (resident) hist_resident(ctx, src, start, n, size, quality, d_hist, stream);
	else hist_bmp_ring(ctx, src, start, n, size, quality, threads, d_hist, stream);
	if (agmv_hip_memcpy_async(ctx, hist, d_hist, 4u << 19, 1, stream) || agmv_hip_stream_sync(ctx, stream)) agmv_die("histogram download");
	agmv_hip_free_on(ctx, d_hist);
	agmv_hip_stream_destroy(ctx, stream);
	TRACE("palette pass 1: %u %sframes histogrammed in %.3f s\n", (unsigned)n, resident ? "resident " : "", now_s() - t0);
}


/* ------------------------------------------------------------------------------------------
 * decode pipeline
 * ------------------------------------------------------------------------------------------ */
typedef struct dbatch {
	unsigned n; uint32_t first;            /* the frames for the GPU stage, and the frame_count of the first of them */
	unsigned skip;                         /* a view: the slot's rows in front of them, the frames before g0, which do not enter the GPU stage */
	int fresh;                             /* the GPU stage takes this batch from the state of a fresh decoder (the first batch of a run, of a reader's seek) */
	u8* h_slab;                           /* pinned [cap][stride] (host LZ stage) */
	uint32_t *h_bpos, *h_out;              /* pinned [cap], [cap][npx] */
	uint8_t* d_slab; uint32_t* d_bpos;     /* AGMV_LZ_DECODE_DEVICE: the batch's rows [cap][stride] on the device, their bpos, and */
	void* ready;                           /* the event behind their commit on the LZ stage's stream */
	unsigned long name0;                   /* quick_export_<name0 + k>.bmp */
	int filled, decoded; unsigned saves_left;
} dbatch;

/* the last sequence decode's AGMV_DEBLOCK_STATS: zeroed when agmv_decode_stream opens, set when the run that delivered closes */
static AGMV_DEBLOCK_STATS g_deblock_stats;

void AGMV_GetDeblockStats(AGMV_DEBLOCK_STATS* out) { if (out) *out = g_deblock_stats; }

typedef struct dplan { int viewed, packed, in_place, direct, buffered, needs_scaled, view_whole, view_packs, deblock_buffered, to_bmp, lz_dev; } dplan;

typedef struct dpipe {
	agmv_hip_ctx* ctx; void* stream;
	uint32_t w, h; size_t npx, stride;
	unsigned cap, nslots; dbatch* slot;
	pthread_mutex_t mu; pthread_cond_t cv;
	unsigned nfilled; int closing, failed; /* nfilled: batches handed to the GPU worker */
	agmv_pool* pool; pthread_t th;
	uint8_t* d_bits; uint32_t *d_bpos, *d_nent, *d_out[2], *d_iframe;
	agmv_sink sink;                        /* where the batches go (agmv_pipeline.h) */
	dplan plan;                            /* ... and everything that is derived from it (dplan_of); each calls for one batch of: */
	uint32_t *d_scaled, *d_view, *d_deblock;               /* needs_scaled: scaled XRGB32 frames; view_packs: packed windows (sink_view); deblock_buffered: deblocked frames */
	void* d_table;                         /* the tensor sink's table on the device, uploaded once per call */
	uint32_t g0;                           /* a view: the GOP start at which the GPU stage begins, from the fresh state */
	int restart;                           /* ... the first decoded batch derives from the state before g0: the call runs again from frame 0 */
	unsigned gpu_frames;                   /* frames through the GPU stage */
	unsigned deblock;                      /* strength of the deblocking of every batch in front of its sink, 0 = off (AGMV_SetDeblock / AGMV_DEBLOCK) */
	unsigned long long* d_dbcounts;        /* deblock: [2] the weak and the strong lines of this run, downloaded behind the worker's join */
	size_t lz_cap; u8* persist;            /* the reference's ONE decompression buffer, zero-initialised, and its bytes (device LZ stage: dlz.d_persist) */
	struct dchunk* chunks; struct unlz* jobs;              /* [cap] the chunks of a batch, and the host LZ stage's jobs */
	agmv_dfile f;                          /* the file image the LZ stage reads ... */
	size_t pos; uint32_t done;             /* ... where it stands there, and the frames before that place: the next frame of the LZ stage */
	int fresh;                             /* the next batch handed over starts the GPU stage anew, at g0 */
	unsigned ndone;                        /* batches the worker has released (under mu) */
	unsigned long long lz_frames;          /* frames through the LZ stage, over all runs of this pipe */
	int keep;                              /* a reader's pipe: the worker outlives a restart, which the calling thread answers (dreader_read) */
	/* a reader's seek index (include/agmv_reader.h): checkpoint k > 0 is the persistent buffer as it stood before frame k * interval, in slot k - 1 of
	   ckpt (host LZ stage) or d_ckpt (device LZ stage, on the LZ context), with the place of that frame's chunk; checkpoint 0 is the zero buffer at the
	   first chunk and is not stored.  interval 0: no index (the one-shot drivers) */
	uint32_t interval, nckpt, *recorded; unsigned checkpoints;
	u8* ckpt; uint8_t* d_ckpt; size_t* ckpt_pos;
} dpipe;

/* The plan of a run over a w x h file: what the driver branches on, derived here alone.  Whatever the sink, a batch is decoded at the file's size.
   packed: a packed XRGB32 destination without a target size -- a clip of the file's size or, for a view, of its window's.
   in_place: that and no view: the clip holds every frame where the decoder puts it, and no converter runs.
   direct: in place and no deblocking: a batch is decoded straight into the caller's clip, and the frame before a batch is the one before it there.
   buffered: every other run decodes into the double buffer d_out, which exists for them alone; the decoder's state stays there, unfiltered, and the sink takes the batch from it.
   needs_scaled: the box filter makes XRGB32: straight into an XRGB32 clip, through d_scaled for any other layout and a tensor.
   view_whole: the view's window is the whole frame.  view_packs: the frames a view selects are packed into d_view first: not for a packed
   destination, which receives the windows itself, and not for consecutive whole frames, which are sunk from where they lie.
   deblock_buffered: the filter writes d_deblock, from where the sink takes the batch; only the clip in place receives the filter's output itself. */
static dplan dplan_of(const agmv_sink* s, uint32_t w, uint32_t h, unsigned deblock, int lz_dev)
{
	const agmv_target* t = agmv_sink_target(s);
	const int xrgb = s->kind == AGMV_SINK_FRAMES && s->frames.fmt == AGMV_PIXFMT_XRGB32;
	dplan p = {.viewed = s->viewed, .packed = xrgb && !t, .needs_scaled = t && t->filter == AGMV_SCALE_AREA && !xrgb, .to_bmp = s->kind == AGMV_SINK_EXPORT, .lz_dev = lz_dev};
	p.in_place = p.packed && !p.viewed; p.direct = p.in_place && !deblock; p.buffered = !p.direct; p.deblock_buffered = deblock && !p.in_place;
	p.view_whole = p.viewed && s->view.width == w && s->view.height == h;
	p.view_packs = p.viewed && !p.packed && !(s->view.step == 1 && p.view_whole);
	return p;
}

/* the bytes of one frame of the destination (MEASURE: of the reference clip); w x h is the file's size */
static size_t sink_frame_bytes(const agmv_sink* s, uint32_t w, uint32_t h)
{
	const agmv_target* t = agmv_sink_target(s);
	if (t) { w = t->w; h = t->h; }
	if (s->kind == AGMV_SINK_TENSOR) return agmv_hip_tensor_frame_bytes(s->tensor.type, (size_t)w * h);
	return agmv_fmt_frame_bytes(s->kind == AGMV_SINK_FRAMES ? s->frames.fmt : s->kind == AGMV_SINK_MEASURE ? s->measure.fmt : AGMV_PIXFMT_XRGB32, w, h);
}

typedef struct savearg { dpipe* d; dbatch* b; unsigned k; } savearg;

static void save_task(void* p)
{
	savearg* sa = (savearg*)p;
	dpipe* d = sa->d;
	char name[64];
	snprintf(name, sizeof(name), "quick_export_%lu.bmp", sa->b->name0 + sa->k);   /* AGIDL_QuickExport naming, agidl_img_export.c:20-41 */
	agmv_bmp_save(name, sa->b->h_out + (size_t)sa->k * d->npx, d->w, d->h);
	pthread_mutex_lock(&d->mu);
	if (--sa->b->saves_left == 0) { sa->b->filled = 0; sa->b->decoded = 0; pthread_cond_broadcast(&d->cv); }
	pthread_mutex_unlock(&d->mu);
	free(sa);
}

/* n frames of sw x sh at `out` -- batch b as it was decoded, or the frames and windows of it that a view selects -- to the sink as
   its frames `at_frame` onwards, on the worker's stream: one launch, behind the box filter's where that goes through d_scaled;
   for EXPORT the download to the slot's pinned frames; nothing for a batch decoded in place */
static int sink_batch(dpipe* d, const dbatch* b, const uint32_t* out, uint32_t sw, uint32_t sh, unsigned n, uint32_t at_frame)
{
	const agmv_sink* s = &d->sink;
	const agmv_target* t = agmv_sink_target(s);
	int filter = t ? t->filter : 0;                            /* (sw x sh: the size of the frames at `out`) the filter still to apply, the target size */
	const uint32_t tw = t ? t->w : sw, th = t ? t->h : sh;
	const size_t at = (size_t)at_frame * sink_frame_bytes(s, sw, sh);
	if (d->plan.needs_scaled) {
		if (agmv_hip_scale_area_dev(d->ctx, AGMV_PIXFMT_XRGB32, out, sw, sh, n, tw, th, d->d_scaled, d->stream)) return -1;
		out = d->d_scaled; sw = tw; sh = th; filter = 0;
	}
	switch (s->kind) {
	case AGMV_SINK_EXPORT:
		return agmv_hip_memcpy_async(d->ctx, b->h_out, out, d->npx * 4 * n, 1, d->stream);
	case AGMV_SINK_MEASURE:
		return agmv_hip_measure_frames_async(d->ctx, out, s->measure.fmt, (const u8*)s->measure.d_ref + at, sw, sh, n,
		                                     (u8*)s->measure.d_quality + sizeof(AGMV_FRAME_QUALITY) * (size_t)at_frame, d->stream);
	case AGMV_SINK_TENSOR:
		return agmv_hip_tensor_from_xrgb_async(d->ctx, s->tensor.type, out, sw, sh, n, filter, tw, th, d->d_table, (u8*)s->tensor.d_dst + at, d->stream);
	default: {
		void* dst = (u8*)s->frames.d_dst + at;
		if (filter == AGMV_SCALE_AREA) return agmv_hip_scale_area_dev(d->ctx, AGMV_PIXFMT_XRGB32, out, sw, sh, n, tw, th, (uint32_t*)dst, d->stream);
		if (filter) return agmv_hip_scale_frames_async(d->ctx, filter, out, sw, sh, n, s->frames.fmt, tw, th, dst, d->stream);
		return d->plan.in_place ? 0 : agmv_fmt_from_xrgb(d->ctx, s->frames.fmt, tw, th, out, n, dst, d->stream);      /* XRGB32 to the caller's layout */
	}
	}
}

uint32_t agmv_view_length(uint32_t first, uint32_t step, uint32_t count, uint32_t nframes)
{
	const uint32_t n = first < nframes ? (nframes - first - 1) / step + 1 : 0;
	return count && count < n ? count : n;
}

uint32_t agmv_view_in_batch(uint32_t first, uint32_t step, uint32_t count, uint32_t batch_first, uint32_t batch_n, uint32_t* row, uint32_t* index)
{
	const uint64_t end = (uint64_t)batch_first + batch_n;       /* the view's frame j is frame first + j * step of the file */
	const uint64_t j0 = batch_first > first ? ((uint64_t)(batch_first - first) + step - 1) / step : 0, f0 = first + j0 * step;
	uint64_t j1;
	if (batch_n == 0 || f0 >= end || (count && j0 >= count)) return 0;
	j1 = (end - 1 - first) / step;                              /* the last j of the batch, then of the view */
	if (count && j1 >= count) j1 = count - 1;
	*row = (uint32_t)(f0 - batch_first); *index = (uint32_t)j0;
	return (uint32_t)(j1 - j0 + 1);
}

/* the nd frames decoded at `out`, the first of them frame f0 of the file, to the sink of a view: the frames the view selects,
   packed with their windows by one launch, then sunk as a batch of a file of the window's size.  Two shortcuts: consecutive full
   frames are sunk from where they lie, and a packed XRGB32 destination at the window's size receives the copy itself. */
static int sink_view(dpipe* d, const dbatch* b, const uint32_t* out, uint32_t f0, unsigned nd)
{
	const AGMV_VIEW* v = &d->sink.view;
	const int packed = d->plan.packed;
	const size_t wpx = (size_t)v->width * v->height;
	uint32_t row, index, *win;
	const uint32_t len = agmv_view_in_batch(v->first, v->step, v->count, f0, nd, &row, &index);
	if (!len) return 0;
	*d->sink.count += len;                                     /* (this thread alone writes it during a view; it is read behind the join) */
	win = packed ? (uint32_t*)d->sink.frames.d_dst + index * wpx : d->d_view;
	if (d->plan.view_whole && (v->step == 1 || len == 1)) {
		const uint32_t* src = out + (size_t)row * d->npx;
		return packed ? agmv_hip_memcpy_async(d->ctx, win, src, wpx * 4 * len, 2, d->stream) : sink_batch(d, b, src, d->w, d->h, len, index);
	}
	if (agmv_hip_view_frames_async(d->ctx, out, d->w, d->h, row, v->step, len, v->x, v->y, v->width, v->height, win, d->stream)) return -1;
	return packed ? 0 : sink_batch(d, b, win, v->width, v->height, len, index);
}

/* The worker, by step.  Take: batch id once the calling thread has handed it over; NULL when the pipe closes with none left. */
static dbatch* dworker_take(dpipe* d, unsigned id)
{
	int handed;
	pthread_mutex_lock(&d->mu);
	while (!(id < d->nfilled) && !d->closing) pthread_cond_wait(&d->cv, &d->mu);
	handed = id < d->nfilled;
	pthread_mutex_unlock(&d->mu);
	return handed ? &d->slot[id % d->nslots] : NULL;
}

/* Decode: the frames of batch id to *at on the worker's stream, behind the upload of their rows or, on the device, the LZ stage's commit; then
   the state for the next batch.  prev_n: the frames of the batch before, 0 = the fresh state.  Returns 0, negative on error, 1 for the restart. */
static int dworker_decode(dpipe* d, const dbatch* b, unsigned id, unsigned prev_n, uint32_t** at)
{
	const int direct = d->plan.direct;
	const uint32_t skip = b->skip, n = b->n, first = b->first;
	const uint8_t* bits = b->d_slab ? b->d_slab + (size_t)skip * d->stride : d->d_bits;
	const uint32_t* bpos = b->d_slab ? b->d_bpos + skip : d->d_bpos;
	uint32_t* out = *at = direct ? (uint32_t*)d->sink.frames.d_dst + (size_t)first * d->npx : d->d_out[id & 1];
	const uint32_t* prev = !prev_n ? NULL : direct ? out - d->npx : d->d_out[(id - 1) & 1] + (size_t)(prev_n - 1) * d->npx;
	unsigned k; int last_i = -1, dependent;
	if (b->d_slab) {                       /* the LZ stage left the rows on the device: wait for their commit, on the device */
		if (agmv_hip_stream_wait_event(d->ctx, d->stream, b->ready)) return -1;
	} else if (agmv_hip_memcpy_async(d->ctx, d->d_bits, b->h_slab + (size_t)skip * d->stride, d->stride * n, 0, d->stream) ||
	           agmv_hip_memcpy_async(d->ctx, d->d_bpos, b->h_bpos + skip, 4 * (size_t)n, 0, d->stream))
		return -1;
	if (agmv_hip_decode_bitstreams_dev(d->ctx, bits, d->stride, bpos, n, d->w, d->h, first, d->d_nent, out, prev, prev_n ? d->d_iframe : NULL, d->stream)) return -1;
	d->gpu_frames += n;
	/* a view that starts inside the file: is this batch a function of its own streams alone? */
	dependent = !prev_n && d->g0 ? agmv_hip_decode_prior_dependent(d->ctx, d->w, d->h, d->stream) : 0;
	if (dependent) return dependent < 0 ? -1 : 1;
	/* the state stays on the device: img_data = the last frame (read in place from this batch's output), iframe = the last I-frame of the batch (src/agmv_decode.c:401-405) */
	for (k = 0; k < n; k++) if (((first + k) & 3u) == 0) last_i = (int)k;
	if (!prev_n && last_i < 0 && agmv_hip_memset_async(d->ctx, d->d_iframe, 0, d->npx * 4, d->stream)) return -1;
	if (last_i >= 0 && agmv_hip_memcpy_async(d->ctx, d->d_iframe, out + (size_t)last_i * d->npx, d->npx * 4, 2, d->stream)) return -1;
	return 0;
}

/* Deliver: the sinks' frames are the batch as it was decoded, or, behind the snapshot, its deblocked copy (whole frames at the file's size, before a
   view's window and stride and before any scaling) -- in the caller's clip where that is in place.  On return the frames are where they belong. */
static int dworker_deliver(dpipe* d, const dbatch* b, const uint32_t* out)
{
	if (d->deblock) {
		uint32_t* to = d->plan.deblock_buffered ? d->d_deblock : (uint32_t*)d->sink.frames.d_dst + (size_t)b->first * d->npx;
		if (agmv_hip_deblock_frames_async(d->ctx, d->deblock, out, d->w, d->h, b->n, to, d->d_dbcounts, d->stream)) return -1;
		out = to;
	}
	if (d->plan.viewed ? sink_view(d, b, out, b->first, b->n) : sink_batch(d, b, out, d->w, d->h, b->n, b->first)) return -1;
	return agmv_hip_stream_sync(d->ctx, d->stream) ? -1 : 0;
}

/* Release: the slot is free again, for the BMP export once the pool has saved its frames */
static void dworker_release(dpipe* d, dbatch* b)
{
	const unsigned saves = d->plan.to_bmp ? b->n : 0; unsigned k;
	pthread_mutex_lock(&d->mu);
	if (!saves) b->filled = 0;                         /* the frames are where they belong */
	else { b->decoded = 1; b->saves_left = saves; }
	d->ndone++;
	pthread_cond_broadcast(&d->cv);
	pthread_mutex_unlock(&d->mu);
	for (k = 0; k < saves; k++) {
		savearg* sa = (savearg*)xmalloc(sizeof(*sa));
		sa->d = d; sa->b = b; sa->k = k;
		agmv_pool_submit(d->pool, save_task, sa);
	}
}

static void* dworker_main(void* p)
{
	dpipe* d = (dpipe*)p;
	unsigned id, prev_n = 0;
	dbatch* b; uint32_t* out;
	for (id = 0; (b = dworker_take(d, id)) != NULL; id++) {
		int rc;
		if (b->fresh) prev_n = 0;
		if (d->keep && d->restart) { dworker_release(d, b); continue; }      /* (a reader's run that is given up: its later batches are dropped) */
		rc = dworker_decode(d, b, id, prev_n, &out);
		if (!rc) rc = dworker_deliver(d, b, out);
		if (rc > 0 && d->keep) {               /* a reader: the calling thread finds `restart` behind this batch and runs again from frame 0 */
			pthread_mutex_lock(&d->mu);
			d->restart = 1;
			pthread_mutex_unlock(&d->mu);
			dworker_release(d, b);
			continue;
		}
		if (rc) {                              /* (failed: what stops the batch loop, for the restart too) */
			if (rc < 0) fprintf(stderr, "libagmv(amd): batch decode: %s (the AGMV hot path runs on the GPU only -- no CPU fallback)\n", agmv_hip_last_error());
			pthread_mutex_lock(&d->mu);
			d->failed = 1; d->restart = rc > 0;
			pthread_cond_broadcast(&d->cv);
			pthread_mutex_unlock(&d->mu);
			break;
		}
		prev_n = b->n;
		dworker_release(d, b);
	}
	return NULL;
}

/* AGMV_FindNextFrameChunk / AGMV_FindNextAudioChunk (reference src/agmv_utils.c:140-194) from pos: the four bytes at pos are compared
   once, the loop behind them reads its first four from pos + 4 and only then steps by one byte, so a FourCC that starts 1, 2 or 3
   bytes behind pos is not found.  Returns len where the reference would never return. */
static size_t scan_fourcc(const u8* d, size_t len, size_t pos, const char* cc)
{
	if (pos + 4 <= len && memcmp(d + pos, cc, 4) == 0) return pos;
	pos += 4;
	while (pos + 4 <= len) {
		if (memcmp(d + pos, cc, 4) == 0) return pos;
		pos++;
	}
	return len;
}

static uint32_t le32(const u8* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

/* where the reference's reader stands behind a frame chunk at c whose LZ stage consumed `used` payload bytes (audio: AGMV_FindNextAudioChunk
   + the chunk's payload) */
static size_t behind_chunk(const u8* file, size_t len, size_t c, size_t used, int has_audio)
{
	size_t pos = c + 16 + used;
	if (has_audio) {
		size_t ac = scan_fourcc(file, len, pos, "AGAC");
		if (ac + 8 <= len) pos = ac + 8 + le32(file + ac + 4);
	}
	return pos;
}

/* Where frame k+1's chunk is depends on how many payload bytes the bit reader of frame k consumed (it runs past csize into
   the guard, src/agmv_decode.c:171-198).  So the chunks of a batch are first located as if every reader stopped right
   behind its payload (locate_chunks), the LZ stage decompresses them all at once and reports what each reader consumed,
   and the true positions are then checked in order (cut_batch): at the first chunk that was not where it was assumed the
   batch is cut, and the next one starts from the true position.  A chunk: its "AGFC" at `at`, the usize and csize fields of its 16-byte header, the
   `avail` bytes of file behind that header, the `used` payload bytes that its LZ stage reports; chunk_payload: the payload bytes that the file holds. */
typedef struct dchunk { size_t at; uint32_t usize, csize; size_t avail, used; } dchunk;
static size_t chunk_payload(const dchunk* c) { return c->csize < c->avail ? c->csize : c->avail; }

static unsigned locate_chunks(const u8* file, size_t len, size_t pos, int has_audio, dchunk* c, unsigned want)
{
	unsigned n;
	for (n = 0; n < want; n++) {
		const size_t at = scan_fourcc(file, len, pos, "AGFC");
		if (at + 16 > len) break;
		c[n].at = at; c[n].usize = le32(file + at + 8); c[n].csize = le32(file + at + 12); c[n].avail = len - (at + 16);
		pos = behind_chunk(file, len, at, chunk_payload(&c[n]), has_audio);
	}
	return n;
}

/* The AGAC payloads of the first nframes frames, back to back in out[0, cap): the walk of AGMV_DecodeAudio (reference
   src/agmv_decode.c:725-729), which skips every frame chunk by its csize field -- what locate_chunks assumes of a reader -- and
   reads each audio chunk's own size field.  Payload bytes the file does not hold are zeros.  Returns the bytes gathered. */
size_t agmv_gather_audio(const u8* file, size_t len, size_t pos, uint32_t nframes, u8* out, size_t cap)
{
	dchunk c[64];
	size_t total = 0;
	while (nframes && total < cap) {
		const unsigned want = nframes < 64 ? (unsigned)nframes : 64u, n = locate_chunks(file, len, pos, 1, c, want);
		unsigned k;
		for (k = 0; k < n && total < cap; k++) {
			const size_t ac = scan_fourcc(file, len, c[k].at + 16 + chunk_payload(&c[k]), "AGAC");
			size_t size, held;
			if (ac + 8 > len) return total;
			size = le32(file + ac + 4);
			if (size > cap - total) size = cap - total;
			held = size < len - (ac + 8) ? size : len - (ac + 8);
			memcpy(out + total, file + ac + 8, held);
			memset(out + total + held, 0, size - held);
			total += size;
			pos = ac + 8 + le32(file + ac + 4);
		}
		if (n < want) break;
		nframes -= n;
	}
	return total;
}

/* *pos = the true position behind the last chunk that was where it was assumed; returns the frames up to and including it
   (the rest was decompressed from the wrong place) */
static unsigned cut_batch(const u8* file, size_t len, int has_audio, const dchunk* c, unsigned n, size_t* pos)
{
	unsigned k;
	for (k = 0; k < n; k++) {
		*pos = behind_chunk(file, len, c[k].at, c[k].used, has_audio);
		if (k + 1 < n && scan_fourcc(file, len, *pos, "AGFC") != c[k + 1].at) return k + 1;
	}
	return n;
}

uint32_t agmv_reader_checkpoint(uint32_t nframes, size_t lz_cap, size_t index_bytes, uint32_t f, const uint32_t* recorded, uint32_t* interval)
{
	const uint64_t n = nframes ? nframes : 1, slots = lz_cap ? index_bytes / lz_cap : n;          /* the checkpoints the budget holds */
	uint64_t iv = slots ? (n + slots - 1) / slots : n;                                             /* the least interval with ceil(n / iv) <= slots */
	uint32_t k;
	iv = iv < 4 ? 4 : (iv + 3) & ~(uint64_t)3;
	if (iv > 0xFFFFFFFCu) iv = 0xFFFFFFFCu;
	if (interval) *interval = (uint32_t)iv;
	k = (uint32_t)(((uint64_t)(f & ~3u) < n ? (f & ~3u) : n - 1) / iv);                            /* (a frame behind the file: the last checkpoint the file has) */
	while (k > 0 && !(recorded && (recorded[k >> 5] >> (k & 31) & 1u))) k--;
	return k * (uint32_t)iv;
}

/* a reader's LZ stage stands in front of frame f: is that a checkpoint it has not recorded yet?  Then the caller copies the buffer and says so */
static int checkpoint_due(const dpipe* d, uint32_t f)
{
	return d->interval && f && f % d->interval == 0 && f / d->interval < d->nckpt && !(d->recorded[f / d->interval >> 5] >> (f / d->interval & 31) & 1u);
}

static void checkpoint_recorded(dpipe* d, uint32_t f, size_t at)
{
	const uint32_t k = f / d->interval;
	d->recorded[k >> 5] |= 1u << (k & 31); d->ckpt_pos[k] = at; d->checkpoints++;
}

/* the host LZ stage of one frame on a pool thread: straight into the frame's row of the batch slab (the decoder copies only
   from bytes it has written itself, src < bpos, so the row's old content does not matter) */
typedef struct unlz { dpipe* d; int ver; const u8* payload; dchunk* c; size_t cap; uint32_t bpos; u8* row; unsigned* left; } unlz;

static void unlz_task(void* p)
{
	unlz* j = (unlz*)p;
	dpipe* d = j->d;
	j->bpos = agmv_lz_decode_mem(j->ver, j->payload, j->c->avail, j->c->usize, j->c->csize, j->row, j->cap, &j->c->used);
	pthread_mutex_lock(&d->mu);
	if (--*j->left == 0) pthread_cond_broadcast(&d->cv);
	pthread_mutex_unlock(&d->mu);
}

/* AGMV_LZ_DECODE_DEVICE=1: the LZ stage of a batch on the GPU (agmv_hip_lz_decode_frames_dev + agmv_hip_lz_decode_commit_dev),
   on a context and stream of its own (the worker thread owns the decoder's context), into the device rows of the batch's
   slot.  The persistent buffer stays on the device, zero-initialised like `persist`. */
typedef struct dlz {
	agmv_hip_ctx* ctx;
	void* stream;
	u8* h_stage;                           /* pinned: the file range that holds a batch's rows ... */
	uint8_t* d_src; size_t src_cap;        /* ... and its device copy, src_cap bytes each */
	uint8_t* d_persist;
	unsigned long long *h_off, *d_off;     /* pinned / device [cap] */
	uint32_t *h_avail, *h_usize, *h_csize, *h_used;              /* pinned [cap] each */
	uint32_t* d_used;                      /* device [cap] */
	unsigned batches;
	double secs;
} dlz;

static int dlz_open(dlz* z, agmv_hip_ctx* ctx, unsigned cap_frames, size_t cap)
{
	const size_t n = cap_frames;
	memset(z, 0, sizeof(*z));
	z->ctx = agmv_hip_create(agmv_hip_ctx_device(ctx));
	if (!z->ctx) return -1;
	z->stream = agmv_hip_stream_create(z->ctx);
	z->d_persist = (uint8_t*)agmv_hip_malloc_on(z->ctx, cap);
	z->h_off = (unsigned long long*)agmv_hip_host_alloc(8 * n);
	z->d_off = (unsigned long long*)agmv_hip_malloc_on(z->ctx, 8 * n);
	z->h_avail = (uint32_t*)agmv_hip_host_alloc(4 * 4 * n);
	z->d_used = (uint32_t*)agmv_hip_malloc_on(z->ctx, 4 * n);
	if (!z->stream || !z->d_persist || !z->h_off || !z->d_off || !z->h_avail || !z->d_used) return -1;
	z->h_usize = z->h_avail + n; z->h_csize = z->h_usize + n; z->h_used = z->h_csize + n;
	return agmv_hip_memset_async(z->ctx, z->d_persist, 0, cap, z->stream) || agmv_hip_stream_sync(z->ctx, z->stream) ? -1 : 0;
}

static void dlz_close(dlz* z)
{
	if (!z->ctx) return;
	agmv_hip_host_free(z->h_stage); agmv_hip_host_free(z->h_off); agmv_hip_host_free(z->h_avail);
	agmv_hip_free_on(z->ctx, z->d_src); agmv_hip_free_on(z->ctx, z->d_persist); agmv_hip_free_on(z->ctx, z->d_off);
	agmv_hip_free_on(z->ctx, z->d_used);
	agmv_hip_stream_destroy(z->ctx, z->stream);
	agmv_hip_destroy(z->ctx);
}

/* locate up to `want` chunks from *pos, upload the file range that holds their rows in one copy, decompress them into b's
   device rows, read back used (the one synchronisation a batch needs), cut the batch, commit the frames before the cut to
   the persistent buffer and record b->ready behind the commit: the worker's stream waits for that event, not the host.
   Returns the frames of the batch (0: none left), negative on error. */
static int dlz_batch(dlz* z, dpipe* d, dbatch* b, unsigned want)
{
	const u8* file = d->f.image; const size_t len = d->f.len, cap = d->lz_cap; const int has_audio = d->f.has_audio;
	dchunk* c = d->chunks;
	const double t0 = now_s();
	unsigned n = locate_chunks(file, len, d->pos, has_audio, c, want), k, k1;
	size_t lo, hi = 0;
	if (!n) return 0;
	lo = c[0].at + 16;
	for (k = 0; k < n; k++) {
		const size_t r = (size_t)c[k].csize + 3 < c[k].avail ? (size_t)c[k].csize + 3 : c[k].avail;       /* the most a reader fetches */
		if (c[k].at + 16 + r > hi) hi = c[k].at + 16 + r;
		z->h_off[k] = c[k].at + 16 - lo;
		z->h_avail[k] = c[k].avail > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)c[k].avail;
		z->h_usize[k] = c[k].usize; z->h_csize[k] = c[k].csize;
	}
	if (hi - lo + 1 > z->src_cap) {
		agmv_hip_host_free(z->h_stage); agmv_hip_free_on(z->ctx, z->d_src);
		z->src_cap = (hi - lo + 1) * 5 / 4 + 4096;
		z->h_stage = (u8*)agmv_hip_host_alloc(z->src_cap);
		z->d_src = (uint8_t*)agmv_hip_malloc_on(z->ctx, z->src_cap);
		if (!z->h_stage || !z->d_src) { z->src_cap = 0; return -1; }
	}
	memcpy(z->h_stage, file + lo, hi - lo);
	/* (the staging and h_off of the batch before are free again: the read of its `used` waited for its uploads) */
	if (agmv_hip_memcpy_async(z->ctx, z->d_src, z->h_stage, hi - lo, 0, z->stream) ||
	    agmv_hip_memcpy_async(z->ctx, z->d_off, z->h_off, 8 * (size_t)n, 0, z->stream) ||
	    agmv_hip_lz_decode_frames_sized_dev(z->ctx, d->f.ver, z->d_src, z->d_off, z->h_avail, z->h_usize, z->h_csize, n, b->d_slab, d->stride,
	                                        cap, b->d_bpos, z->d_used, z->stream) ||
	    agmv_hip_memcpy_async(z->ctx, z->h_used, z->d_used, 4 * (size_t)n, 1, z->stream) ||
	    agmv_hip_stream_sync(z->ctx, z->stream))
		return -1;
	for (k = 0; k < n; k++) c[k].used = z->h_used[k];
	n = cut_batch(file, len, has_audio, c, n, &d->pos);
	/* one commit -- or, for a reader, one per stretch between the checkpoints the batch passes, each taken from the buffer in front of its frame */
	for (k = 0; k < n; k = k1) {
		if (checkpoint_due(d, d->done + k)) {
			if (agmv_hip_memcpy_async(z->ctx, d->d_ckpt + (size_t)((d->done + k) / d->interval - 1) * cap, z->d_persist, cap, 2, z->stream)) return -1;
			checkpoint_recorded(d, d->done + k, c[k].at);
		}
		k1 = d->interval && d->interval - (d->done + k) % d->interval < n - k ? k + d->interval - (d->done + k) % d->interval : n;
		if (agmv_hip_lz_decode_commit_dev(z->ctx, b->d_slab + (size_t)k * d->stride, d->stride, b->d_bpos + k, k1 - k, z->d_persist, cap, z->stream)) return -1;
	}
	if (agmv_hip_event_record(z->ctx, b->ready, z->stream)) return -1;
	z->batches++;
	z->secs += now_s() - t0;
	return (int)n;
}

/* The host LZ stage of a batch, dlz_batch's counterpart: locate up to `want` chunks from *pos, decompress them on the pool, one frame per task, into
   the rows of b's pinned slab, cut the batch, and then, in frame order and for the frames before the cut, a row takes its stale tail from the
   persistent buffer and the buffer takes the row.  Returns the frames of the batch (0: none left); nothing in this stage can fail. */
static int host_lz_batch(dpipe* d, dbatch* b, unsigned want)
{
	const u8* file = d->f.image; const size_t len = d->f.len, cap = d->lz_cap; const int has_audio = d->f.has_audio;
	dchunk* c = d->chunks;
	unsigned left, k, n = left = locate_chunks(file, len, d->pos, has_audio, c, want);
	for (k = 0; k < n; k++) {
		unlz* j = &d->jobs[k];
		j->d = d; j->ver = d->f.ver; j->c = &c[k]; j->left = &left; j->cap = cap;
		j->payload = file + c[k].at + 16; j->row = b->h_slab + (size_t)k * d->stride;
		agmv_pool_submit(d->pool, unlz_task, j);
	}
	pthread_mutex_lock(&d->mu);
	while (left) pthread_cond_wait(&d->cv, &d->mu);
	pthread_mutex_unlock(&d->mu);
	n = cut_batch(file, len, has_audio, c, n, &d->pos);
	for (k = 0; k < n; k++) {                              /* in order: (a reader's checkpoint in front of the frame,) stale bytes, persistent buffer */
		const unlz* j = &d->jobs[k];
		const size_t bp = j->bpos, tail = bp + 16 < d->stride ? 16 : (bp < d->stride ? d->stride - bp : 0);
		if (checkpoint_due(d, d->done + k)) {
			memcpy(d->ckpt + (size_t)((d->done + k) / d->interval - 1) * cap, d->persist, cap);
			checkpoint_recorded(d, d->done + k, c[k].at);
		}
		if (tail) memcpy(j->row + bp, d->persist + bp, tail);
		memcpy(d->persist, j->row, bp < cap ? bp : cap);
		b->h_bpos[k] = j->bpos;
	}
	return (int)n;
}

/* Everything a run holds, from the plan: a buffer the plan does not call for stays NULL, one it calls for is checked where it is
   made.  The pool and the worker start last.  Returns 0, or -1 with the pipe half-opened: dpipe_close takes it as it is. */
static int dpipe_open(dpipe* d, dlz* z, agmv_hip_ctx* ctx, const agmv_dfile* f, unsigned cap_frames, unsigned threads, const agmv_sink* sink, uint32_t g0, unsigned deblock)
{
	const uint32_t w = f->w, h = f->h;
	const char* lzv = getenv("AGMV_LZ_DECODE_DEVICE");     /* opt-in: the LZ stage on the GPU (read when a decode starts) */
	const dplan* p = &d->plan;
	const agmv_target* t = agmv_sink_target(sink);
	const size_t table = sink->kind == AGMV_SINK_TENSOR ? agmv_hip_tensor_frame_bytes(sink->tensor.type, 256) : 0;       /* 3 x 256 elements, uploaded once per call */
	const size_t npx = (size_t)w * h, lz_cap = npx * 33 / 16 + 4096, stride = (lz_cap + 255) & ~(size_t)255;
	const size_t batch = npx * 4 * cap_frames, rows = stride * cap_frames;     /* a batch of XRGB32 frames at the file's size; of LZ stage rows */
	unsigned i;
	memset(d, 0, sizeof(*d)); memset(z, 0, sizeof(*z));
	pthread_mutex_init(&d->mu, NULL); pthread_cond_init(&d->cv, NULL);
	d->ctx = ctx; d->w = w; d->h = h; d->npx = npx; d->lz_cap = lz_cap; d->stride = stride; d->cap = cap_frames;
	d->sink = *sink; d->g0 = g0; d->deblock = deblock; d->plan = dplan_of(sink, w, h, deblock, lzv && atoi(lzv) == 1);
	d->f = *f; d->pos = f->pos; d->fresh = 1;
	d->persist = (u8*)calloc(lz_cap, 1); d->chunks = (dchunk*)calloc(d->cap, sizeof(dchunk)); d->slot = (dbatch*)calloc(3, sizeof(dbatch));
	if (!d->persist || !d->chunks || !d->slot || (!p->lz_dev && !(d->jobs = (unlz*)calloc(d->cap, sizeof(unlz))))) return -1;
	d->nslots = 3;
	if (!(d->stream = agmv_hip_stream_create(ctx))) return -1;
	if (!p->lz_dev && (!(d->d_bits = (uint8_t*)agmv_hip_malloc_on(ctx, rows)) || !(d->d_bpos = (uint32_t*)agmv_hip_malloc_on(ctx, 4 * (size_t)d->cap)))) return -1;
	if (!(d->d_nent = (uint32_t*)agmv_hip_malloc_on(ctx, 4 * (size_t)d->cap))) return -1;         /* (d_bits: the host LZ stage's upload slab) */
	if (p->buffered && (!(d->d_out[0] = (uint32_t*)agmv_hip_malloc_on(ctx, batch)) || !(d->d_out[1] = (uint32_t*)agmv_hip_malloc_on(ctx, batch)))) return -1;
	if (!(d->d_iframe = (uint32_t*)agmv_hip_malloc_on(ctx, npx * 4))) return -1;
	if (p->needs_scaled && !(d->d_scaled = (uint32_t*)agmv_hip_malloc_on(ctx, (size_t)t->w * t->h * 4 * d->cap))) return -1;
	if (p->view_packs && !(d->d_view = (uint32_t*)agmv_hip_malloc_on(ctx, (size_t)sink->view.width * sink->view.height * 4 * d->cap))) return -1;
	if (p->deblock_buffered && !(d->d_deblock = (uint32_t*)agmv_hip_malloc_on(ctx, batch))) return -1;
	if (deblock && (!(d->d_dbcounts = (unsigned long long*)agmv_hip_malloc_on(ctx, 2 * sizeof(unsigned long long))) ||       /* the counters of this run */
	                agmv_hip_memset_async(ctx, d->d_dbcounts, 0, 2 * sizeof(unsigned long long), d->stream) || agmv_hip_stream_sync(ctx, d->stream)))
		return -1;
	if (table && (!(d->d_table = agmv_hip_malloc_on(ctx, table)) || agmv_hip_memcpy_async(ctx, d->d_table, sink->tensor.table, table, 0, d->stream) ||
	              agmv_hip_stream_sync(ctx, d->stream)))
		return -1;
	if (p->lz_dev && dlz_open(z, ctx, d->cap, d->lz_cap)) return -1;
	for (i = 0; i < d->nslots; i++) {                      /* a slot's rows: with the LZ stage on the device they live there only */
		dbatch* b = &d->slot[i];
		if (p->lz_dev && (!(b->d_slab = (uint8_t*)agmv_hip_malloc_on(ctx, rows)) || !(b->d_bpos = (uint32_t*)agmv_hip_malloc_on(ctx, 4 * (size_t)d->cap)) ||
		                  !(b->ready = agmv_hip_event_create(ctx))))
			return -1;
		if (!p->lz_dev && (!(b->h_slab = (u8*)agmv_hip_host_alloc(rows)) || !(b->h_bpos = (uint32_t*)agmv_hip_host_alloc(4 * (size_t)d->cap + 64)))) return -1;
		if (p->to_bmp && !(b->h_out = (uint32_t*)agmv_hip_host_alloc(batch))) return -1;
	}
	d->pool = agmv_pool_start(threads);
	if (!pthread_create(&d->th, NULL, dworker_main, d)) return 0;
	agmv_pool_stop(d->pool);                               /* no worker: nothing to join, nothing would ever consume a batch */
	return -1;
}

/* frees what dpipe_open made, however far it came; the worker is joined and the pool stopped before */
static void dpipe_close(dpipe* d, dlz* z)
{
	agmv_hip_ctx* ctx = d->ctx; unsigned i;
	for (i = 0; i < d->nslots; i++) {
		const dbatch* b = &d->slot[i];
		agmv_hip_host_free(b->h_slab); agmv_hip_host_free(b->h_bpos); agmv_hip_host_free(b->h_out);
		agmv_hip_free_on(ctx, b->d_slab); agmv_hip_free_on(ctx, b->d_bpos); agmv_hip_event_destroy(ctx, b->ready);
	}
	if (z->ctx) agmv_hip_free_on(z->ctx, d->d_ckpt);
	free(d->ckpt); free(d->ckpt_pos); free(d->recorded);
	dlz_close(z);
	agmv_hip_free_on(ctx, d->d_bits); agmv_hip_free_on(ctx, d->d_bpos); agmv_hip_free_on(ctx, d->d_nent);
	agmv_hip_free_on(ctx, d->d_out[0]); agmv_hip_free_on(ctx, d->d_out[1]); agmv_hip_free_on(ctx, d->d_iframe); agmv_hip_free_on(ctx, d->d_scaled);
	agmv_hip_free_on(ctx, d->d_table); agmv_hip_free_on(ctx, d->d_view); agmv_hip_free_on(ctx, d->d_deblock); agmv_hip_free_on(ctx, d->d_dbcounts);
	agmv_hip_stream_destroy(ctx, d->stream);
	free(d->slot); free(d->persist); free(d->chunks); free(d->jobs);
	pthread_mutex_destroy(&d->mu); pthread_cond_destroy(&d->cv);
}

/* Step: the one batch loop.  From where the LZ stage stands (d->pos, d->done) batch by batch -- LZ stage, then the hand-over to the worker -- until `upto` frames have been
   through the LZ stage, the file holds no further chunk, the worker has failed or (a reader) asks for the restart.  A batch wholly before g0 is not handed over and its
   slot is filled again; the batch that holds g0 is decoded from row g0 - first on.  Returns an Error. */
static int dpipe_run(dpipe* d, dlz* z, uint32_t upto)
{
	const int viewed = d->sink.viewed;
	while (d->done < upto) {
		dbatch* b = &d->slot[d->nfilled % d->nslots];      /* (nfilled is written by this thread alone) */
		const unsigned want = d->cap < upto - d->done ? d->cap : upto - d->done;
		unsigned n; int got, stop;
		pthread_mutex_lock(&d->mu);
		while (b->filled && !d->failed) pthread_cond_wait(&d->cv, &d->mu);   /* the slot's frames of batch id - nslots are all exported */
		stop = d->failed || d->restart;
		pthread_mutex_unlock(&d->mu);
		if (stop) break;
		got = d->plan.lz_dev ? dlz_batch(z, d, b, want) : host_lz_batch(d, b, want);
		if (got < 0) fprintf(stderr, "libagmv(amd): batch LZ stage: %s (the AGMV hot path runs on the GPU only -- no CPU fallback)\n", agmv_hip_last_error());
		if (got < 0) return MEMORY_CORRUPTION_ERR;
		if (got == 0) break;
		n = (unsigned)got;
		d->lz_frames += n;
		if (d->done + n <= d->g0) { d->done += n; continue; }      /* wholly before the view's GOP: the LZ stage was all it needed */
		b->skip = d->g0 > d->done ? d->g0 - d->done : 0;           /* (the batch that holds g0: from row g0 - done on) */
		b->n = n - b->skip; b->first = d->done + b->skip; b->name0 = *d->sink.count + 1;
		b->fresh = d->fresh; d->fresh = 0;
		if (!viewed) *d->sink.count += n;                          /* (a view's frames are counted where they are selected: sink_view) */
		pthread_mutex_lock(&d->mu);
		b->filled = 1; d->nfilled++;
		pthread_cond_broadcast(&d->cv);
		pthread_mutex_unlock(&d->mu);
		d->done += n;
	}
	return NO_ERR;
}

/* ... and the end of the worker and the pool, before dpipe_close: what was handed over is decoded, delivered and, for the BMP export, on disk */
static void dpipe_finish(dpipe* d)
{
	unsigned i;
	pthread_mutex_lock(&d->mu);
	d->closing = 1;
	pthread_cond_broadcast(&d->cv);
	pthread_mutex_unlock(&d->mu);
	pthread_join(d->th, NULL);
	pthread_mutex_lock(&d->mu);                            /* every frame that was decoded is on disk before the call returns */
	for (i = 0; i < d->nslots; i++) while (d->slot[i].decoded && !d->failed) pthread_cond_wait(&d->cv, &d->mu);
	pthread_mutex_unlock(&d->mu);
	agmv_pool_stop(d->pool);
}

/* The frame loop of AGMV_DecodeAGMV / AGMV_DecodeVideo on a file image, `pos` = first byte behind the header: open (dpipe_open), loop (dpipe_run), close (dpipe_finish, dpipe_close): the three steps a reader session (agmv_dreader, below) takes apart.  The LZ stage of a
   batch runs on the pool (host_lz_batch) or on the GPU (dlz_batch).  The frames go to `sink` (agmv_pipeline.h), whose count advances by the frames
   decoded; how they get there is the plan's matter (dplan_of).  A view (sink->viewed; nframes then ends behind the last frame it needs) runs its LZ
   stage from frame 0 like any other, because only that keeps the persistent buffer right; its GPU stage starts at the GOP start g0 from the fresh
   state: a batch wholly before g0 is not handed to the worker and its slot is filled again, the batch that holds g0 is decoded from row g0 - first
   on.  *restart = 1 (and NO_ERR) when the worker found that the first decoded batch derives from the state before it: nothing that run delivered
   counts, and the caller runs g0 = 0. */
static int decode_run(agmv_hip_ctx* ctx, const agmv_dfile* f, unsigned cap_frames, unsigned threads, const agmv_sink* sink, uint32_t g0, unsigned deblock,
                      AGMV_VIEW_STATS* stats, int* restart)
{
	const int viewed = sink->viewed;
	const uint32_t w = f->w, h = f->h;
	uint32_t done;
	dpipe d; dlz z;
	int rc = dpipe_open(&d, &z, ctx, f, cap_frames, threads, sink, g0, deblock) ? MEMORY_CORRUPTION_ERR : NO_ERR;
	if (rc != NO_ERR) { dpipe_close(&d, &z); return rc; }
	rc = dpipe_run(&d, &z, f->nframes);
	dpipe_finish(&d);
	done = d.done;
	if (d.restart) *restart = 1;
	else if (d.failed) rc = MEMORY_CORRUPTION_ERR;
	if (d.plan.lz_dev) TRACE("decode: LZ stage device, %u frames in %u batches, %.3f s\n", (unsigned)done, z.batches, z.secs);
	if (viewed) TRACE("decode: view from GOP start %u, %u frames through the LZ stage, %u through the GPU stage%s\n", (unsigned)g0, (unsigned)done, d.gpu_frames,
	                  d.restart ? ", which depend on the state before them: again from frame 0" : "");
	if (stats) { stats->lz_frames += done; stats->gpu_frames += d.gpu_frames; }
	if (deblock && rc == NO_ERR && !d.restart) {           /* (the worker synchronised its stream behind its last batch) */
		unsigned long long counts[2] = {0, 0};
		if (agmv_hip_memcpy_async(ctx, counts, d.d_dbcounts, sizeof(counts), 1, d.stream) || agmv_hip_stream_sync(ctx, d.stream)) rc = MEMORY_CORRUPTION_ERR;
		g_deblock_stats.strength = deblock; g_deblock_stats.frames = d.gpu_frames; g_deblock_stats.weak = counts[0]; g_deblock_stats.strong = counts[1];
		g_deblock_stats.lines = (unsigned long long)d.gpu_frames * ((unsigned long long)(w / 4 - 1) * h + (unsigned long long)(h / 4 - 1) * w);
		TRACE("decode: deblocking, strength %u: %u frames, %llu weak and %llu strong of %llu lines\n", deblock, g_deblock_stats.frames, counts[0], counts[1],
		      g_deblock_stats.lines);
	}
	dpipe_close(&d, &z);
	return rc;
}

/* decode_run, and for a view that starts inside the file and cannot be trusted from the fresh state the same call again from
   frame 0, which writes the same destinations.  *stats (may be NULL) receives what the run that delivered did. */
int agmv_decode_stream(agmv_hip_ctx* ctx, const u8* file, size_t len, size_t pos, uint32_t w, uint32_t h, uint32_t nframes, int ver,
                       int has_audio, unsigned cap_frames, unsigned threads, const agmv_sink* sink, AGMV_VIEW_STATS* stats)
{
	const agmv_dfile f = {file, len, pos, w, h, nframes, ver, has_audio};
	const unsigned long count0 = *sink->count;
	const unsigned deblock = agmv_deblock_strength();
	int restart = 0, rc;
	if (stats) memset(stats, 0, sizeof(*stats));
	memset(&g_deblock_stats, 0, sizeof(g_deblock_stats));
	if (deblock) TRACE("decode: deblocking of every batch in front of its sink, strength %u\n", deblock);
	rc = decode_run(ctx, &f, cap_frames, threads, sink, sink->viewed ? sink->view.first & ~3u : 0, deblock, stats, &restart);
	if (rc == NO_ERR && restart) {
		*sink->count = count0;
		if (stats) memset(stats, 0, sizeof(*stats));               /* (how far the LZ stage of the run given up had come is a matter of timing) */
		rc = decode_run(ctx, &f, cap_frames, threads, sink, 0, deblock, stats, &restart);
	}
	if (stats) { stats->restarts = (unsigned)restart; stats->delivered = rc == NO_ERR ? (unsigned)(*sink->count - count0) : 0; }
	return rc;
}

/* ------------------------------------------------------------------------------------------
 * reader sessions (include/agmv_reader.h): the pipe of decode_run, kept open between calls
 * ------------------------------------------------------------------------------------------ */
struct agmv_dreader {
	dpipe d; dlz z;
	uint32_t position, end;                /* the file frame the next read starts at; the frames the file is known to hold (the header's, fewer once a read found its end) */
	int moved, dead;                       /* a seek left the position somewhere else: the next read starts from a checkpoint; the GPU failed: every read fails */
	size_t index_bytes;
	unsigned long count;                   /* the frames the running read has delivered (the sink's count) */
	unsigned long long delivered; unsigned reads, seeks, restarts;
};

/* Open: dpipe_open, with the sink of a view of every frame, and the seek index, whose slots are all made here */
agmv_dreader* agmv_dreader_open(agmv_hip_ctx* ctx, const agmv_dfile* f, unsigned cap_frames, unsigned threads, const agmv_sink* sink, unsigned deblock, size_t index_bytes)
{
	agmv_dreader* r = (agmv_dreader*)calloc(1, sizeof(*r));
	agmv_sink s = *sink;
	dpipe* d;
	if (!r) return NULL;
	d = &r->d;
	s.viewed = 1; s.count = &r->count;                     /* (a view, whatever it selects: no read decodes into the caller's clip or takes a frame from it) */
	r->end = f->nframes; r->index_bytes = index_bytes;
	if (dpipe_open(d, &r->z, ctx, f, cap_frames, threads, &s, 0, deblock)) goto fail;
	d->keep = 1;                                           /* (the worker reads it behind its first batch at the earliest, which a read hands over) */
	agmv_reader_checkpoint(f->nframes, d->lz_cap, index_bytes, 0, NULL, &d->interval);
	d->nckpt = (f->nframes + d->interval - 1) / d->interval;
	if (d->nckpt < 1) d->nckpt = 1;
	d->recorded = (uint32_t*)calloc(d->nckpt / 32 + 1, 4); d->ckpt_pos = (size_t*)calloc(d->nckpt, sizeof(size_t));
	if (!d->recorded || !d->ckpt_pos) goto fail_open;
	d->recorded[0] = 1; d->ckpt_pos[0] = f->pos;
	if (d->nckpt > 1) {
		const size_t bytes = (size_t)(d->nckpt - 1) * d->lz_cap;
		if (d->plan.lz_dev ? !(d->d_ckpt = (uint8_t*)agmv_hip_malloc_on(r->z.ctx, bytes)) : !(d->ckpt = (u8*)malloc(bytes))) goto fail_open;
	}
	TRACE("reader: open, batches of %u frames, seek index of %u checkpoints every %u frames (%.1f MB, %s)\n", d->cap, (unsigned)d->nckpt - 1, (unsigned)d->interval,
	      (d->nckpt - 1) * (double)d->lz_cap / 1e6, d->plan.lz_dev ? "device" : "host");
	return r;
fail_open:
	dpipe_finish(d);
fail:
	dpipe_close(d, &r->z);
	free(r);
	return NULL;
}

/* the worker has released every batch handed over (or has failed) */
static void dreader_wait(dpipe* d)
{
	pthread_mutex_lock(&d->mu);
	while (d->ndone < d->nfilled && !d->failed) pthread_cond_wait(&d->cv, &d->mu);
	pthread_mutex_unlock(&d->mu);
}

/* The LZ stage to the greatest recorded checkpoint <= g0 -- its buffer, its place in the file -- and the GPU stage to start at g0 from the fresh state.  The worker is idle. */
static int dreader_start_at(agmv_dreader* r, uint32_t g0)
{
	dpipe* d = &r->d; dlz* z = &r->z;
	const uint32_t c = agmv_reader_checkpoint(d->f.nframes, d->lz_cap, r->index_bytes, g0, d->recorded, NULL), k = c / d->interval;
	if (d->plan.lz_dev) {
		if (k ? agmv_hip_memcpy_async(z->ctx, z->d_persist, d->d_ckpt + (size_t)(k - 1) * d->lz_cap, d->lz_cap, 2, z->stream)
		      : agmv_hip_memset_async(z->ctx, z->d_persist, 0, d->lz_cap, z->stream))
			return -1;
	} else if (k) memcpy(d->persist, d->ckpt + (size_t)(k - 1) * d->lz_cap, d->lz_cap);
	else memset(d->persist, 0, d->lz_cap);
	d->pos = d->ckpt_pos[k]; d->done = c; d->g0 = g0; d->fresh = 1;
	TRACE("reader: LZ stage from checkpoint %u, GPU stage from frame %u\n", (unsigned)c, (unsigned)g0);
	return 0;
}

int agmv_dreader_read(agmv_dreader* r, void* d_dst, uint32_t n)
{
	dpipe* d = &r->d;
	const AGMV_VIEW* v = &d->sink.view;
	const uint32_t p = r->position, len = agmv_view_length(p, v->step, n, r->end);
	uint32_t upto, g0 = p & ~3u;
	int rc;
	if (r->dead) return -MEMORY_CORRUPTION_ERR;
	r->reads++;
	if (!len) return 0;
	upto = p + (len - 1) * v->step + 1;                    /* behind the last frame the read needs */
	d->sink.view.first = p; d->sink.view.count = len;      /* (the worker is idle: it reads the sink behind the next hand-over) */
	if (d->sink.kind == AGMV_SINK_TENSOR) d->sink.tensor.d_dst = d_dst; else d->sink.frames.d_dst = d_dst;
	for (;;) {
		r->count = 0;
		rc = r->moved && dreader_start_at(r, g0) ? MEMORY_CORRUPTION_ERR : NO_ERR;
		r->moved = 0;
		if (rc == NO_ERR) rc = dpipe_run(d, &r->z, upto);
		dreader_wait(d);
		if (rc != NO_ERR || d->failed) { r->dead = 1; return -MEMORY_CORRUPTION_ERR; }
		if (!d->restart) break;
		/* the first batch from the fresh state derives from the state before it: the same read again, both stages from frame 0 */
		d->restart = 0; r->restarts++; r->moved = 1; g0 = 0;
	}
	if (r->count < len) r->end = d->done;                  /* the file holds no further chunk */
	r->delivered += r->count;
	r->position = p + (uint32_t)r->count * v->step;
	if (d->sink.kind == AGMV_SINK_TENSOR) d->sink.tensor.d_dst = NULL; else d->sink.frames.d_dst = NULL;      /* nothing of the caller's is held */
	return (int)r->count;
}

void agmv_dreader_seek(agmv_dreader* r, uint32_t frame)
{
	r->seeks++;
	if (frame == r->position) return;
	r->position = frame; r->moved = 1;
}

uint32_t agmv_dreader_tell(const agmv_dreader* r) { return r->position; }

void agmv_dreader_stats(const agmv_dreader* r, AGMV_READER_STATS* out)
{
	const AGMV_READER_STATS s = {r->d.lz_frames, r->d.gpu_frames, r->delivered, r->reads, r->seeks, r->restarts, r->d.checkpoints, r->d.interval};
	*out = s;
}

void agmv_dreader_close(agmv_dreader* r)
{
	dpipe_finish(&r->d);
	dpipe_close(&r->d, &r->z);
	free(r);
}
