/*
 * libagmv_amd/csrc/agmv_codec.c -- libagmv's encode/decode entry points on top of the GPU hot path.
 *
 *   per frame   AGMV_EncodeFrame (reference src/agmv_encode.c:529-634) and AGMV_DecodeFrameChunk
 *               (src/agmv_decode.c:145-410): same FILE* protocol, one frame per call through the
 *               batch C-ABI of include/agmv_hip.h with n_frames = 1.
 *   sequences   AGMV_EncodeAGMV / AGMV_EncodeFullAGMV / AGMV_EncodeVideo (src/agmv_encode.c:719-4407,
 *               BMP branch) and AGMV_DecodeAGMV / AGMV_DecodeVideo (src/agmv_decode.c:455-647): these
 *               own the loop, so frames go to the GPU in GOP-aligned batches while the host threads
 *               run the LZ stage and the container is written strictly in frame order.
 *
 * Everything on the hot path (quantise, block classification, byte assembly, parse, reconstruct,
 * PDIFS midpoint, palette histogram) runs on the GPU.  There is no CPU fallback: if the GPU path
 * fails these functions print the reason and abort (the void encoders have no error channel).
 */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "agmv_hip.h"
#include "agmv_internal.h"
#include "agmv_pipeline.h"
#include "agmv_writer.h"

/* ------------------------------------------------------------------------------------------ */
static agmv_hip_ctx* g_ctx = NULL;
static uint32_t g_pal[512];
static int g_pal_mode = -1;
static unsigned g_batch_frames = 0, g_lz_threads = 0, g_devices = 0, g_palette_refine = 0, g_dither = 0, g_stabilise = 0, g_deblock = 0;
/* the device track AGMV_SetAudioDev attached to the next AGMV_EncodeFrames*Dev call (d_pcm NULL: none) */
static struct { const void* d_pcm; int fmt; u32 samples, rate; u16 channels; } g_audio;
static unsigned long g_export_count = 0;            /* AGIDL's expcount, extern/agidl/src/agidl_img_export.c:18 */

void agmv_die(const char* what)
{
	fprintf(stderr, "libagmv(amd): %s: %s\n", what, agmv_hip_last_error());
	fprintf(stderr, "libagmv(amd): the AGMV hot path runs on the GPU only (no CPU fallback) -- aborting\n");
	abort();
}

/* the decoders have an error channel (enum Error): a GPU failure is reported on stderr AND returned, never papered over */
static int gpu_failed(const char* what)
{
	fprintf(stderr, "libagmv(amd): %s: %s (the AGMV hot path runs on the GPU only -- no CPU fallback)\n", what, agmv_hip_last_error());
	return MEMORY_CORRUPTION_ERR;
}

static int bad_geometry(uint32_t w, uint32_t h)
{
	return w == 0 || h == 0 || (w & 3u) || (h & 3u) || (unsigned long long)w * h > (1ull << 28);
}

void AGMV_SetBatchFrames(unsigned n) { g_batch_frames = n; }
void AGMV_SetLZThreads(unsigned n) { g_lz_threads = n; }
void AGMV_SetDevices(unsigned n) { g_devices = n; }
void AGMV_SetPaletteRefine(unsigned n) { g_palette_refine = n; }
void AGMV_SetDither(unsigned n) { g_dither = n; }
void AGMV_SetStabilise(unsigned n) { g_stabilise = n; }
void AGMV_SetDeblock(unsigned n) { g_deblock = n; }

/* frames per GPU batch: what the caller asked for, else about 128 MB of source pixels (64 frames at most), whole GOPs */
static unsigned batch_frames(size_t npx)
{
	unsigned n = g_batch_frames;
	const char* e = getenv("AGMV_BATCH_FRAMES");
	if (!n && e) n = (unsigned)atoi(e);
	if (!n) {
		size_t f = ((size_t)128 << 20) / (npx ? npx * 4 : 4);
		n = f < 8 ? 8 : (f > 64 ? 64 : (unsigned)f);
	}
	return (n + 3u) & ~3u;
}

/* GPUs the sequence encoders spread their batches over (AGMV_SetDevices / env AGMV_DEVICES; default 1) */
static unsigned devices(void)
{
	unsigned n = g_devices;
	const char* e = getenv("AGMV_DEVICES");
	if (!n && e) n = (unsigned)atoi(e);
	return n ? n : 1;
}

/* rounds of the palette refinement the sequence encoders run (AGMV_SetPaletteRefine / env AGMV_PALETTE_REFINE; default 0 = off) */
static unsigned palette_refine(void)
{
	unsigned n = g_palette_refine;
	const char* e = getenv("AGMV_PALETTE_REFINE");
	if (!n && e && atoi(e) > 0) n = (unsigned)atoi(e);
	return n > 64 ? 64 : n;
}

/* strength of the pattern dithering a sequence opened now runs before its encodes (AGMV_SetDither / env AGMV_DITHER, 1 .. 64;
   default 0 = off); agmv_seq_open reads it */
unsigned agmv_dither_strength(void)
{
	const char* e = getenv("AGMV_DITHER");
	if (g_dither) return g_dither > 64 ? 64 : g_dither;
	return e && atoi(e) >= 1 && atoi(e) <= 64 ? (unsigned)atoi(e) : 0;
}

/* strength of the temporal stabilisation a sequence opened now runs before its encodes (AGMV_SetStabilise / env AGMV_STABILISE,
   1 .. 64; default 0 = off); agmv_seq_open reads it */
unsigned agmv_stabilise_strength(void)
{
	const char* e = getenv("AGMV_STABILISE");
	if (g_stabilise) return g_stabilise > 64 ? 64 : g_stabilise;
	return e && atoi(e) >= 1 && atoi(e) <= 64 ? (unsigned)atoi(e) : 0;
}

/* strength of the deblocking a sequence decode opened now runs between reconstruction and its sink (AGMV_SetDeblock / env
   AGMV_DEBLOCK, 1 .. 64; default 0 = off); agmv_decode_stream reads it */
unsigned agmv_deblock_strength(void)
{
	const char* e = getenv("AGMV_DEBLOCK");
	char* end;
	unsigned long v;
	if (g_deblock) return g_deblock > 64 ? 64 : g_deblock;
	if (!e || *e < '0' || *e > '9') return 0;                  /* (no sign, no leading blank: a decimal number and nothing else) */
	v = strtoul(e, &end, 10);
	return *end == 0 && v >= 1 && v <= 64 ? (unsigned)v : 0;
}

/* host threads of the pipelines (BMP parse, LZ, BMP export): what the caller asked for, else the cores this process may
   use -- the online count, cut to the cgroup's CPU quota where there is one (a container's share of a big host) */
static unsigned lz_threads(void)
{
	unsigned n = g_lz_threads;
	const char* e = getenv("AGMV_LZ_THREADS");
	if (!n && e) n = (unsigned)atoi(e);
	if (!n) {
		long c = sysconf(_SC_NPROCESSORS_ONLN);
		FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r");
		n = c > 0 ? (unsigned)c : 1;
		if (f) {
			long long quota = 0, period = 0;
			if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) {
				unsigned q = (unsigned)((quota + period - 1) / period);
				if (q >= 1 && q < n) n = q;
			}
			fclose(f);
		}
	}
	return n > 64 ? 64 : n;
}

/* the library's context, opened on first use: NULL where the device cannot be opened, for the callers with an error channel
   (the decoders, gpu_failed); ctx() is for the others, which abort */
static agmv_hip_ctx* open_ctx(void)
{
	const char* e = getenv("AGMV_DEVICE");
	if (!g_ctx) g_ctx = agmv_hip_create(e ? atoi(e) : 0);
	return g_ctx;
}

static agmv_hip_ctx* ctx(void)
{
	if (!open_ctx()) agmv_die("cannot open the GPU");
	return g_ctx;
}

static int mode512_of(AGMV_OPT opt) { return opt != AGMV_OPT_II && opt != AGMV_OPT_ANIM && opt != AGMV_OPT_GBA_II; }

/* (re)build the exact LUT when the palette of the object differs from the one on the device */
static void use_palette(const u32* p0, const u32* p1, int mode512)
{
	uint32_t pal[512];
	int i;
	for (i = 0; i < 256; i++) { pal[i] = (uint32_t)p0[i]; pal[256 + i] = mode512 ? (uint32_t)p1[i] : 0; }
	if (g_pal_mode == mode512 && memcmp(pal, g_pal, sizeof(pal)) == 0) { ctx(); return; }
	if (agmv_hip_set_palette(ctx(), pal, pal + 256, mode512, NULL)) agmv_die("palette upload");
	memcpy(g_pal, pal, sizeof(pal));
	g_pal_mode = mode512;
}

/* ------------------------------------------------------------------------------------------
 * container pieces
 * ------------------------------------------------------------------------------------------ */
/* header, reference src/agmv_encode.c:21-94 (palette1 only in the 512-colour versions) */
void AGMV_EncodeHeader(FILE* f, AGMV* a)
{
	AGMV_OPT opt = AGMV_GetOPT(a);
	int pals = mode512_of(opt) ? 2 : 1, p, i;
	AGMV_WriteFourCC(f, 'A', 'G', 'M', 'V');
	AGMV_WriteLong(f, AGMV_GetNumberOfFrames(a));
	AGMV_WriteLong(f, AGMV_GetWidth(a));
	AGMV_WriteLong(f, AGMV_GetHeight(a));
	AGMV_WriteByte(f, 1);
	AGMV_WriteByte(f, AGMV_GetVersionFromOPT(opt, AGMV_GetCompression(a)));
	AGMV_WriteLong(f, AGMV_GetFramesPerSecond(a));
	AGMV_WriteLong(f, AGMV_GetTotalAudioDuration(a));
	AGMV_WriteLong(f, AGMV_GetSampleRate(a));
	AGMV_WriteLong(f, AGMV_GetAudioSize(a));
	AGMV_WriteShort(f, AGMV_GetNumberOfChannels(a));
	AGMV_WriteShort(f, AGMV_GetBitsPerSample(a));
	for (p = 0; p < pals; p++)
		for (i = 0; i < 256; i++) {
			u32 c = p ? a->header.palette1[i] : a->header.palette0[i];
			AGMV_WriteByte(f, AGMV_GetR(c)); AGMV_WriteByte(f, AGMV_GetG(c)); AGMV_WriteByte(f, AGMV_GetB(c));
		}
}

/* reference src/agmv_decode.c:91-143 */
int AGMV_DecodeHeader(FILE* f, AGMV* a)
{
	int pals, p, i;
	AGMV_ReadFourCC(f, a->header.fourcc);
	a->header.num_of_frames = AGMV_ReadLong(f);
	a->header.width = AGMV_ReadLong(f);
	a->header.height = AGMV_ReadLong(f);
	a->header.fmt = AGMV_ReadByte(f);
	a->header.version = AGMV_ReadByte(f);
	a->header.frames_per_second = AGMV_ReadLong(f);
	a->header.total_audio_duration = AGMV_ReadLong(f);
	a->header.sample_rate = AGMV_ReadLong(f);
	a->header.audio_size = AGMV_ReadLong(f);
	a->header.num_of_channels = AGMV_ReadShort(f);
	a->header.bits_per_sample = AGMV_ReadShort(f);
	if (!AGMV_IsCorrectFourCC(a->header.fourcc, 'A', 'G', 'M', 'V') || a->header.version < 1 || a->header.version > 4 ||
	    a->header.frames_per_second >= 200 || !(a->header.bits_per_sample == 16 || a->header.bits_per_sample == 8))
		return INVALID_HEADER_FORMATTING_ERR;
	pals = (a->header.version == 1 || a->header.version == 3) ? 2 : 1;
	for (p = 0; p < pals; p++)
		for (i = 0; i < 256; i++) {
			u32 r = AGMV_ReadByte(f), g = AGMV_ReadByte(f), b = AGMV_ReadByte(f);
			/* AGIDL_RGB(r,g,b,fmt): the encoder always writes fmt 1 = RGB_888; 2 = BGR_888 */
			u32 c = a->header.fmt == 2 ? (b << 16 | g << 8 | r) : (r << 16 | g << 8 | b);
			if (p) a->header.palette1[i] = c; else a->header.palette0[i] = c;
		}
	return NO_ERR;
}

/* chunk framing around an already compressed payload, reference src/agmv_encode.c:549-550,
   567-585, 622-624: 'AGFC', frame number, usize, csize, csize payload bytes, 8 x 0xFF.
   (the reference writes the flushed partial byte and then overwrites it with the first 0xFF) */
void agmv_write_frame_chunk(FILE* f, u32 frame_no, u32 usize, u32 csize, const u8* payload)
{
	static const u8 guard[8] = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
	AGMV_WriteFourCC(f, 'A', 'G', 'F', 'C');
	AGMV_WriteLong(f, frame_no);
	AGMV_WriteLong(f, usize);
	AGMV_WriteLong(f, csize);
	fwrite(payload, 1, csize, f);
	fwrite(guard, 1, 8, f);
}

/* ------------------------------------------------------------------------------------------
 * per-frame entry points
 * ------------------------------------------------------------------------------------------ */
void AGMV_EncodeFrame(FILE* file, AGMV* a, u32* img_data)
{
	const uint32_t w = (uint32_t)AGMV_GetWidth(a), h = (uint32_t)AGMV_GetHeight(a);
	const size_t npx = (size_t)w * h, stride = agmv_hip_max_usize(w, h, 1);
	const int m512 = mode512_of(AGMV_GetOPT(a));
	const int is_i = a->frame_count % 4 == 0;
	uint32_t* pix = (uint32_t*)malloc(npx * 4);
	uint16_t* ient = (uint16_t*)malloc(npx * 2);
	u8* bytes = (u8*)malloc(stride);
	u8* comp;
	uint32_t usize = 0;
	u32 csize;
	size_t i;

	use_palette(a->header.palette0, a->header.palette1, m512);
	for (i = 0; i < npx; i++) pix[i] = (uint32_t)img_data[i];          /* LP64: 8 -> 4 bytes per pixel */
	for (i = 0; i < npx; i++) ient[i] = (uint16_t)(a->iframe_entries[i].pal_num << 8 | a->iframe_entries[i].index);
	if (agmv_hip_encode_frames(ctx(), pix, 1, w, h, (uint32_t)a->frame_count, bytes, stride, &usize, ient))
		agmv_die("AGMV_EncodeFrame");

	AGMV_SyncFrameAndImage(a, img_data);                               /* :548 */
	if ((size_t)usize > a->bitstream->len) {                           /* objects built by foreign code: w*h*2 */
		a->bitstream->data = (u8*)realloc(a->bitstream->data, usize + 64);
		a->bitstream->len = usize + 64;
	}
	memcpy(a->bitstream->data, bytes, usize);
	a->bitstream->pos = usize;

	comp = (u8*)malloc((size_t)usize * 4 + 64);
	/* LZ77 peeks one byte past the stream (:222): hand it the byte the persistent buffer holds there */
	csize = AGMV_GetCompression(a) == AGMV_LZSS_COMPRESSION ? agmv_lzss_mem(a->bitstream->data, usize, comp)
	                                                        : agmv_lz77_mem(a->bitstream->data, usize, comp);
	agmv_write_frame_chunk(file, a->frame_count + 1, usize, csize, comp);

	if (is_i)                                                          /* :626-630 */
		for (i = 0; i < npx; i++) { a->iframe_entries[i].pal_num = (u8)(ient[i] >> 8); a->iframe_entries[i].index = (u8)ient[i]; }
	a->frame_count++;
	free(comp); free(bytes); free(ient); free(pix);
}

int AGMV_DecodeFrameChunk(FILE* file, AGMV* a)
{
	const uint32_t w = (uint32_t)a->frame->width, h = (uint32_t)a->frame->height;
	const size_t npx = (size_t)w * h;
	const int ver = a->header.version, m512 = (ver == 1 || ver == 3);
	uint32_t bpos = 0, *prev, *prev_i, *out;
	size_t i, cap, stride;
	u8* slab;

	if (bad_geometry(w, h)) return INVALID_HEADER_FORMATTING_ERR;      /* the block loops need multiples of 4 (src/agmv_decode.c:226-227) */
	a->bitstream->pos = 0;
	AGMV_ReadFourCC(file, a->frame_chunk->fourcc);
	a->frame_chunk->frame_num = AGMV_ReadLong(file);
	a->frame_chunk->uncompressed_size = AGMV_ReadLong(file);
	a->frame_chunk->compressed_size = AGMV_ReadLong(file);
	if (!AGMV_IsCorrectFourCC(a->frame_chunk->fourcc, 'A', 'G', 'F', 'C')) return INVALID_HEADER_FORMATTING_ERR;

	/* D1: LZ stage on the host straight from the FILE*, same bit reader protocol as the reference
	   (src/agmv_decode.c:171-222) so the file position ends where the reference's does */
	cap = a->bitstream->len;
	{
		u8* data = a->bitstream->data;
		const u32 usize = a->frame_chunk->uncompressed_size, csize = a->frame_chunk->compressed_size;
		unsigned long long bp = 0, lim = cap > 16 ? cap - 16 : 0;
		if (ver == 1 || ver == 2) {
			unsigned long long nbits = (unsigned long long)csize * 8, bits = 0;
			while (bits < nbits && bp < usize && bp < lim) {
				u32 flag = AGMV_ReadBits(file, 1);
				bits++;
				if (flag & 1) { data[bp++] = (u8)AGMV_ReadBits(file, 8); bits += 8; }
				else {
					u32 offset = AGMV_ReadBits(file, 16), len = AGMV_ReadBits(file, 4), k;
					unsigned long long pos = bp;
					bits += 20;
					for (k = 0; k < len; k++) {
						unsigned long long src = pos - offset + k;
						if (src < bp && bp < lim) data[bp++] = data[src];
					}
				}
			}
		} else {
			u32 t;
			for (t = 0; t < csize; t += 4) {
				u32 offset = AGMV_ReadShort(file), len = AGMV_ReadByte(file), k;
				u8 byte = AGMV_ReadByte(file);
				unsigned long long pos = bp;
				for (k = 0; k < len; k++) {
					unsigned long long src = pos - offset + k;
					if (src < bp && bp < lim) data[bp++] = data[src];
				}
				if (bp < lim) data[bp++] = byte;
			}
		}
		bpos = (uint32_t)bp;
	}
	a->bitstream->pos = bpos;
	AGMV_FlushReadBits();

	/* D2-D4 on the GPU: parse + reconstruct one frame on top of img_data / iframe */
	use_palette(a->header.palette0, a->header.palette1, m512);
	stride = ((size_t)bpos + 16 + 255) & ~(size_t)255;
	slab = (u8*)calloc(stride, 1);
	prev = (uint32_t*)malloc(npx * 4); prev_i = (uint32_t*)malloc(npx * 4); out = (uint32_t*)malloc(npx * 4);
	if (!slab || !prev || !prev_i || !out) { free(slab); free(prev); free(prev_i); free(out); return MEMORY_CORRUPTION_ERR; }
	memcpy(slab, a->bitstream->data, (size_t)bpos + 16 <= cap ? (size_t)bpos + 16 : cap);   /* incl. the stale bytes */
	for (i = 0; i < npx; i++) { prev[i] = (uint32_t)a->frame->img_data[i]; prev_i[i] = (uint32_t)a->iframe->img_data[i]; }
	if (agmv_hip_decode_frames(ctx(), slab, stride, &bpos, 1, w, h, (uint32_t)a->frame_count, out, prev, prev_i)) {
		free(slab); free(prev); free(prev_i); free(out);
		return gpu_failed("AGMV_DecodeFrameChunk");
	}
	for (i = 0; i < npx; i++) a->frame->img_data[i] = out[i];
	if (a->frame_count % 4 == 0) memcpy(a->iframe->img_data, a->frame->img_data, npx * sizeof(u32));   /* :401-405 */
	a->frame_count++;
	free(slab); free(prev); free(prev_i); free(out);
	return NO_ERR;
}

/* ------------------------------------------------------------------------------------------
 * helper entry points of the reference API that work on host AGMV_ENTRY planes.  They are steps
 * of AGMV_EncodeFrame; kept exported for source compatibility and routed through the same GPU
 * tables (exact LUT / bit matrix) so no second implementation of the hot path exists.
 * ------------------------------------------------------------------------------------------ */
static uint16_t gpu_entry_of(const u32* p0, const u32* p1, int m512, u32 color)
{
	/* the reference's own search, run on the GPU against the caller's palettes (no table is built for a single
	   colour; the device scratch lives in the context): src/agmv_utils.c:785-816, :851-895 */
	uint32_t pal[512], px = (uint32_t)color;
	uint16_t e = 0;
	int i;
	for (i = 0; i < 256; i++) { pal[i] = (uint32_t)p0[i]; pal[256 + i] = m512 ? (uint32_t)p1[i] : 0; }
	if (agmv_hip_nearest(ctx(), pal, pal + 256, m512, &px, 1, &e)) agmv_die("nearest entry");
	return e;
}

u8 AGMV_FindNearestColor(u32 palette[256], u32 color) { return (u8)gpu_entry_of(palette, palette, 0, color); }

AGMV_ENTRY AGMV_FindNearestEntry(u32 palette0[256], u32 palette1[256], u32 color)
{
	uint16_t e = gpu_entry_of(palette0, palette1, 1, color);
	AGMV_ENTRY r;
	memset(&r, 0, sizeof(r));
	r.pal_num = (u8)(e >> 8); r.index = (u8)e;
	return r;
}

static u32 entry_colour(AGMV* a, const AGMV_ENTRY* e) { return e->pal_num ? a->header.palette1[e->index] : a->header.palette0[e->index]; }

/* the two block predicates (reference src/agmv_encode.c:302-352, :240-300): the 16 palette colours of the block and the
   16 colours they are compared with go to the GPU, which counts the pairs within +-2 on every channel */
static u8 count_within2(const uint32_t* a, const uint32_t* b)
{
	int n = agmv_hip_within2_count(ctx(), a, b);
	if (n < 0) agmv_die("block compare");
	return (u8)n;
}

u8 AGMV_CompareIFrameBlock(AGMV* a, u32 x, u32 y, u32 color, AGMV_ENTRY* e)
{
	u32 w = a->frame->width, i, j;
	uint32_t ca[16], cb[16];
	for (j = 0; j < 4; j++) for (i = 0; i < 4; i++) { ca[j * 4 + i] = (uint32_t)entry_colour(a, &e[(x + i) + (y + j) * w]); cb[j * 4 + i] = (uint32_t)color; }
	return count_within2(ca, cb);
}

u8 AGMV_ComparePFrameBlock(AGMV* a, u32 x, u32 y, AGMV_ENTRY* e)
{
	u32 w = a->frame->width, i, j;
	uint32_t ca[16], cb[16];
	for (j = 0; j < 4; j++)
		for (i = 0; i < 4; i++) {
			size_t k = (x + i) + (size_t)(y + j) * w;
			ca[j * 4 + i] = (uint32_t)entry_colour(a, &e[k]);
			cb[j * 4 + i] = (uint32_t)entry_colour(a, &a->iframe_entries[k]);
		}
	return count_within2(ca, cb);
}

/* entries -> bitstream on the GPU: the entry plane goes to the encoder AS ENTRIES (agmv_hip_encode_entries: no
   quantisation), so classification and codes are exactly those of the given plane -- also for palettes with duplicate
   colours, where re-quantising an entry's colour would return the first of the duplicates
   (reference src/agmv_encode.c:354-436, :438-527; bytes are appended at bitstream->pos like the reference does) */
static void assemble_via_gpu(AGMV* a, AGMV_ENTRY* e, int iframe)
{
	const uint32_t w = (uint32_t)a->frame->width, h = (uint32_t)a->frame->height;
	const int m512 = mode512_of(AGMV_GetOPT(a));
	const size_t npx = (size_t)w * h, stride = agmv_hip_max_usize(w, h, 1);
	uint32_t* ent = (uint32_t*)malloc(npx * 4), usize = 0;
	uint16_t* ient = (uint16_t*)malloc(npx * 2);
	u8* bytes = (u8*)malloc(stride);
	size_t i;
	use_palette(a->header.palette0, a->header.palette1, m512);
	for (i = 0; i < npx; i++) {
		ent[i] = m512 ? (uint32_t)((e[i].pal_num & 1u) << 8 | e[i].index) : (uint32_t)e[i].index;
		ient[i] = (uint16_t)((a->iframe_entries[i].pal_num & 1u) << 8 | a->iframe_entries[i].index);
	}
	if (agmv_hip_encode_entries(ctx(), ent, 1, w, h, iframe ? 0u : 1u, bytes, stride, &usize, ient)) agmv_die("AGMV_Assemble*FrameBitstream");
	if ((size_t)a->bitstream->pos + usize > a->bitstream->len) {
		a->bitstream->len = a->bitstream->pos + usize + 64;
		a->bitstream->data = (u8*)realloc(a->bitstream->data, a->bitstream->len);
	}
	memcpy(a->bitstream->data + a->bitstream->pos, bytes, usize);
	a->bitstream->pos += usize;
	free(ent); free(ient); free(bytes);
}

void AGMV_AssembleIFrameBitstream(AGMV* a, AGMV_ENTRY* e) { assemble_via_gpu(a, e, 1); }
void AGMV_AssemblePFrameBitstream(AGMV* a, AGMV_ENTRY* e) { assemble_via_gpu(a, e, 0); }

/* ------------------------------------------------------------------------------------------
 * sequence encoders: the drivers decide WHICH frames are encoded (PDIFS schedules, frame skipping), the pipelined engine
 * of agmv_pipeline.c loads, encodes, compresses and writes them
 * ------------------------------------------------------------------------------------------ */
static int is_gba(AGMV_OPT o) { return o == AGMV_OPT_GBA_I || o == AGMV_OPT_GBA_II || o == AGMV_OPT_GBA_III; }

/* the size the GBA / NDS opts scale every source frame to (0: the opt encodes the frames as they are) */
static void scaled_size(AGMV_OPT opt, int* sw, int* sh)
{
	*sw = *sh = 0;
	if (is_gba(opt)) { *sw = AGMV_GBA_W; *sh = AGMV_GBA_H; }
	if (opt == AGMV_OPT_NDS) { *sw = AGMV_NDS_W; *sh = AGMV_NDS_H; }
}

static agmv_seq* seq_open(AGMV* a, FILE* file, const agmv_source* src, AGMV_OPT opt, int audio_chunks, int use_interp)
{
	uint32_t pal[512];
	agmv_seq_opts o = {.mode512 = mode512_of(opt), .lz77 = AGMV_GetCompression(a) != AGMV_LZSS_COMPRESSION, .audio_chunks = audio_chunks, .use_interp = use_interp,
	                   .cap = batch_frames((size_t)AGMV_GetWidth(a) * AGMV_GetHeight(a)), .devices = devices(), .threads = lz_threads(), .pal = pal};
	int i;
	if (!src->ring_frames) scaled_size(opt, &o.scale_w, &o.scale_h);      /* (a writer's ring holds the frames at the encode size) */
	for (i = 0; i < 256; i++) { pal[i] = (uint32_t)a->header.palette0[i]; pal[256 + i] = o.mode512 ? (uint32_t)a->header.palette1[i] : 0; }
	if (!file) o.pal = NULL;                                  /* a writer session: palette and file follow (seq_start) */
	return agmv_seq_open(a, file, src, &o);
}

/* ... for a sequence opened without a file: the object's palette, as seq_open reads it, and the file */
static void seq_start(agmv_seq* s, AGMV* a, FILE* file, AGMV_OPT opt)
{
	uint32_t pal[512];
	const int m512 = mode512_of(opt);
	int i;
	for (i = 0; i < 256; i++) { pal[i] = (uint32_t)a->header.palette0[i]; pal[256 + i] = m512 ? (uint32_t)a->header.palette1[i] : 0; }
	agmv_seq_start(s, file, pal, m512);
}

/* AGMV_BuildPalette with the picked colours moved by weighted k-means on the GPU between the pick and the slot map
   (include/agmv.h, "palette refinement").  The 512-colour opts pin centroid 511 at black: the slot map drops pick 511, and
   palette0[126], which it never fills, is the black the encoder can choose. */
int AGMV_BuildPaletteRefined(const unsigned* hist, AGMV_QUALITY quality, AGMV_OPT opt, u32 pal0[256], u32 pal1[256], unsigned iterations,
                             unsigned long long sse[2])
{
	u32 pal[512];
	uint32_t clr[512], rounds = 0, *d_hist, *d_pal, *d_rounds;
	uint64_t e[2] = { 0, 0 }, *d_sse;
	const uint32_t k = mode512_of(opt) ? 512 : 256, n_free = mode512_of(opt) ? 511 : 256;
	struct timespec t0, t1;
	agmv_hip_ctx* c;
	u32 n;
	if (!hist || !pal0 || !pal1 || opt < AGMV_OPT_I || opt > AGMV_OPT_NDS || quality < AGMV_HIGH_QUALITY || quality > AGMV_LOW_QUALITY) return -1;
	if (iterations == 0) {
		AGMV_BuildPalette(hist, quality, opt, pal0, pal1);
		return 0;
	}
	clock_gettime(CLOCK_MONOTONIC, &t0);
	agmv_palette_pick(hist, quality, pal);
	for (n = 0; n < 512; n++) clr[n] = (uint32_t)AGMV_ReverseQuantizeColor(pal[n], quality);
	if (k == 512) clr[511] = 0;
	c = ctx();
	d_hist = (uint32_t*)agmv_hip_malloc_on(c, 4u << 19); d_pal = (uint32_t*)agmv_hip_malloc_on(c, 4 * 512);
	d_rounds = (uint32_t*)agmv_hip_malloc_on(c, 4); d_sse = (uint64_t*)agmv_hip_malloc_on(c, 16);
	if (!d_hist || !d_pal || !d_rounds || !d_sse) agmv_die("device allocation for the palette refinement");
	if (agmv_hip_memcpy_async(c, d_hist, hist, 4u << 19, 0, NULL) || agmv_hip_memcpy_async(c, d_pal, clr, 4 * k, 0, NULL) ||
	    agmv_hip_palette_refine_dev(c, d_hist, (int)quality, d_pal, k, n_free, iterations, d_rounds, d_sse, NULL) ||
	    agmv_hip_memcpy_async(c, clr, d_pal, 4 * k, 1, NULL) || agmv_hip_memcpy_async(c, &rounds, d_rounds, 4, 1, NULL) ||
	    agmv_hip_memcpy_async(c, e, d_sse, 16, 1, NULL) || agmv_hip_stream_sync(c, NULL))
		agmv_die("palette refinement");
	agmv_hip_free_on(c, d_hist); agmv_hip_free_on(c, d_pal); agmv_hip_free_on(c, d_rounds); agmv_hip_free_on(c, d_sse);
	for (n = 0; n < 512; n++) pal[n] = n < k ? (u32)clr[n] : 0;
	agmv_palette_slots(pal, opt, pal0, pal1);
	if (sse) { sse[0] = e[0]; sse[1] = e[1]; }
	clock_gettime(CLOCK_MONOTONIC, &t1);
	if (getenv("AGMV_TRACE"))
		fprintf(stderr, "agmv trace: palette refinement: %u colours, %u of %u rounds moved a colour, distortion %llu -> %llu, %.3f s with the pick\n", (unsigned)k,
		        (unsigned)rounds, iterations, (unsigned long long)e[0], (unsigned long long)e[1], (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
	return 0;
}

/* Histogram -> palette -> header, the step the sequence encoders and a writer session share: the pick on the host, `refine` rounds of the
   refinement (0: none) on the GPU, then the file created with the header that carries the palette.  Aborts where the file cannot be created. */
static FILE* create_with_palette(AGMV* a, const char* filename, const uint32_t* hist, AGMV_QUALITY quality, AGMV_OPT opt, unsigned refine)
{
	u32 p0[256], p1[256];
	FILE* file;
	if (AGMV_BuildPaletteRefined(hist, quality, opt, p0, p1, refine, NULL)) agmv_die("internal: palette build refused its arguments");
	file = fopen(filename, "wb");
	if (!file) { fprintf(stderr, "libagmv(amd): cannot create %s\n", filename); abort(); }
	AGMV_SetICP0(a, p0);
	AGMV_SetICP1(a, p1);
	AGMV_EncodeHeader(file, a);
	return file;
}

/* the frame span a PDIFS file's rate and audio chunks are formed from (reference src/agmv_encode.c:2296-2353): integer halves for the heavy
   modes, x0.75 in double (float for GBA_III) for the light ones */
static int heavy_pdifs(AGMV_OPT o) { return o == AGMV_OPT_I || o == AGMV_OPT_ANIM || o == AGMV_OPT_GBA_I || o == AGMV_OPT_GBA_II; }

static u32 pdifs_adjusted(AGMV_OPT opt, u32 span)
{
	if (heavy_pdifs(opt)) return span / 2;
	return opt == AGMV_OPT_GBA_III ? (u32)(span * 0.75f) : (u32)(span * 0.75);
}

/* the header fields that depend on what was written, patched behind the last chunk (:3615-3620, :2225-2231): the frame count at
   offset 4 and the frames per second, times `rate`, at offset 18 */
static void patch_header(FILE* file, AGMV* a, u32 written, f32 rate)
{
	fseek(file, 4, SEEK_SET);
	AGMV_WriteLong(file, written);
	fseek(file, 18, SEEK_SET);
	AGMV_WriteLong(file, (u32)round(AGMV_GetFramesPerSecond(a) * rate));
}

static void dump_gba_header(const char* filename)
{
	/* reference src/agmv_encode.c:3627-3656: the finished file as a C array in GBA_GEN_AGMV.h (CWD) */
	FILE *in = fopen(filename, "rb"), *out;
	long n, i;
	u8* data;
	if (!in) return;
	fseek(in, 0, SEEK_END); n = ftell(in); fseek(in, 0, SEEK_SET);
	data = (u8*)malloc((size_t)n);
	if (fread(data, 1, (size_t)n, in) != (size_t)n) { /* short read: dump what we have */ }
	fclose(in);
	out = fopen("GBA_GEN_AGMV.h", "w");
	fprintf(out, "#ifndef GBA_GEN_AGMV_H\n#define GBA_GEN_AGMV_H\n\nconst unsigned char GBA_AGMV_FILE[%ld] = {\n", n);
	for (i = 0; i < n; i++) {
		if (i != 0 && i % 4000 == 0) fprintf(out, "\n");
		fprintf(out, "%d,", data[i]);
	}
	fprintf(out, "};\n\n#endif");
	fclose(out);
	free(data);
}

static void require_bmp(u8 img_type)
{
	if (img_type != AGMV_IMG_BMP) {
		fprintf(stderr, "libagmv(amd): only AGMV_IMG_BMP input is supported by this build (image type %u is out of scope)\n", img_type);
		abort();
	}
}

/* "is the pair of source frames (x, x + 1) similar", the decision behind AGMV_EncodeVideo's frame skipping: the grey-equality
   ratio of the two frames as the encoder sees them against the leniency (reference src/agmv_encode.c:744-790, :920-947).
   The two sources differ only in where the count comes from. */
typedef struct similarity {
	f32 leniency;
	uint32_t w, h;                         /* of the frames the encoder sees */
	/* BMP source: the two frames are loaded and compared on the calling thread, per decision */
	const agmv_source* src;
	int scale_w, scale_h;
	u32 *fa, *fb;
	uint32_t* tmp;
	/* device source: counts[x - first] of every adjacent pair, from one agmv_hip_similarity_dev launch over the clip */
	uint32_t* counts;
} similarity;

static void similarity_open(similarity* m, const agmv_source* src, AGMV* a, AGMV_OPT opt)
{
	const size_t npx = (size_t)AGMV_GetWidth(a) * AGMV_GetHeight(a);
	memset(m, 0, sizeof(*m));
	m->leniency = AGMV_GetLeniency(a); m->src = src; m->w = (uint32_t)AGMV_GetWidth(a); m->h = (uint32_t)AGMV_GetHeight(a);
	scaled_size(opt, &m->scale_w, &m->scale_h);
	if (!src->d_frames) {
		m->fa = (u32*)malloc(npx * sizeof(u32)); m->fb = (u32*)malloc(npx * sizeof(u32)); m->tmp = (uint32_t*)malloc(npx * 4);
		return;
	}
	{	/* the whole clip at once; with a scale, of the scaled frames (the same gather the workers run) */
		agmv_hip_ctx* c = ctx();
		const uint32_t n = src->n_frames;
		uint32_t *d_scaled = NULL, *d_index = NULL, *index = NULL, *d_counts = (uint32_t*)agmv_hip_malloc_on(c, 4 * (size_t)n);
		m->counts = (uint32_t*)calloc(n, 4);
		if (!d_counts || !m->counts) agmv_die("device allocation");
		if (m->scale_w) {
			d_index = agmv_source_index_dev(c, NULL, src, m->scale_w, m->scale_h, m->w, m->h, &index);
			d_scaled = (uint32_t*)agmv_hip_malloc_on(c, npx * 4 * n);
			if (!d_index || !d_scaled || agmv_fmt_gather(c, src->fmt, src->src_w, src->src_h, src->d_frames, n, d_index, npx, d_scaled, NULL))
				agmv_die("frame gather");
		}
		if ((d_scaled ? agmv_hip_similarity_dev(c, d_scaled, n, npx, d_counts, NULL)
		            : agmv_fmt_similarity(c, src->fmt, src->src_w, src->src_h, src->d_frames, n, d_counts, NULL)) ||
		    (n > 1 && agmv_hip_memcpy_async(c, m->counts, d_counts, 4 * (size_t)(n - 1), 1, NULL)) || agmv_hip_stream_sync(c, NULL))
			agmv_die("frame similarity");
		free(index);                                           /* (the upload has read it) */
		agmv_hip_free_on(c, d_counts); agmv_hip_free_on(c, d_scaled); agmv_hip_free_on(c, d_index);
	}
}

static int similar(similarity* m, long x)
{
	const size_t npx = (size_t)m->w * m->h;
	size_t k;
	if (m->counts) return m->counts[x - m->src->first] / (f32)npx >= m->leniency;
	agmv_load_source(m->src->dir, m->src->base, x, m->scale_w, m->scale_h, m->w, m->h, m->tmp); for (k = 0; k < npx; k++) m->fa[k] = m->tmp[k];
	agmv_load_source(m->src->dir, m->src->base, x + 1, m->scale_w, m->scale_h, m->w, m->h, m->tmp); for (k = 0; k < npx; k++) m->fb[k] = m->tmp[k];
	return AGMV_CompareFrameSimilarity(m->fa, m->fb, m->w, m->h) >= m->leniency;
}

static void similarity_close(similarity* m) { free(m->fa); free(m->fb); free(m->tmp); free(m->counts); }

/* The three sequence encoders of the reference (src/agmv_encode.c:2270-3657 AGMV_EncodeAGMV = AGMV_SCHEDULE_PDIFS, :3659-4407
   AGMV_EncodeFullAGMV = AGMV_SCHEDULE_FULL, :719-2268 AGMV_EncodeVideo = AGMV_SCHEDULE_ADAPTIVE; BMP branch) over one body:
   they differ in which frames they push and in how they patch the header afterwards.  `src` says where the frames start_frame
   .. end_frame are: BMP files, or device memory (AGMV_EncodeFramesDev).  Frees `a`, like the reference's drivers. */
static void encode_sequence(AGMV* a, const char* filename, const agmv_source* src, AGMV_SCHEDULE schedule, u32 start_frame,
                            u32 end_frame, u32 width, u32 height, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression)
{
	u32 adjusted = end_frame - start_frame, i;
	int sw, sh;
	FILE* file;
	agmv_seq* s;
	u32 written;
	uint32_t* hist = (uint32_t*)malloc(4u << 19);
	if (!hist) agmv_die("out of host memory");
	AGMV_SetOPT(a, opt);
	AGMV_SetCompression(a, compression);
	if (schedule == AGMV_SCHEDULE_PDIFS) {
		AGMV_SetLeniency(a, 0);
		adjusted = pdifs_adjusted(opt, adjusted);
	} else if (schedule == AGMV_SCHEDULE_ADAPTIVE) {
		f32 len;
		switch (opt) {                                        /* :744-790 */
		case AGMV_OPT_II: len = 0.1282f; break;
		case AGMV_OPT_GBA_I: case AGMV_OPT_GBA_II: case AGMV_OPT_GBA_III: case AGMV_OPT_NDS: len = 0.0f; break;
		default: len = 0.2282f; break;
		}
		AGMV_SetLeniency(a, len);
	}
	scaled_size(opt, &sw, &sh);
	if (sw) { AGMV_SetWidth(a, (u32)sw); AGMV_SetHeight(a, (u32)sh); }     /* the GBA / NDS opts encode at their own size */

	/* pass 1 of the palette build on the GPU (histogram) */
	agmv_histogram_frames(ctx(), src, start_frame, end_frame, width * height, (int)quality, lz_threads(), hist);
	if (schedule == AGMV_SCHEDULE_PDIFS && a->audio_chunk) a->audio_chunk->size = (u32)(a->header.audio_size / (f32)adjusted);   /* 0 without an audio track */
	/* :4024 divides by end_frame - start_frame, one less than the frames (and chunks) it writes: with a track, the chunks of a FULL
	   file ask for more codes than audio_size holds, and AGMV_EncodeAudioChunk writes zeros where the reference reads on */
	if (schedule == AGMV_SCHEDULE_FULL && a->audio_chunk)
		a->audio_chunk->size = (u32)(a->header.audio_size / (f32)(end_frame > start_frame ? end_frame - start_frame : 1));

	if (AGMV_GetTotalAudioDuration(a) != 0 && a->audio_chunk && a->audio_track) {      /* :2661-2667, :4023-4029 */
		/* an object with a track gets its codes; a track that came from device memory brought them along (attach_audio_dev) */
		if (!a->audio_chunk->atsample && (AGMV_GetBitsPerSample(a) == 16 ? (void*)a->audio_track->pcm : (void*)a->audio_track->pcm8)) {
			a->audio_chunk->atsample = (u8*)calloc(AGMV_GetAudioSize(a) ? AGMV_GetAudioSize(a) : 1, 1);
			if (!a->audio_chunk->atsample) { fprintf(stderr, "libagmv(amd): out of host memory for the audio codes\n"); abort(); }
			AGMV_CompressAudio(a);
		}
		a->audio_track->start_point = 0;
	}

	file = create_with_palette(a, filename, hist, quality, opt, palette_refine());
	free(hist);

	if (schedule == AGMV_SCHEDULE_FULL) {                     /* every input frame, no PDIFS, no header patch */
		s = seq_open(a, file, src, opt, AGMV_GetTotalAudioDuration(a) != 0, 0);
		for (i = start_frame; i <= end_frame; i++) agmv_seq_push(s, i, -1);
		(void)agmv_seq_close(s);
	} else {
		/* :2678, :3610-3612 and :719-2268: a PDIFS group per step, or -- AGMV_EncodeVideo, where the pair that decides (the two
		   middle frames of a light group, the two frames of a heavy one) is not similar -- the one frame alone.
		   NDS is "light" only for BMP input (:2727 vs :2810), and the frames of both sources are what BMP input gives */
		similarity m;
		s = seq_open(a, file, src, opt, schedule == AGMV_SCHEDULE_PDIFS, 1);
		if (schedule == AGMV_SCHEDULE_ADAPTIVE) similarity_open(&m, src, a, opt);
		for (i = start_frame; i <= end_frame;) {
			if (schedule == AGMV_SCHEDULE_ADAPTIVE && !similar(&m, heavy_pdifs(opt) ? (long)i : (long)i + 1)) { agmv_seq_push(s, i, -1); i += 1; }
			else if (!heavy_pdifs(opt)) { agmv_seq_push(s, i, -1); agmv_seq_push(s, i + 1, i + 2); agmv_seq_push(s, i + 3, -1); i += 4; }
			else { agmv_seq_push(s, i, i + 1); i += 2; }
			if (i + 4 >= end_frame) break;
		}
		if (schedule == AGMV_SCHEDULE_ADAPTIVE) similarity_close(&m);
		written = agmv_seq_close(s);

		patch_header(file, a, written, schedule == AGMV_SCHEDULE_PDIFS ? (f32)adjusted / (AGMV_GetNumberOfFrames(a) + 1) : (f32)written / AGMV_GetNumberOfFrames(a));
	}
	fclose(file);
	DestroyAGMV(a);                                           /* the callee frees the caller's object, :3625 */
	if (is_gba(opt) && !src->d_frames) dump_gba_header(filename);
}

static agmv_source bmp_source(const char* dir, const char* basename, u8 img_type)
{
	const agmv_source src = {.dir = dir, .base = basename};
	require_bmp(img_type);
	return src;
}

void AGMV_EncodeAGMV(AGMV* a, const char* filename, const char* dir, const char* basename, u8 img_type, u32 start_frame,
                     u32 end_frame, u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality,
                     AGMV_COMPRESSION compression)
{
	const agmv_source src = bmp_source(dir, basename, img_type);
	(void)frames_per_second;
	encode_sequence(a, filename, &src, AGMV_SCHEDULE_PDIFS, start_frame, end_frame, width, height, opt, quality, compression);
}

void AGMV_EncodeFullAGMV(AGMV* a, const char* filename, const char* dir, const char* basename, u8 img_type, u32 start_frame,
                         u32 end_frame, u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality,
                         AGMV_COMPRESSION compression)
{
	const agmv_source src = bmp_source(dir, basename, img_type);
	(void)frames_per_second;
	encode_sequence(a, filename, &src, AGMV_SCHEDULE_FULL, start_frame, end_frame, width, height, opt, quality, compression);
}

void AGMV_EncodeVideo(const char* filename, const char* dir, const char* basename, u8 img_type, u32 start_frame, u32 end_frame,
                      u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression)
{
	const agmv_source src = bmp_source(dir, basename, img_type);
	encode_sequence(CreateAGMV(end_frame - start_frame, width, height, frames_per_second), filename, &src, AGMV_SCHEDULE_ADAPTIVE,
	                start_frame, end_frame, width, height, opt, quality, compression);
}

/* an AGMV_PIXFMT the sequence drivers take: a byte layout without flags, or a YUV 4:2:0 layout with its two flags at most */
static int known_pixfmt(int fmt)
{
	const int base = fmt & 0xFF, flags = fmt & ~0xFF;
	if (base == AGMV_PIXFMT_NV12 || base == AGMV_PIXFMT_I420) return (flags & ~(AGMV_YUV_BT709 | AGMV_YUV_FULL_RANGE)) == 0;
	return flags == 0 && base >= AGMV_PIXFMT_XRGB32 && base <= AGMV_PIXFMT_RGB8P;
}

int AGMV_SetAudioDev(const void* d_pcm, AGMV_PCMFMT fmt, u32 samples_per_channel, u32 sample_rate, u16 channels)
{
	memset(&g_audio, 0, sizeof(g_audio));
	if (!d_pcm) return 0;
	if (fmt != AGMV_PCM_S16 && fmt != AGMV_PCM_U8 && fmt != AGMV_PCM_F32P) return -1;
	if (channels == 0 || channels > 255 || (fmt == AGMV_PCM_F32P && channels > 8)) return -2;      /* the object holds the count in a u8 */
	if (sample_rate == 0) return -3;
	if (samples_per_channel / sample_rate == 0) return -4;
	if (samples_per_channel > 0xFFFFFFFFul / channels) return -5;
	g_audio.d_pcm = d_pcm; g_audio.fmt = (int)fmt; g_audio.samples = samples_per_channel; g_audio.rate = sample_rate; g_audio.channels = channels;
	return 0;
}

/* the pending device track becomes the object's: the header as the WAV importer sets it for that PCM, and the codes of the whole
   track from one compand kernel on the library's device (the object holds no PCM of its own, encode_sequence finds the codes) */
static void attach_audio_dev(AGMV* a)
{
	agmv_hip_ctx* c = ctx();
	const size_t n = (size_t)g_audio.samples * g_audio.channels;
	void* stream = agmv_hip_stream_create(c);
	uint8_t *d_codes = (uint8_t*)agmv_hip_malloc_on(c, n), *h_codes = (uint8_t*)agmv_hip_host_alloc(n);
	u8* codes = (u8*)malloc(n);
	if (!stream || !d_codes || !h_codes || !codes) agmv_die("buffers for the audio track");
	if (agmv_hip_audio_compand_async(c, g_audio.fmt, g_audio.d_pcm, g_audio.channels, g_audio.samples, d_codes, stream) ||
	    agmv_hip_memcpy_async(c, h_codes, d_codes, n, 1, stream) || agmv_hip_stream_sync(c, stream))
		agmv_die("audio compand");
	memcpy(codes, h_codes, n);
	agmv_hip_host_free(h_codes); agmv_hip_free_on(c, d_codes); agmv_hip_stream_destroy(c, stream);
	AGMV_SetBitsPerSample(a, g_audio.fmt == AGMV_PCM_U8 ? 8 : 16);
	AGMV_SetAudioSize(a, (u32)n);
	AGMV_SetSampleRate(a, g_audio.rate);
	AGMV_SetNumberOfChannels(a, (u8)g_audio.channels);
	AGMV_SetTotalAudioDuration(a, g_audio.samples / g_audio.rate);
	a->audio_chunk->atsample = codes;
}

/* a pending AGMV_SetAudioDev track is consumed by every AGMV_EncodeFrames*Dev call, whatever it returns: each of them returns through here */
static int audio_consumed(int rc) { memset(&g_audio, 0, sizeof(g_audio)); return rc; }

/* what every AGMV_EncodeFrames*Dev refuses of its enums (-1), of a pending track (-5) and of the number of frames (-2), in this
   order; 0 where it has nothing to object to.  Needs no device. */
static int encode_args_refused(u32 num_of_frames, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	if (opt < AGMV_OPT_I || opt > AGMV_OPT_NDS || quality < AGMV_HIGH_QUALITY || quality > AGMV_LOW_QUALITY ||
	    (compression != AGMV_LZSS_COMPRESSION && compression != AGMV_LZ77_COMPRESSION) ||
	    (schedule != AGMV_SCHEDULE_FULL && schedule != AGMV_SCHEDULE_PDIFS && schedule != AGMV_SCHEDULE_ADAPTIVE))
		return -1;
	if (schedule == AGMV_SCHEDULE_ADAPTIVE && g_audio.d_pcm) return -5;      /* AGMV_EncodeVideo has no audio */
	/* the first group of the schedule reads this many frames whatever the length of the clip */
	if (num_of_frames < (schedule == AGMV_SCHEDULE_FULL ? 1u : (heavy_pdifs(opt) ? 2u : 4u)) || num_of_frames > 0x7FFFFFFFul) return -2;
	return 0;
}

/* what AGMV_EncodeFramesDev refuses, in its order (-1, -5, -2, -3): 0, or the negative value; needs no device */
static int encode_frames_refused(const char* filename, const void* d_frames, u32 num_of_frames, u32 width, u32 height, AGMV_OPT opt, AGMV_QUALITY quality,
                                 AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	int sw, sh;
	const int rc = filename && d_frames ? encode_args_refused(num_of_frames, opt, quality, compression, schedule) : -1;
	if (rc) return rc;
	scaled_size(opt, &sw, &sh);
	if (width == 0 || height == 0 || (unsigned long long)width * height > (1ull << 28)) return -3;
	return (sw ? width < 2 || height < 2 : bad_geometry((uint32_t)width, (uint32_t)height)) ? -3 : 0;
}

/* The same three files from frames in device memory (include/agmv.h): what the BMP drivers write for f1.bmp .. f<n>.bmp holding these
   frames, byte for byte (for AGMV_SCHEDULE_ADAPTIVE with AGMV_EncodeVideo's CreateAGMV(n - 1, ...)); GBA_GEN_AGMV.h is not written.
   Returns 0, or a negative value -- before any file is created -- for arguments that cannot be encoded. */
static int encode_frames_dev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 width, u32 height,
                             u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	agmv_source src = {.d_frames = d_frames, .fmt = (int)fmt, .src_w = (uint32_t)width, .src_h = (uint32_t)height, .n_frames = (uint32_t)num_of_frames, .first = 1};
	AGMV* a;
	const int refused = known_pixfmt((int)fmt) ? encode_frames_refused(filename, d_frames, num_of_frames, width, height, opt, quality, compression, schedule) : -1;
	if (refused) return refused;
	src.device = agmv_hip_ctx_device(ctx());
	a = CreateAGMV(schedule == AGMV_SCHEDULE_ADAPTIVE ? num_of_frames - 1 : num_of_frames, width, height, frames_per_second);
	if (g_audio.d_pcm) attach_audio_dev(a);
	encode_sequence(a, filename, &src, schedule, 1, num_of_frames, width, height, opt, quality, compression);
	return 0;
}

int AGMV_EncodeFramesFmtDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 width, u32 height,
                            u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	return audio_consumed(encode_frames_dev(filename, d_frames, fmt, num_of_frames, width, height, frames_per_second, opt, quality, compression, schedule));
}

int AGMV_EncodeFramesDev(const char* filename, const unsigned* d_frames, u32 num_of_frames, u32 width, u32 height,
                         u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	return AGMV_EncodeFramesFmtDev(filename, d_frames, AGMV_PIXFMT_XRGB32, num_of_frames, width, height, frames_per_second, opt, quality, compression, schedule);
}

/* A clip that is not encoded as it lies there (a target size, a tensor, a view; include/agmv.h has the rules): the XRGB32 clip it
   stands for is materialised once on the library's device -- the source is read once in its own layout, where the histogram, the
   similarity and the encode would each read it -- and AGMV_EncodeFramesDev runs on that.  Nothing of the source's size or layout is
   allocated.  How the clip is filled: the box filter, a gather through agmv_scale_index, agmv_hip_tensor_to_xrgb_async, or the
   windows of selected frames by agmv_hip_view_source_async.  FILL_AREA / FILL_NEAREST with a view scale those windows: they exist one
   staging batch at a time, which the scaler reads as an XRGB32 source.  A view at another frame rate is the same with R in the place
   of V: agmv_hip_time_frames_async writes what agmv_hip_view_source_async would. */
static AGMV_ENCODE_VIEW_STATS g_encode_view_stats;  /* of the last AGMV_EncodeViewDev */

void AGMV_GetEncodeViewStats(AGMV_ENCODE_VIEW_STATS* out) { if (out) *out = g_encode_view_stats; }

typedef struct clip_fill {
	enum { FILL_AREA, FILL_NEAREST, FILL_TENSOR, FILL_VIEW } how;
	const void* d_src;
	int fmt;                               /* the AGMV_PIXFMT of d_src; FILL_TENSOR: its AGMV_TENSORFMT */
	uint32_t src_w, src_h;                 /* of a source frame (FILL_TENSOR: not read, the clip has the tensor's size) */
	const float* ab;                       /* FILL_TENSOR: a[3] then b[3] of the reading rule */
	const AGMV_VIEW* view;                 /* FILL_VIEW, or a scale of a view: first, step and the window, resolved; clip frame j is source frame first + j * step */
	AGMV_ENCODE_VIEW_STATS* stats;         /* where a view reports the clip it materialised; else NULL */
	const AGMV_RATE* rate;                 /* a view at another frame rate (reduced, not 1 : 1): the clip is R, made by agmv_hip_time_frames_async; else NULL */
	uint32_t view_len, src_frames;         /* with a rate: the length of V and the frames of the source clip */
} clip_fill;

/* frames j0 .. j0 + n - 1 of a view (with a rate: of R) as packed XRGB32 at d_dst: one launch */
static int fill_view_frames(agmv_hip_ctx* c, const clip_fill* f, uint32_t j0, uint32_t n, uint32_t* d_dst, void* stream)
{
	const AGMV_VIEW* v = f->view;
	if (f->rate)
		return agmv_hip_time_frames_async(c, f->fmt, f->d_src, f->src_w, f->src_h, f->src_frames, v->first, v->step, f->view_len, v->x, v->y, v->width, v->height,
		                                  f->rate->src, f->rate->dst, (int)f->rate->filter, j0, n, d_dst, stream);
	return agmv_hip_view_source_async(c, f->fmt, f->d_src, f->src_w, f->src_h, v->first + j0 * v->step, v->step, n, v->x, v->y, v->width, v->height, d_dst, stream);
}

/* A staging batch of a scaled view: as many windows as fit 256 MiB -- the size of the memory-side cache, taken as a bound
   on memory, not as a tuned value -- and at least one; AGMV_VIEW_STAGE_FRAMES=n (read per call, a test aid) forces n. */
#define VIEW_STAGE_BYTES ((size_t)256 << 20)

static uint32_t view_stage_frames(size_t window_px, uint32_t length)
{
	const char* e = getenv("AGMV_VIEW_STAGE_FRAMES");
	size_t n = e && atol(e) > 0 ? (size_t)atol(e) : VIEW_STAGE_BYTES / (4 * window_px);
	if (n < 1) n = 1;
	return n < length ? (uint32_t)n : length;
}

/* the windows of a view scaled into d_clip: batch by batch through d_stage, every launch on `stream` and in its order */
static int fill_scaled_view(agmv_hip_ctx* c, const clip_fill* f, uint32_t n, uint32_t w, uint32_t h, uint32_t stage, uint32_t* d_stage, const uint32_t* d_index,
                            uint32_t* d_clip, void* stream)
{
	const AGMV_VIEW* v = f->view;
	const size_t npx = (size_t)w * h;
	uint32_t j, nb;
	for (j = 0; j < n; j += nb) {
		nb = n - j < stage ? n - j : stage;
		if (fill_view_frames(c, f, j, nb, d_stage, stream)) return -1;
		if (f->how == FILL_AREA ? agmv_hip_scale_area_dev(c, AGMV_PIXFMT_XRGB32, d_stage, v->width, v->height, nb, w, h, d_clip + j * npx, stream)
		                        : agmv_fmt_gather(c, AGMV_PIXFMT_XRGB32, v->width, v->height, d_stage, nb, d_index, npx, d_clip + j * npx, stream))
			return -1;
	}
	return 0;
}

/* -4 where the clip (or the index of FILL_NEAREST, or the staging batch of a scaled view) cannot be allocated, else what
   encode_frames_dev returns for the clip */
static int encode_materialised(const char* filename, const clip_fill* f, u32 num_of_frames, u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt,
                               AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	agmv_hip_ctx* c = ctx();
	const uint32_t n = (uint32_t)num_of_frames, w = (uint32_t)width, h = (uint32_t)height;
	const size_t npx = (size_t)w * h;
	const int tensor = f->how == FILL_TENSOR, staged = f->view && f->how != FILL_VIEW;
	const uint32_t from_w = staged ? f->view->width : f->src_w, from_h = staged ? f->view->height : f->src_h;      /* what the scaler reads */
	const uint32_t stage = staged ? view_stage_frames((size_t)from_w * from_h, n) : 0;
	uint32_t *d_clip = (uint32_t*)agmv_hip_malloc_on(c, 4 * npx * num_of_frames), *d_index = NULL, *index = NULL, *d_stage = NULL;
	void* stream;
	int failed, rc;
	if (!d_clip) return -4;
	if (f->how == FILL_NEAREST) {
		index = agmv_scale_index(from_w, from_h, w, h);
		d_index = (uint32_t*)agmv_hip_malloc_on(c, 4 * npx);
	}
	if (staged) d_stage = (uint32_t*)agmv_hip_malloc_on(c, 4 * (size_t)from_w * from_h * stage);
	if ((f->how == FILL_NEAREST && (!index || !d_index)) || (staged && !d_stage)) {
		free(index); agmv_hip_free_on(c, d_index); agmv_hip_free_on(c, d_stage); agmv_hip_free_on(c, d_clip);
		return -4;
	}
	stream = agmv_hip_stream_create(c);
	if (!stream) agmv_die(tensor ? "stream for the tensor clip" : f->view ? "stream for the view" : "stream for the scaled clip");
	if (f->how == FILL_NEAREST && agmv_hip_memcpy_async(c, d_index, index, 4 * npx, 0, stream)) failed = -1;
	else if (tensor) failed = agmv_hip_tensor_to_xrgb_async(c, f->fmt, f->d_src, npx, n, f->ab, d_clip, stream);
	else if (f->how == FILL_VIEW)
		failed = fill_view_frames(c, f, 0, n, d_clip, stream);
	else if (staged) failed = fill_scaled_view(c, f, n, w, h, stage, d_stage, d_index, d_clip, stream);
	else if (f->how == FILL_AREA) failed = agmv_hip_scale_area_dev(c, f->fmt, f->d_src, f->src_w, f->src_h, n, w, h, d_clip, stream);
	else failed = agmv_fmt_gather(c, f->fmt, f->src_w, f->src_h, f->d_src, n, d_index, npx, d_clip, stream);
	if (failed || agmv_hip_stream_sync(c, stream)) agmv_die(tensor ? "tensor clip" : f->view ? "view of the source" : "frame scale");
	agmv_hip_stream_destroy(c, stream);
	free(index); agmv_hip_free_on(c, d_index); agmv_hip_free_on(c, d_stage);
	if (f->stats) { f->stats->clip_bytes = 4ull * npx * n; f->stats->staging_bytes = 4ull * from_w * from_h * stage; }
	rc = encode_frames_dev(filename, d_clip, AGMV_PIXFMT_XRGB32, num_of_frames, width, height, frames_per_second, opt, quality, compression, schedule);
	agmv_hip_free_on(c, d_clip);
	return rc;
}

/* what AGMV_EncodeFramesScaledDev refuses before a device is opened, in its order: -1, -5, -3 and only then -2 */
static int encode_scaled_refused(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height, u32 width,
                                 u32 height, AGMV_SCALE filter, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	const unsigned long long src_px = (unsigned long long)src_width * src_height;
	int sw, sh, rc;
	if (!known_pixfmt((int)fmt) || !filename || !d_frames || (filter != AGMV_SCALE_NEAREST && filter != AGMV_SCALE_AREA)) return -1;
	rc = encode_args_refused(num_of_frames, opt, quality, compression, schedule);
	if (rc == -1 || rc == -5) return rc;
	scaled_size(opt, &sw, &sh);
	if (sw || bad_geometry((uint32_t)width, (uint32_t)height) || width > 0xFFFFFFFFul || height > 0xFFFFFFFFul) return -3;
	if (src_width == 0 || src_height == 0 || src_width > 0xFFFFFFFFul || src_height > 0xFFFFFFFFul || src_px > (1ull << 28)) return -3;
	if (filter == AGMV_SCALE_AREA && (width > src_width || height > src_height || src_px > (1ull << 24))) return -3;
	return rc;
}

int AGMV_EncodeFramesScaledDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height,
                               u32 width, u32 height, AGMV_SCALE filter, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality,
                               AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	const clip_fill f = {filter == AGMV_SCALE_AREA ? FILL_AREA : FILL_NEAREST, d_frames, (int)fmt, (uint32_t)src_width, (uint32_t)src_height, NULL};
	const int rc = encode_scaled_refused(filename, d_frames, fmt, num_of_frames, src_width, src_height, width, height, filter, opt, quality, compression, schedule);
	return audio_consumed(rc ? rc : encode_materialised(filename, &f, num_of_frames, width, height, frames_per_second, opt, quality, compression, schedule));
}

/* a normalisation the tensor entry points take: agmv_hip_tensor_table holds the bounds (and needs no device) */
static int known_tensor(AGMV_TENSORFMT type, const float* mean, const float* std, void* table) { return mean && std && agmv_hip_tensor_table((int)type, mean, std, table) == 0; }

int AGMV_EncodeFramesTensorDev(const char* filename, const void* d_tensor, AGMV_TENSORFMT type, const float mean[3], const float std[3], u32 num_of_frames,
                               u32 width, u32 height, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression,
                               AGMV_SCHEDULE schedule)
{
	uint32_t table[768];
	float ab[6];
	const clip_fill f = {FILL_TENSOR, d_tensor, (int)type, 0, 0, ab};
	int i, rc = known_tensor(type, mean, std, table) ? encode_frames_refused(filename, d_tensor, num_of_frames, width, height, opt, quality, compression, schedule) : -1;
	for (i = 0; i < 3 && !rc; i++) { ab[i] = (float)(255.0 * (double)std[i]); ab[3 + i] = (float)(255.0 * (double)mean[i]); }
	return audio_consumed(rc ? rc : encode_materialised(filename, &f, num_of_frames, width, height, frames_per_second, opt, quality, compression, schedule));
}

/* Writer sessions (include/agmv_writer.h has the contract): the checks of the one-shot call of the same layout, one persistent histogram for pass 1,
   and for pass 2 a ring of XRGB32 frames at the encode size that is the source of an agmv_seq opened here and started at the first write.  How a
   stretch of frames reaches the ring: a conversion (STAGE_COPY), the box filter (STAGE_AREA), a gather through d_index (STAGE_GATHER: the nearest
   filter of a target size, or the scale of a GBA / NDS opt), or the tensor's reading rule (STAGE_TENSOR; under a GBA / NDS opt into d_xrgb first,
   at the source's size, and gathered from there). */
struct AGMV_WRITER {
	AGMV_WRITER_DESC d; char* filename; AGMV* a; FILE* file; agmv_seq* s;
	agmv_hip_ctx* c; void* stream;
	enum { STAGE_COPY, STAGE_AREA, STAGE_GATHER, STAGE_TENSOR } how;
	int fmt;                               /* of the frames handed in: the AGMV_PIXFMT with its flags, or the AGMV_TENSORFMT */
	int hist_as_handed_in;                 /* the palette's histogram is of the frames before the scale (no target size: the one-shot call's rule) */
	uint32_t src_w, src_h, w, h;           /* of the frames handed in, of the frames encoded */
	size_t src_px, src_bytes, npx;
	float ab[6];
	uint32_t *d_hist, *d_ring, *d_index, *d_xrgb, ring, xrgb_frames;
	unsigned refine; int pdifs, heavy;
	unsigned long long analysed, taken;
	uint32_t groups;                       /* PDIFS: groups pushed */
	unsigned writes, waits;
};

/* what the one-shot call of the description's layout refuses before it opens a device, with a clip that is never read and a frame count that passes
   (the count's check waits for the close) */
static int writer_refused(const char* filename, const AGMV_WRITER_DESC* q)
{
	const u32 any = 0x7FFFFFFFul;
	const int sized = q->width != 0 || q->height != 0, fmt = (int)q->fmt | q->yuv_flags;
	uint32_t table[768];
	int rc;
	if (q->schedule == AGMV_SCHEDULE_ADAPTIVE) return -1;
	if (q->tensor) {
		rc = known_tensor(q->type, q->mean, q->std, table) ? encode_frames_refused(filename, q, any, q->src_width, q->src_height, q->opt, q->quality, q->compression, q->schedule) : -1;
		return rc ? rc : sized ? -3 : 0;
	}
	if (sized)
		return encode_scaled_refused(filename, q, (AGMV_PIXFMT)fmt, any, q->src_width, q->src_height, q->width, q->height, q->filter, q->opt, q->quality, q->compression, q->schedule);
	return known_pixfmt(fmt) ? encode_frames_refused(filename, q, any, q->src_width, q->src_height, q->opt, q->quality, q->compression, q->schedule) : -1;
}

static void writer_free(AGMV_WRITER* w)
{
	agmv_hip_free_on(w->c, w->d_hist); agmv_hip_free_on(w->c, w->d_ring); agmv_hip_free_on(w->c, w->d_index); agmv_hip_free_on(w->c, w->d_xrgb);
	if (w->stream) agmv_hip_stream_destroy(w->c, w->stream);
	DestroyAGMV(w->a);
	free(w->filename);
	free(w);
}

AGMV_WRITER* AGMV_OpenWriterDev(const char* filename, const AGMV_WRITER_DESC* q, int* error)
{
	int err = q ? writer_refused(filename, q) : -1, sw, sh, i;
	AGMV_WRITER* w = NULL;
	if (!err && !(w = (AGMV_WRITER*)calloc(1, sizeof(*w)))) agmv_die("out of host memory");
	if (w) {
		const int sized = q->width != 0 || q->height != 0;
		uint32_t* index = NULL;
		unsigned cap, batch_sources;
		scaled_size(q->opt, &sw, &sh);
		w->d = *q; w->c = ctx(); w->pdifs = q->schedule == AGMV_SCHEDULE_PDIFS; w->heavy = heavy_pdifs(q->opt); w->refine = palette_refine();
		w->src_w = (uint32_t)q->src_width; w->src_h = (uint32_t)q->src_height; w->src_px = (size_t)w->src_w * w->src_h;
		w->w = sw ? (uint32_t)sw : sized ? (uint32_t)q->width : w->src_w; w->h = sw ? (uint32_t)sh : sized ? (uint32_t)q->height : w->src_h; w->npx = (size_t)w->w * w->h;
		w->fmt = q->tensor ? (int)q->type : (int)q->fmt | q->yuv_flags;
		w->src_bytes = q->tensor ? agmv_hip_tensor_frame_bytes(w->fmt, w->src_px) : agmv_fmt_frame_bytes(w->fmt, w->src_w, w->src_h);
		w->how = q->tensor ? STAGE_TENSOR : sized ? (q->filter == AGMV_SCALE_AREA ? STAGE_AREA : STAGE_GATHER) : sw ? STAGE_GATHER : STAGE_COPY;
		w->hist_as_handed_in = !q->tensor && !sized;
		for (i = 0; i < 3 && q->tensor; i++) { w->ab[i] = (float)(255.0 * (double)q->std[i]); w->ab[3 + i] = (float)(255.0 * (double)q->mean[i]); }
		cap = batch_frames(w->npx); batch_sources = w->pdifs ? 2 * cap : cap;
		w->ring = 4 * batch_sources + (w->pdifs ? 6 : 0);
		if (q->ring_frames) w->ring = q->ring_frames < batch_sources + (w->pdifs ? 6 : 0) ? batch_sources + (w->pdifs ? 6 : 0) : q->ring_frames;
		w->filename = (char*)malloc(strlen(filename) + 1);
		if (!w->filename) agmv_die("out of host memory");
		strcpy(w->filename, filename);
		if (sw) index = agmv_source_index(w->src_w, w->src_h, sw, sh, w->w, w->h);
		else if (w->how == STAGE_GATHER && !(index = agmv_scale_index(w->src_w, w->src_h, w->w, w->h))) agmv_die("out of host memory");
		w->d_hist = (uint32_t*)agmv_hip_malloc_on(w->c, 4u << 19); w->d_ring = (uint32_t*)agmv_hip_malloc_on(w->c, 4 * w->npx * w->ring);
		if (index) w->d_index = (uint32_t*)agmv_hip_malloc_on(w->c, 4 * w->npx);
		if (index && q->tensor) { w->xrgb_frames = cap; w->d_xrgb = (uint32_t*)agmv_hip_malloc_on(w->c, 4 * w->src_px * cap); }
		if (!w->d_hist || !w->d_ring || (index && !w->d_index) || (w->xrgb_frames && !w->d_xrgb)) {      /* as the one-shot calls answer a clip they cannot hold */
			free(index); writer_free(w);
			w = NULL; err = -4;
		} else {
			const agmv_source src = {.d_frames = w->d_ring, .fmt = AGMV_PIXFMT_XRGB32, .src_w = w->w, .src_h = w->h, .first = 1, .device = agmv_hip_ctx_device(w->c), .ring_frames = w->ring};
			if (!(w->stream = agmv_hip_stream_create(w->c))) agmv_die("stream for the writer");
			if (agmv_hip_memset_async(w->c, w->d_hist, 0, 4u << 19, w->stream) || (index && agmv_hip_memcpy_async(w->c, w->d_index, index, 4 * w->npx, 0, w->stream)) ||
			    agmv_hip_stream_sync(w->c, w->stream))
				agmv_die("writer set-up");
			free(index);
			w->a = CreateAGMV(0, w->w, w->h, q->frames_per_second);
			AGMV_SetOPT(w->a, q->opt); AGMV_SetCompression(w->a, q->compression);
			if (w->pdifs) AGMV_SetLeniency(w->a, 0);
			w->s = seq_open(w->a, NULL, &src, q->opt, w->pdifs, w->pdifs);      /* (a PDIFS file carries an AGAC chunk header behind every frame, empty without a track) */
		}
	}
	if (error) *error = err;
	return w;
}

/* n frames at `at`, as handed in, to n XRGB32 frames of the encode size at dst, on the writer's stream */
static int writer_stage(AGMV_WRITER* w, const u8* at, uint32_t n, uint32_t* dst)
{
	uint32_t nb;
	switch (w->how) {
	case STAGE_AREA: return agmv_hip_scale_area_dev(w->c, w->fmt, at, w->src_w, w->src_h, n, w->w, w->h, dst, w->stream);
	case STAGE_GATHER: return agmv_fmt_gather(w->c, w->fmt, w->src_w, w->src_h, at, n, w->d_index, w->npx, dst, w->stream);
	case STAGE_TENSOR:
		if (!w->d_xrgb) return agmv_hip_tensor_to_xrgb_async(w->c, w->fmt, at, w->npx, n, w->ab, dst, w->stream);
		for (; n; n -= nb, at += nb * w->src_bytes, dst += nb * w->npx) {
			nb = n < w->xrgb_frames ? n : w->xrgb_frames;
			if (agmv_hip_tensor_to_xrgb_async(w->c, w->fmt, at, w->src_px, nb, w->ab, w->d_xrgb, w->stream) ||
			    agmv_fmt_gather(w->c, AGMV_PIXFMT_XRGB32, w->src_w, w->src_h, w->d_xrgb, nb, w->d_index, w->npx, dst, w->stream))
				return -1;
		}
		return 0;
	default: return agmv_fmt_to_xrgb(w->c, w->fmt, w->src_w, w->src_h, at, n, w->npx, dst, w->stream);
	}
}

/* Pass 1: the frames join d_hist in the layout the one-shot call histograms -- as handed in, or, for a target size and a tensor, as XRGB32 frames made
   piece by piece in the ring, which is empty until the first write (a tensor under a GBA / NDS opt: in d_xrgb, before the scale) */
int AGMV_WriterAnalyseDev(AGMV_WRITER* w, const void* d_frames, u32 n)
{
	const u8* at = (const u8*)d_frames;
	uint32_t left = (uint32_t)n, nb;
	int failed = 0;
	if (!w || (!d_frames && n)) return -1;
	if (!n) return 0;
	if (w->file) return -6;
	if (n > 0x7FFFFFFFul || w->analysed + n > 0x7FFFFFFFul) return -2;
	if (w->hist_as_handed_in) failed = agmv_fmt_histogram(w->c, w->fmt, w->src_w, w->src_h, at, left, w->src_px, (int)w->d.quality, w->d_hist, w->stream);
	else for (; left && !failed; left -= nb, at += nb * w->src_bytes) {
		if (w->d_xrgb) {
			nb = left < w->xrgb_frames ? left : w->xrgb_frames;
			failed = agmv_hip_tensor_to_xrgb_async(w->c, w->fmt, at, w->src_px, nb, w->ab, w->d_xrgb, w->stream) ||
			         agmv_fmt_histogram(w->c, AGMV_PIXFMT_XRGB32, w->src_w, w->src_h, w->d_xrgb, nb, w->src_px, (int)w->d.quality, w->d_hist, w->stream);
		} else {
			nb = left < w->ring ? left : w->ring;
			failed = writer_stage(w, at, nb, w->d_ring) || agmv_fmt_histogram(w->c, AGMV_PIXFMT_XRGB32, w->w, w->h, w->d_ring, nb, w->npx, (int)w->d.quality, w->d_hist, w->stream);
		}
	}
	if (failed || agmv_hip_stream_sync(w->c, w->stream)) agmv_die("writer histogram");
	w->analysed += n;
	return 0;
}

/* the schedule's frames that the arrivals so far decide, pushed: sources are numbered from 1, as the one-shot calls number theirs */
static void writer_push(AGMV_WRITER* w, unsigned long long before)
{
	if (!w->pdifs) {
		for (; before < w->taken; before++) agmv_seq_push(w->s, (long)before + 1, -1);
		return;
	}
	for (; w->groups < agmv_writer_groups((uint32_t)w->taken, w->heavy, 0); w->groups++) {
		const long i = (long)w->groups * (w->heavy ? 2 : 4) + 1;
		if (w->heavy) agmv_seq_push(w->s, i, i + 1);
		else { agmv_seq_push(w->s, i, -1); agmv_seq_push(w->s, i + 1, i + 2); agmv_seq_push(w->s, i + 3, -1); }
	}
}

/* Pass 2.  The first write freezes the palette: histogram -> palette -> header, then the workers receive the palette and the file.  The frames go into the
   ring stretch by stretch -- as far as it is free and does not wrap -- and are pushed once they are complete there. */
int AGMV_WriterWriteDev(AGMV_WRITER* w, const void* d_frames, u32 n)
{
	const u8* at = (const u8*)d_frames;
	uint32_t left = (uint32_t)n;
	if (!w || (!d_frames && n)) return -1;
	if (!n) return 0;
	if (!w->analysed) return -6;
	if (n > 0x7FFFFFFFul || w->taken + n > 0x7FFFFFFFul) return -2;
	if (!w->file) {
		uint32_t* hist = (uint32_t*)malloc(4u << 19);
		if (!hist) agmv_die("out of host memory");
		if (agmv_hip_memcpy_async(w->c, hist, w->d_hist, 4u << 19, 1, w->stream) || agmv_hip_stream_sync(w->c, w->stream)) agmv_die("histogram download");
		w->file = create_with_palette(w->a, w->filename, hist, w->d.quality, w->d.opt, w->refine);
		free(hist);
		seq_start(w->s, w->a, w->file, w->d.opt);
	}
	w->writes++;
	while (left) {
		const unsigned long long before = w->taken;
		unsigned long freed = agmv_seq_sources_free(w->s);
		const uint32_t pos = (uint32_t)(w->taken % w->ring);
		uint32_t nb;
		if (w->taken - freed >= w->ring) {             /* the ring is full: until the batch that holds its oldest frame has left */
			w->waits++;
			freed = agmv_seq_wait_sources_free(w->s, (unsigned long)(w->taken - w->ring + 1));
		}
		nb = w->ring - (uint32_t)(w->taken - freed);
		if (nb > w->ring - pos) nb = w->ring - pos;
		if (nb > left) nb = left;
		if (writer_stage(w, at, nb, w->d_ring + (size_t)pos * w->npx) || agmv_hip_stream_sync(w->c, w->stream)) agmv_die("writer staging");
		w->taken += nb; left -= nb; at += (size_t)nb * w->src_bytes;
		writer_push(w, before);
	}
	return 0;
}

int AGMV_CloseWriter(AGMV_WRITER* w, u32* frames_written)
{
	u32 written;
	int too_few;
	if (!w) return 0;
	too_few = w->taken < (w->pdifs ? (w->heavy ? 2u : 4u) : 1u);
	written = agmv_seq_close(w->s);
	if (w->file) {
		const u32 n = (u32)w->taken;
		if (!too_few) patch_header(w->file, w->a, written, w->pdifs ? (f32)pdifs_adjusted(w->d.opt, n - 1) / (n + 1) : 1.0f);
		fclose(w->file);
		if (too_few) remove(w->filename);
	}
	if (frames_written) *frames_written = too_few ? 0 : written;
	writer_free(w);
	return too_few ? -2 : 0;
}

void AGMV_GetWriterStats(const AGMV_WRITER* w, AGMV_WRITER_STATS* stats)
{
	if (!stats) return;
	memset(stats, 0, sizeof(*stats));
	if (!w) return;
	stats->analysed = w->analysed; stats->taken = w->taken; stats->writes = w->writes; stats->waits = w->waits; stats->ring_frames = w->ring;
	agmv_seq_counts(w->s, &stats->batches, &stats->written);
}

/* ------------------------------------------------------------------------------------------
 * sequence decoders (reference src/agmv_decode.c:455-647): host does the chunk scan and the LZ stage
 * frame by frame into ONE persistent buffer (so the stale-tail semantics hold), the GPU parses and
 * reconstructs whole batches, frames are exported as quick_export_<n>.bmp in the CWD.
 * ------------------------------------------------------------------------------------------ */
/* the entries of n measured frames from the device array where agmv_hip_measure_frames_async made them, once */
static void download_quality(agmv_hip_ctx* c, const void* d_q, AGMV_FRAME_QUALITY* quality, size_t n)
{
	if (n && (agmv_hip_memcpy_async(c, quality, d_q, n * sizeof(AGMV_FRAME_QUALITY), 1, NULL) || agmv_hip_stream_sync(c, NULL))) agmv_die("quality download");
}

/* An .agmv file the decoders read: agmv_file_open reads the header (and fills *info, which may be NULL), agmv_file_slurp then holds the whole file
   in memory, `len` bytes with 16 zero bytes behind them, `pos` the first byte behind the header.  Both return an Error; agmv_file_close after either. */
typedef struct agmv_file { FILE* f; AGMV hdr; u8* image; size_t len, pos; } agmv_file;

static int agmv_file_open(agmv_file* af, const char* filename, AGMV_INFO* info)
{
	int err;
	af->image = NULL;
	if (!(af->f = filename ? fopen(filename, "rb") : NULL)) return FILE_NOT_FOUND_ERR;
	memset(&af->hdr, 0, sizeof(af->hdr.header));
	err = AGMV_DecodeHeader(af->f, &af->hdr);
	if (err == NO_ERR && info) *info = AGMV_GetVideoInfo(&af->hdr);
	return err;
}

static int agmv_file_slurp(agmv_file* af)
{
	long flen;
	af->pos = (size_t)ftell(af->f);
	fseek(af->f, 0, SEEK_END); flen = ftell(af->f); fseek(af->f, 0, SEEK_SET);
	af->image = (u8*)malloc((size_t)flen + 16);
	if (!af->image) return MEMORY_CORRUPTION_ERR;
	af->len = fread(af->image, 1, (size_t)flen, af->f);
	memset(af->image + af->len, 0, 16);
	return NO_ERR;
}

static void agmv_file_close(agmv_file* af) { if (af->f) fclose(af->f); free(af->image); }

/* the public return value of a decoder: the frames (samples) it made, or its Error negated; -3 and -4 of decode_file are negative already.
   (The count by address: it is read here, behind the decode that the caller's expression holds as the other argument.) */
static int decode_result(int err, const unsigned long* count) { return err == NO_ERR ? (int)*count : err < 0 ? err : -err; }

/* The file's frames into `sink`: every frame for EXPORT (AGMV_DecodeAGMV / AGMV_DecodeVideo), up to cap_frames frames for the other
   kinds, their number added to *sink->count.  For MEASURE (AGMV_MeasureFileDev) the reference clip holds exactly cap_frames frames,
   the device array sink->measure.d_quality is made here, and the entries of the frames measured land in quality[] (host memory),
   downloaded once.  *info (may be NULL) = the header's; with info_only nothing else happens.  Returns an Error, or before a device is opened
   -3 where the reference cannot correspond to the file, -4 where the box filter cannot scale the file's frames to the sink's target. */
static AGMV_VIEW_STATS g_view_stats;                 /* of the last AGMV_DecodeViewDev / AGMV_DecodeViewTensorDev */

void AGMV_GetViewStats(AGMV_VIEW_STATS* out) { if (out) *out = g_view_stats; }

/* The view of a sink as the caller gave it (include/agmv.h) against the file's header: the window's own size, the number of frames it
   delivers in count, and `viewed` cleared for the view that selects everything, which is the decode without a view of that many
   frames.  -4 where the file refuses the view, else NO_ERR. */
static int resolve_view(agmv_sink* sink, const AGMV_MAIN_HEADER* hd, u32 cap_frames)
{
	const agmv_target* to = agmv_sink_target(sink);
	AGMV_VIEW* v = &sink->view;
	const u32 fw = hd->width, fh = hd->height;
	uint32_t n;
	if (v->width == 0) { v->width = (unsigned)fw; v->height = (unsigned)fh; }
	else if (v->x > fw || v->width > fw - v->x || v->y > fh || v->height > fh - v->y) return -4;
	if (to && to->filter == AGMV_SCALE_AREA && (to->w > v->width || to->h > v->height || (unsigned long long)fw * fh > (1ull << 24))) return -4;
	if (!to && sink->kind == AGMV_SINK_FRAMES && AGMV_FMT_IS_YUV(sink->frames.fmt) && ((v->width | v->height) & 1)) return -4;
	n = agmv_view_length(v->first, v->step, v->count, hd->num_of_frames > 0xFFFFFFFFul ? 0xFFFFFFFFu : (uint32_t)hd->num_of_frames);
	v->count = n > cap_frames ? (unsigned)cap_frames : n;
	if (v->first == 0 && v->step == 1 && v->width == fw && v->height == fh) sink->viewed = 0;
	return NO_ERR;
}

/* the palette of a file's header as the device takes it, and whether it is two palettes */
static void header_palette(const AGMV_MAIN_HEADER* hd, uint32_t pal[512], int* m512)
{
	int i;
	*m512 = hd->version == 1 || hd->version == 3;
	for (i = 0; i < 256; i++) { pal[i] = (uint32_t)hd->palette0[i]; pal[256 + i] = *m512 ? (uint32_t)hd->palette1[i] : 0; }
}

/* ... on the device, uploaded when it differs from the one that is there */
static int device_palette(agmv_hip_ctx* c, const uint32_t pal[512], int m512)
{
	if (g_pal_mode == m512 && memcmp(pal, g_pal, sizeof(g_pal)) == 0) return 0;
	if (agmv_hip_set_palette(c, pal, pal + 256, m512, NULL) || agmv_hip_sync()) return -1;
	memcpy(g_pal, pal, sizeof(g_pal));
	g_pal_mode = m512;
	return 0;
}

static int decode_file(const char* filename, u8 img_type, agmv_sink* sink, AGMV_FRAME_QUALITY* quality, u32 cap_frames, int info_only, AGMV_INFO* info)
{
	const agmv_target* to = agmv_sink_target(sink);
	const int measure = sink->kind == AGMV_SINK_MEASURE, view = sink->viewed;
	agmv_file af;
	const AGMV_MAIN_HEADER* hd = &af.hdr.header;
	uint32_t nframes, pal[512];
	int err = agmv_file_open(&af, filename, info), m512;
	agmv_hip_ctx* c;
	if (err != FILE_NOT_FOUND_ERR) require_bmp(img_type);        /* (the file exists) */
	if (err == NO_ERR && !info_only) {
		/* (a rule of the API, not a dispatch: 4:2:0 chroma cannot lie over an odd frame) */
		if (measure && (hd->num_of_frames != cap_frames || (AGMV_FMT_IS_YUV(sink->measure.fmt) && ((hd->width | hd->height) & 1)))) err = -3;
		else if (view && resolve_view(sink, hd, cap_frames) != NO_ERR) err = -4;
		else if (!view && to && to->filter == AGMV_SCALE_AREA && (to->w > hd->width || to->h > hd->height || (unsigned long long)hd->width * hd->height > (1ull << 24))) err = -4;
		else if ((err = agmv_file_slurp(&af)) == NO_ERR && bad_geometry((uint32_t)hd->width, (uint32_t)hd->height)) err = INVALID_HEADER_FORMATTING_ERR;
	}
	if (err != NO_ERR || info_only || (sink->viewed && sink->view.count == 0)) { agmv_file_close(&af); return err; }      /* (a view without a frame: nothing to do) */
	c = open_ctx();
	if (!c) { agmv_file_close(&af); return gpu_failed("cannot open the GPU"); }
	header_palette(hd, pal, &m512);
	if (device_palette(c, pal, m512)) { agmv_file_close(&af); return gpu_failed("palette upload"); }
	nframes = (uint32_t)hd->num_of_frames;
	if (sink->kind != AGMV_SINK_EXPORT && nframes > cap_frames) nframes = (uint32_t)cap_frames;
	if (view) nframes = sink->viewed ? sink->view.first + (sink->view.count - 1) * sink->view.step + 1 : sink->view.count;      /* behind the last frame it needs */
	if (measure && nframes) {
		sink->measure.d_quality = agmv_hip_malloc_on(c, (size_t)nframes * sizeof(AGMV_FRAME_QUALITY));
		if (!sink->measure.d_quality) { agmv_file_close(&af); return gpu_failed("result array for the measurement"); }
	}
	err = agmv_decode_stream(c, af.image, af.len, af.pos, (uint32_t)hd->width, (uint32_t)hd->height, nframes, hd->version, hd->total_audio_duration != 0,
	                         batch_frames((size_t)hd->width * hd->height), lz_threads(), sink, view ? &g_view_stats : NULL);
	if (measure && err == NO_ERR) download_quality(c, sink->measure.d_quality, quality, (size_t)*sink->count);
	if (measure) agmv_hip_free_on(c, sink->measure.d_quality);
	agmv_file_close(&af);
	return err;
}

int AGMV_DecodeVideo(const char* filename, u8 img_type)
{
	agmv_sink sink = {AGMV_SINK_EXPORT, &g_export_count, {{0}}};
	return decode_file(filename, img_type, &sink, NULL, 0, 0, NULL);
}

/* the video frames are exported exactly like the reference does; no quick_export.wav / .aiff is written here (callers of this
   build never found one in their working directory): AGMV_DecodeAudio(filename, audio_type) is the audio export */
int AGMV_DecodeAGMV(const char* filename, u8 img_type, AGMV_AUDIO_TYPE audio_type)
{
	(void)audio_type;
	return AGMV_DecodeVideo(filename, img_type);
}

/* AGMV_DecodeAGMV with another destination (include/agmv.h): at most cap_frames frames into d_frames in the layout `fmt`, at the target
   `to` of AGMV_DecodeFramesScaledDev or, with NULL, at the file's size.  With d_frames NULL nothing is decoded and only *info is filled. */
static int decode_frames(const char* filename, void* d_frames, AGMV_PIXFMT fmt, const agmv_target* to, u32 cap_frames, AGMV_INFO* info)
{
	unsigned long decoded = 0;
	agmv_sink sink = {AGMV_SINK_FRAMES, &decoded, .frames = {d_frames, (int)fmt, to ? *to : (agmv_target){0, 0, 0}}};
	return decode_result(decode_file(filename, AGMV_IMG_BMP, &sink, NULL, cap_frames, d_frames == NULL, info), &decoded);
}

int AGMV_DecodeFramesFmtDev(const char* filename, void* d_frames, AGMV_PIXFMT fmt, u32 cap_frames, AGMV_INFO* info)
{
	return known_pixfmt((int)fmt) ? decode_frames(filename, d_frames, fmt, NULL, cap_frames, info) : -1;
}

int AGMV_DecodeFramesDev(const char* filename, unsigned* d_frames, u32 cap_frames, AGMV_INFO* info)
{
	return AGMV_DecodeFramesFmtDev(filename, d_frames, AGMV_PIXFMT_XRGB32, cap_frames, info);
}

/* a target the sized decoders take: -1 for an unknown filter, then -4 for a width or height of zero or more than 2^28 target pixels */
static int target_refused(u32 width, u32 height, AGMV_SCALE filter)
{
	if (filter != AGMV_SCALE_NEAREST && filter != AGMV_SCALE_AREA && filter != AGMV_SCALE_BILINEAR) return -1;
	if (width == 0 || height == 0 || width > (1ul << 28) || height > (1ul << 28) || (unsigned long long)width * height > (1ull << 28)) return -4;
	return 0;
}

/* AGMV_DecodeFramesFmtDev with a target size (include/agmv.h has the rules); the checks that need no device come first, in the header's order */
int AGMV_DecodeFramesScaledDev(const char* filename, void* d_frames, AGMV_PIXFMT fmt, u32 width, u32 height, AGMV_SCALE filter, u32 cap_frames,
                               AGMV_INFO* info)
{
	const agmv_target to = {(uint32_t)width, (uint32_t)height, (int)filter};
	const int refused = filename && known_pixfmt((int)fmt) ? target_refused(width, height, filter) : -1;
	return refused ? refused : decode_frames(filename, d_frames, fmt, &to, cap_frames, info);
}

/* AGMV_DecodeFramesScaledDev into a tensor clip: the same checks in the same order, the table built here; width == height == 0 is the file's size */
int AGMV_DecodeFramesTensorDev(const char* filename, void* d_tensor, AGMV_TENSORFMT type, const float mean[3], const float std[3], u32 width, u32 height,
                               AGMV_SCALE filter, u32 cap_frames, AGMV_INFO* info)
{
	unsigned long decoded = 0;
	uint32_t table[768];
	const int sized = width != 0 || height != 0;
	agmv_sink sink = {AGMV_SINK_TENSOR, &decoded, .tensor = {d_tensor, (int)type, table, {(uint32_t)width, (uint32_t)height, sized ? (int)filter : 0}}};
	const int refused = filename && known_tensor(type, mean, std, table) ? (sized ? target_refused(width, height, filter) : 0) : -1;
	return refused ? refused : decode_result(decode_file(filename, AGMV_IMG_BMP, &sink, NULL, cap_frames, d_tensor == NULL, info), &decoded);
}

/* A view of a file (include/agmv.h): the sized decoders with a selection of frames and a window in front of the sink.  view_refused is
   the -1 class of the view's own fields; NULL is the whole file. */
static const AGMV_VIEW WHOLE_FILE = {0, 0, 1, 0, 0, 0, 0};

static int view_refused(const AGMV_VIEW* v)
{
	return v && (v->step == 0 || (v->width == 0) != (v->height == 0) || (v->width == 0 && (v->x || v->y)));
}

int AGMV_DecodeViewDev(const char* filename, void* d_frames, AGMV_PIXFMT fmt, u32 width, u32 height, AGMV_SCALE filter, const AGMV_VIEW* view,
                       u32 cap_frames, AGMV_INFO* info)
{
	unsigned long decoded = 0;
	const int sized = width != 0 || height != 0;
	agmv_sink sink = {AGMV_SINK_FRAMES, &decoded, .frames = {d_frames, (int)fmt, {(uint32_t)width, (uint32_t)height, sized ? (int)filter : 0}},
	                  .viewed = 1, .view = view ? *view : WHOLE_FILE};
	const int refused = filename && known_pixfmt((int)fmt) && !view_refused(view) ? (sized ? target_refused(width, height, filter) : 0) : -1;
	memset(&g_view_stats, 0, sizeof(g_view_stats));
	return refused ? refused : decode_result(decode_file(filename, AGMV_IMG_BMP, &sink, NULL, cap_frames, d_frames == NULL, info), &decoded);
}

int AGMV_DecodeViewTensorDev(const char* filename, void* d_tensor, AGMV_TENSORFMT type, const float mean[3], const float std[3], u32 width, u32 height,
                             AGMV_SCALE filter, const AGMV_VIEW* view, u32 cap_frames, AGMV_INFO* info)
{
	unsigned long decoded = 0;
	uint32_t table[768];
	const int sized = width != 0 || height != 0;
	agmv_sink sink = {AGMV_SINK_TENSOR, &decoded, .tensor = {d_tensor, (int)type, table, {(uint32_t)width, (uint32_t)height, sized ? (int)filter : 0}},
	                  .viewed = 1, .view = view ? *view : WHOLE_FILE};
	const int refused = filename && known_tensor(type, mean, std, table) && !view_refused(view) ? (sized ? target_refused(width, height, filter) : 0) : -1;
	memset(&g_view_stats, 0, sizeof(g_view_stats));
	return refused ? refused : decode_result(decode_file(filename, AGMV_IMG_BMP, &sink, NULL, cap_frames, d_tensor == NULL, info), &decoded);
}

/* Reader sessions (include/agmv_reader.h): the checks of the two view decoders in their order, the file image and its palette kept, and
   agmv_dreader of agmv_pipeline.h behind them.  The library's context has one palette: a read puts its file's there first when another
   file's decode has replaced it. */
struct AGMV_READER { agmv_file af; agmv_dreader* r; uint32_t pal[512]; int m512; };

AGMV_READER* AGMV_OpenReaderDev(const char* filename, const AGMV_READER_DESC* desc, AGMV_INFO* info, int* error)
{
	static const AGMV_READER_DESC none;
	const AGMV_READER_DESC* q = desc ? desc : &none;
	const AGMV_VIEW view = {0, 0, q->step ? q->step : 1, q->x, q->y, q->win_width, q->win_height};
	const int sized = q->width != 0 || q->height != 0, fmt = (int)q->fmt | q->yuv_flags;
	const agmv_target to = {(uint32_t)q->width, (uint32_t)q->height, sized ? (int)q->filter : 0};
	uint32_t table[768];
	unsigned long unused = 0;
	agmv_sink sink = {AGMV_SINK_FRAMES, &unused, .frames = {NULL, fmt, to}, .viewed = 1, .view = view};
	const int known = q->tensor ? known_tensor(q->type, q->mean, q->std, table) : known_pixfmt(fmt);
	int err = desc && filename && known && !view_refused(&view) ? (sized ? target_refused(q->width, q->height, q->filter) : 0) : -1;
	AGMV_READER* rd = NULL;
	const AGMV_MAIN_HEADER* hd;
	agmv_hip_ctx* c = NULL;
	if (q->tensor) { sink.kind = AGMV_SINK_TENSOR; sink.tensor.d_dst = NULL; sink.tensor.type = (int)q->type; sink.tensor.table = table; sink.tensor.to = to; }
	if (!err && !(rd = (AGMV_READER*)calloc(1, sizeof(*rd)))) err = -MEMORY_CORRUPTION_ERR;
	if (!err) {
		hd = &rd->af.hdr.header;
		err = agmv_file_open(&rd->af, filename, info);
		if (err == NO_ERR && resolve_view(&sink, hd, 0xFFFFFFFFu) != NO_ERR) err = -4;
		else if (err == NO_ERR && (err = agmv_file_slurp(&rd->af)) == NO_ERR && bad_geometry((uint32_t)hd->width, (uint32_t)hd->height)) err = INVALID_HEADER_FORMATTING_ERR;
		if (err == NO_ERR && !(c = open_ctx())) err = gpu_failed("cannot open the GPU");
		if (err == NO_ERR) {
			const agmv_dfile f = {rd->af.image, rd->af.len, rd->af.pos, (uint32_t)hd->width, (uint32_t)hd->height,
			                      hd->num_of_frames > 0xFFFFFFFFul ? 0xFFFFFFFFu : (uint32_t)hd->num_of_frames, hd->version, hd->total_audio_duration != 0};
			const unsigned deblock = q->deblock ? (q->deblock > 64 ? 64 : q->deblock) : agmv_deblock_strength();
			header_palette(hd, rd->pal, &rd->m512);
			if (device_palette(c, rd->pal, rd->m512)) err = gpu_failed("palette upload");
			else if (!(rd->r = agmv_dreader_open(c, &f, batch_frames((size_t)f.w * f.h), lz_threads(), &sink, deblock, q->index_bytes ? q->index_bytes : (size_t)64 << 20)))
				err = gpu_failed("cannot open the reader");
		}
		if (err != NO_ERR) { agmv_file_close(&rd->af); free(rd); rd = NULL; err = err < 0 ? err : -err; }
	}
	if (error) *error = err;
	return rd;
}

int AGMV_ReaderReadDev(AGMV_READER* rd, void* d_dst, u32 n)
{
	if (!rd || (!d_dst && n)) return -1;
	if (!n) return 0;
	if (device_palette(g_ctx, rd->pal, rd->m512)) return -gpu_failed("palette upload");
	return agmv_dreader_read(rd->r, d_dst, n > 0xFFFFFFFFul ? 0xFFFFFFFFu : (uint32_t)n);
}

int AGMV_ReaderSeek(AGMV_READER* rd, u32 frame)
{
	if (!rd) return -1;
	agmv_dreader_seek(rd->r, frame > 0xFFFFFFFFul ? 0xFFFFFFFFu : (uint32_t)frame);
	return 0;
}

u32 AGMV_ReaderTell(const AGMV_READER* rd) { return rd ? agmv_dreader_tell(rd->r) : 0; }

void AGMV_GetReaderStats(const AGMV_READER* rd, AGMV_READER_STATS* stats)
{
	if (!stats) return;
	memset(stats, 0, sizeof(*stats));
	if (rd) agmv_dreader_stats(rd->r, stats);
}

void AGMV_CloseReader(AGMV_READER* rd)
{
	if (!rd) return;
	agmv_dreader_close(rd->r);
	agmv_file_close(&rd->af);
	free(rd);
}

/* a rate as AGMV_EncodeViewRateDev takes it, reduced into *q (NULL: 1 : 1); non-zero for one the header refuses with -1 */
static int rate_refused(const AGMV_RATE* rate, AGMV_RATE* q)
{
	unsigned a, b;
	q->src = q->dst = 1; q->filter = AGMV_TIME_AREA;
	if (!rate) return 0;
	if (rate->src == 0 || rate->dst == 0 || (rate->filter != AGMV_TIME_NEAREST && rate->filter != AGMV_TIME_AREA)) return 1;
	for (a = rate->src, b = rate->dst; b; ) { const unsigned t = a % b; a = b; b = t; }
	q->src = rate->src / a; q->dst = rate->dst / a; q->filter = rate->filter;
	return q->src > 65535u || q->dst > 65535u || (q->filter == AGMV_TIME_AREA && q->dst > q->src);
}

/* A view of a clip encoded (include/agmv.h has the rules).  encode_view_refused is everything that needs no device, in the header's
   order; *r receives the view resolved against the clip: count = its length, width x height = the window's own size.  With a rate
   (reduced; {1, 1} for none) the schedule is asked about the length of R, and a YUV source of odd size is never encoded in place. */
static int encode_view_refused(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height, const AGMV_VIEW* view,
                               const AGMV_RATE* q, u32 width, u32 height, AGMV_SCALE filter, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression,
                               AGMV_SCHEDULE schedule, AGMV_VIEW* r)
{
	const int rated = q->src != 1 || q->dst != 1;
	const int sized = width != 0 || height != 0;
	const unsigned long long src_px = (unsigned long long)src_width * src_height;
	int sw, sh, rc;
	if (!known_pixfmt((int)fmt) || !filename || !d_frames || (sized && filter != AGMV_SCALE_NEAREST && filter != AGMV_SCALE_AREA) || view_refused(view)) return -1;
	*r = view ? *view : WHOLE_FILE;
	r->count = agmv_view_length(r->first, r->step, r->count, num_of_frames > 0xFFFFFFFFul ? 0xFFFFFFFFu : (uint32_t)num_of_frames);
	rc = encode_args_refused((u32)((unsigned long long)r->count * q->dst / q->src), opt, quality, compression, schedule);
	if (rc == -1 || rc == -5) return rc;
	if (src_width == 0 || src_height == 0 || src_width > 0xFFFFFFFFul || src_height > 0xFFFFFFFFul || src_px > (1ull << 28)) return -3;
	if (r->width == 0) { r->width = (unsigned)src_width; r->height = (unsigned)src_height; }
	if (r->x > src_width || r->width > src_width - r->x || r->y > src_height || r->height > src_height - r->y) return -3;
	/* an NV12 / I420 window is cut out of the 2 x 2 cells of an even frame (agmv_hip_view_source_async); consecutive full frames are not cut */
	if (AGMV_FMT_IS_YUV((int)fmt) && ((src_width | src_height) & 1) && (rated || !(r->step == 1 && r->width == src_width && r->height == src_height))) return -3;
	scaled_size(opt, &sw, &sh);
	if (!sized) {
		if (sw ? r->width < 2 || r->height < 2 : bad_geometry(r->width, r->height)) return -3;
	} else {
		if (sw || width > 0xFFFFFFFFul || height > 0xFFFFFFFFul || bad_geometry((uint32_t)width, (uint32_t)height)) return -3;
		if (filter == AGMV_SCALE_AREA && (width > r->width || height > r->height || (unsigned long long)r->width * r->height > (1ull << 24))) return -3;
	}
	return rc;
}

int AGMV_EncodeViewDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height, const AGMV_VIEW* view,
                       u32 width, u32 height, AGMV_SCALE filter, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality, AGMV_COMPRESSION compression,
                       AGMV_SCHEDULE schedule)
{
	const int sized = width != 0 || height != 0;
	static const AGMV_RATE same = {1, 1, AGMV_TIME_AREA};
	AGMV_VIEW v;
	clip_fill f = {sized ? (filter == AGMV_SCALE_AREA ? FILL_AREA : FILL_NEAREST) : FILL_VIEW, d_frames, (int)fmt, (uint32_t)src_width, (uint32_t)src_height, NULL, NULL,
	               &g_encode_view_stats};
	int rc, whole_frames;
	memset(&g_encode_view_stats, 0, sizeof(g_encode_view_stats));
	rc = encode_view_refused(filename, d_frames, fmt, num_of_frames, src_width, src_height, view, &same, width, height, filter, opt, quality, compression, schedule, &v);
	if (rc) return audio_consumed(rc);
	whole_frames = v.step == 1 && v.width == src_width && v.height == src_height;
	if (whole_frames) f.d_src = (const u8*)d_frames + (size_t)v.first * agmv_fmt_frame_bytes((int)fmt, f.src_w, f.src_h);     /* consecutive full frames: read in place */
	else f.view = &v;
	if (whole_frames && !sized) rc = encode_frames_dev(filename, f.d_src, fmt, v.count, src_width, src_height, frames_per_second, opt, quality, compression, schedule);
	else rc = encode_materialised(filename, &f, v.count, sized ? width : v.width, sized ? height : v.height, frames_per_second, opt, quality, compression, schedule);
	if (rc) memset(&g_encode_view_stats, 0, sizeof(g_encode_view_stats));
	else g_encode_view_stats.frames = v.count;
	return audio_consumed(rc);
}

/* The same at another frame rate (include/agmv.h has the rule): the clip that is materialised is R.  1 : 1 is the call above. */
static AGMV_ENCODE_RATE_STATS g_encode_rate_stats;  /* of the last AGMV_EncodeViewRateDev */

void AGMV_GetEncodeRateStats(AGMV_ENCODE_RATE_STATS* out) { if (out) *out = g_encode_rate_stats; }

int AGMV_EncodeViewRateDev(const char* filename, const void* d_frames, AGMV_PIXFMT fmt, u32 num_of_frames, u32 src_width, u32 src_height, const AGMV_VIEW* view,
                           const AGMV_RATE* rate, u32 width, u32 height, AGMV_SCALE filter, u32 frames_per_second, AGMV_OPT opt, AGMV_QUALITY quality,
                           AGMV_COMPRESSION compression, AGMV_SCHEDULE schedule)
{
	const int sized = width != 0 || height != 0;
	AGMV_RATE q;
	AGMV_VIEW v;
	clip_fill f = {sized ? (filter == AGMV_SCALE_AREA ? FILL_AREA : FILL_NEAREST) : FILL_VIEW, d_frames, (int)fmt, (uint32_t)src_width, (uint32_t)src_height, NULL, &v,
	               &g_encode_view_stats, &q};
	unsigned long long m;
	int rc;
	memset(&g_encode_rate_stats, 0, sizeof(g_encode_rate_stats));
	if (rate_refused(rate, &q)) {
		memset(&g_encode_view_stats, 0, sizeof(g_encode_view_stats));
		return audio_consumed(-1);
	}
	if (q.src == 1 && q.dst == 1) {
		rc = AGMV_EncodeViewDev(filename, d_frames, fmt, num_of_frames, src_width, src_height, view, width, height, filter, frames_per_second, opt, quality, compression,
		                        schedule);
		if (!rc) {
			g_encode_rate_stats.frames_in = g_encode_rate_stats.frames_out = g_encode_view_stats.frames;
			g_encode_rate_stats.frame_reads = g_encode_view_stats.frames;
		}
		return rc;
	}
	memset(&g_encode_view_stats, 0, sizeof(g_encode_view_stats));
	rc = encode_view_refused(filename, d_frames, fmt, num_of_frames, src_width, src_height, view, &q, width, height, filter, opt, quality, compression, schedule, &v);
	if (rc) return audio_consumed(rc);
	m = (unsigned long long)v.count * q.dst / q.src;
	f.view_len = v.count;
	f.src_frames = num_of_frames > 0xFFFFFFFFul ? 0xFFFFFFFFu : (uint32_t)num_of_frames;
	rc = encode_materialised(filename, &f, (u32)m, sized ? width : v.width, sized ? height : v.height, frames_per_second, opt, quality, compression, schedule);
	if (rc) memset(&g_encode_view_stats, 0, sizeof(g_encode_view_stats));
	else {
		g_encode_view_stats.frames = (unsigned)m;
		g_encode_rate_stats.frames_in = v.count;
		g_encode_rate_stats.frames_out = (unsigned)m;
		/* AREA: output j reads taps (j sn) div dn .. ((j + 1) sn - 1) div dn, which is one more than the step of (j sn) div dn unless dn divides j + 1 */
		g_encode_rate_stats.frame_reads = q.filter == AGMV_TIME_NEAREST ? m : m * q.src / q.dst + m - m / q.dst;
	}
	return audio_consumed(rc);
}

/* The file's audio track into device memory in the layout `fmt` (include/agmv.h): the AGAC payloads gathered on the host into
   one pinned buffer, one upload, one expand kernel.  No video is decoded. */
int AGMV_DecodeAudioDev(const char* filename, void* d_pcm, AGMV_PCMFMT fmt, u32 cap_samples, AGMV_INFO* info)
{
	agmv_file af;
	const AGMV_MAIN_HEADER* hd = &af.hdr.header;
	uint8_t *h_codes = NULL, *d_codes;
	unsigned long n = 0;
	u32 channels = 0;
	int err;
	agmv_hip_ctx* c;
	void* stream;
	if (fmt != AGMV_PCM_S16 && fmt != AGMV_PCM_U8 && fmt != AGMV_PCM_F32P) return -1;
	err = agmv_file_open(&af, filename, info);
	if (err == NO_ERR && d_pcm && hd->total_audio_duration != 0) {
		const size_t cap = hd->audio_size < cap_samples ? hd->audio_size : cap_samples;
		channels = hd->num_of_channels;
		if ((hd->bits_per_sample == 16) == (fmt == AGMV_PCM_U8) || channels == 0 || (fmt == AGMV_PCM_F32P && channels > 8)) err = -1;
		else if ((err = agmv_file_slurp(&af)) == NO_ERR && !(h_codes = (uint8_t*)agmv_hip_host_alloc(cap ? cap : 1))) err = gpu_failed("pinned buffer for the audio codes");
		if (err == NO_ERR) n = agmv_gather_audio(af.image, af.len, af.pos, (uint32_t)hd->num_of_frames, h_codes, cap);
		if (n > 0x7FFFFFFFu) n = 0x7FFFFFFFu;                  /* the return value is an int */
		if (n) n -= n % channels;
	}
	agmv_file_close(&af);
	if (err != NO_ERR || n == 0) { agmv_hip_host_free(h_codes); return decode_result(err, &n); }
	c = open_ctx();
	if (!c) { agmv_hip_host_free(h_codes); return decode_result(gpu_failed("cannot open the GPU"), &n); }
	stream = agmv_hip_stream_create(c);
	d_codes = (uint8_t*)agmv_hip_malloc_on(c, n);
	if (!stream || !d_codes || agmv_hip_memcpy_async(c, d_codes, h_codes, n, 0, stream) ||
	    agmv_hip_audio_expand_async(c, (int)fmt, d_codes, channels, n / channels, d_pcm, stream) || agmv_hip_stream_sync(c, stream))
		err = gpu_failed("audio expand");
	agmv_hip_free_on(c, d_codes); agmv_hip_host_free(h_codes);
	if (stream) agmv_hip_stream_destroy(c, stream);
	return decode_result(err, &n);
}

/* ------------------------------------------------------------------------------------------
 * measuring a decoded clip (include/agmv.h, "measuring a decoded clip"): the entries are made on the device by
 * agmv_hip_measure_frames_async and downloaded once
 * ------------------------------------------------------------------------------------------ */
int AGMV_MeasureFramesDev(const unsigned* d_test, const void* d_ref, AGMV_PIXFMT ref_fmt, u32 num_of_frames, u32 width, u32 height,
                          AGMV_FRAME_QUALITY* quality)
{
	agmv_hip_ctx* c;
	void *stream, *d_q;
	if (!known_pixfmt((int)ref_fmt) || !d_test || !d_ref || !quality) return -1;
	if (width > 0xFFFFFFFFul || height > 0xFFFFFFFFul || bad_geometry((uint32_t)width, (uint32_t)height) || num_of_frames > 0x7FFFFFFFul) return -3;
	if (num_of_frames == 0) return 0;
	c = ctx();
	stream = agmv_hip_stream_create(c);
	d_q = agmv_hip_malloc_on(c, (size_t)num_of_frames * sizeof(AGMV_FRAME_QUALITY));
	if (!stream || !d_q) agmv_die("stream and result array for the measurement");
	if (agmv_hip_measure_frames_async(c, d_test, (int)ref_fmt, d_ref, (uint32_t)width, (uint32_t)height, (uint32_t)num_of_frames, d_q, stream) || agmv_hip_stream_sync(c, stream))
		agmv_die("frame measurement");
	download_quality(c, d_q, quality, (size_t)num_of_frames);
	agmv_hip_free_on(c, d_q);
	agmv_hip_stream_destroy(c, stream);
	return 0;
}

int AGMV_MeasureFileDev(const char* filename, const void* d_ref, AGMV_PIXFMT ref_fmt, u32 num_of_frames, AGMV_FRAME_QUALITY* quality, AGMV_INFO* info)
{
	unsigned long measured = 0;
	agmv_sink sink = {AGMV_SINK_MEASURE, &measured, .measure = {d_ref, (int)ref_fmt, NULL}};
	if (!known_pixfmt((int)ref_fmt) || (quality && !d_ref)) return -1;
	return decode_result(decode_file(filename, AGMV_IMG_BMP, &sink, quality, num_of_frames, quality == NULL, info), &measured);
}

/* ------------------------------------------------------------------------------------------
 * playback helpers, restated from reference src/agmv_playback.c:18-115.  They keep the reference's
 * bookkeeping exactly: offset_table[] is filled as frames are played or skipped over (not only by
 * AGMV_ParseAGMV), seeks are relative to frame_count, and the reset offset is 1574 for container
 * version 1 ONLY (a 512-colour LZ77 file, version 3, is sought to 806 and the next chunk scan walks
 * over its second palette -- that is what the reference does, src/agmv_playback.c:19-24).
 * The one deviation is in undefined territory: indices outside offset_table[MAX_OFFSET_TABLE] are
 * not written / read (the reference has no bound), and a backwards skip past frame 0 lands on frame 0
 * (the reference stores the negative count into the unsigned field, :86-92).
 * ------------------------------------------------------------------------------------------ */
void AGMV_ResetVideo(FILE* f, AGMV* a)
{
	fseek(f, AGMV_GetVersion(a) == 1 ? 1574 : 806, SEEK_SET);     /* :18-26 */
	a->frame_count = 0;
}

Bool AGMV_IsVideoDone(AGMV* a) { return a->frame_count >= AGMV_GetNumberOfFrames(a) ? TRUE : FALSE; }   /* :28-33 */

static void note_offset(FILE* f, AGMV* a)
{
	if (a->frame_count < MAX_OFFSET_TABLE) a->offset_table[a->frame_count] = (u32)ftell(f);
}

/* :35-83: walk forward over NextIFrame(n, frame_count) frame chunks, recording where each one starts */
static void skip_forwards(FILE* f, AGMV* a, int n, int decode_audio)
{
	const int audio = AGMV_GetTotalAudioDuration(a) != 0;
	int i;
	n = AGMV_NextIFrame(n, (int)a->frame_count);
	for (i = 0; i < n; i++) {
		AGMV_FindNextFrameChunk(f);
		note_offset(f, a);
		a->frame_count++;
		AGMV_SkipFrameChunk(f);
		if (audio) {
			AGMV_FindNextAudioChunk(f);
			if (decode_audio) AGMV_DecodeAudioChunk(f, a); else AGMV_SkipAudioChunk(f);
		}
	}
}

void AGMV_SkipForwards(FILE* f, AGMV* a, int n) { skip_forwards(f, a, n, 0); }
void AGMV_SkipForwardsAndDecodeAudio(FILE* f, AGMV* a, int n) { skip_forwards(f, a, n, 1); }

void AGMV_SkipBackwards(FILE* f, AGMV* a, int n)                 /* :85-94 */
{
	int fc = (int)a->frame_count;
	n = AGMV_PrevIFrame(n, fc);
	fc -= n;
	if (fc < 0) fc = 0;
	a->frame_count = (u32)fc;
	if (fc < MAX_OFFSET_TABLE) fseek(f, (long)a->offset_table[fc], SEEK_SET);
}

/* :96-104 ("only call after all frames have been read": offset_table must hold entry n) */
void AGMV_SkipTo(FILE* f, AGMV* a, int n)
{
	n = AGMV_SkipToNearestIFrame(n);
	if (n >= 0 && (u32)n < AGMV_GetNumberOfFrames(a) && n < MAX_OFFSET_TABLE) {
		fseek(f, (long)a->offset_table[n], SEEK_SET);
		a->frame_count = (u32)n;
	}
}

void AGMV_PlayAGMV(FILE* f, AGMV* a)                            /* :106-119 */
{
	AGMV_FindNextFrameChunk(f);
	note_offset(f, a);
	AGMV_DecodeFrameChunk(f, a);
	if (AGMV_GetTotalAudioDuration(a) != 0) { AGMV_FindNextAudioChunk(f); AGMV_SkipAudioChunk(f); }
}
