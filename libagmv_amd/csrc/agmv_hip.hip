// libagmv_amd/csrc/agmv_hip.hip -- hand-written gfx950 (CDNA4 / MI355X) kernels for the AGMV
// per-frame hot path, and the C-ABI of include/agmv_hip.h.
//
// What runs where (reference = /root/reference, cited as file:line):
//   k_lut_build     exact colour -> entry table; replaces the 256/512-way search of
//                   AGMV_FindNearestColor / AGMV_FindNearestEntry (src/agmv_utils.c:785-895)
//   k_mtx_build     512x512 bit matrix "palette colours within +-2 on every channel",
//                   the predicate of CompareI/PFrameBlock (src/agmv_encode.c:293,345)
//   k_dither        opt-in, no counterpart in the reference: pattern dithering of a clip in place before k_encode sees it
//                   (include/agmv.h, "pattern dithering"); the other reader of the table and the palette
//   k_encode        loops A+B of AGMV_EncodeFrame fused (src/agmv_encode.c:552-565, 240-527):
//                   one lane = one 4x4 block carried through the 4 frames of its GOP, one
//                   workgroup = 512 consecutive blocks; per-frame byte offsets by a decoupled
//                   look-back over tiles (single pass over the pixels); no workgroup barrier in
//                   the steady state -- the waves exchange tagged LDS words
// The decoder (the parsers k_parse_* / k_fp_*, k_decode, k_fixup and the calls that launch them) is in agmv_decode_hip.hip.
// The encoder's LZSS stage (AGMV_LZSS, src/agmv_encode.c:106-177) is in agmv_lz_hip.hip; the clip front end (synth, interp,
// histogram, similarity, gather, pixel layouts, area scale) is in agmv_clip_hip.hip.
// Integer/byte work only: no MFMA. The bound is HBM (4 B/px in, usize out).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>

#include "agmv_hip_impl.h"

// ----------------------------------------------------------------------------------------------
// error plumbing
// ----------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int agmv_hip_err(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return -1;
}

int agmv_hip_hip_failed(const char* what, hipError_t e, const char* file, int line)
{
	return agmv_hip_err("agmv_hip: %s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}

extern "C" const char* agmv_hip_last_error(void) { return g_err; }

// ----------------------------------------------------------------------------------------------
// geometry constants
// ----------------------------------------------------------------------------------------------
#ifndef ENC_T_OVERRIDE
#define ENC_T_OVERRIDE 512
#endif
#ifndef ENC_WPE
#define ENC_WPE 4
#endif
#ifndef ENC_PRIO
#define ENC_PRIO 2          /* s_setprio while a wave issues its look-ups + pixel loads (0 = off): the memory pipeline is the scarce unit */
#endif
#ifndef ENC_PIXAUX
#define ENC_PIXAUX 2          /* cache policy of the pixel loads: 2 = nt (streamed once; keeps L2 for the table), 0 = default */
#endif
#ifndef ENC_LUTAUX
#define ENC_LUTAUX 0          /* cache policy of the table look-ups */
#endif
constexpr int ENC_PFDEPTH = 1;     // items whose pixels are in flight per wave (the loop is unrolled by this many register sets); 2 measured the same as 1
constexpr int ENC_T = ENC_T_OVERRIDE;          // threads per encode workgroup = 4x4 blocks per tile
constexpr int ENC_WAVES = ENC_T / 64;
static_assert(ENC_WAVES >= 1 && ENC_WAVES <= 16, "the per-wave offsets are scanned inside one 16-lane row");
constexpr int MROW = 17;            // dwords per matrix row: 16 used + 1 pad (LDS bank spread)
constexpr uint32_t LUT_COLOURS = 1u << 24;
constexpr uint32_t LUT_ENTRIES = 1u << 28;   // index space of the table (see lut_index): 32 MiB populated in 512 MiB

constexpr unsigned long long ST_AGG = 1ull << 32;     // look-back status tags (high word)
constexpr unsigned long long ST_PREFIX = 2ull << 32;

extern "C" size_t agmv_hip_max_usize(uint32_t w, uint32_t h, int mode512)
{
	size_t nblk = (size_t)(w / 4) * (h / 4);
	size_t n = nblk * (mode512 ? 33 : 17) + 64;
	return (n + 255) & ~(size_t)255;
}

// LUT layout: one 128-byte line (64 u16 entries) holds a 4x4x4 cube of colour space, so the pixels
// of a neighbourhood (which differ mostly in the low bits of each channel) share lines.  The L1
// services one distinct line per cycle per gather instruction, which is what bounds the encoder
// (measured: gathers were 35 % of k_encode on the synthetic clip and 90 % on noise with a linear
// R,G,B table).  index = R[7:2] G[7:2] B[7:2] | R[1:0] G[1:0] B[1:0]
__host__ __device__ __forceinline__ uint32_t lut_index(uint32_t px)
{
	// same 4x4x4 cubes, but the cube number keeps the 2-bit holes of the masked pixel (R6 .. G6 .. B6): 6 VALU per
	// look-up instead of 12; the table spans 512 MiB of address space, 32 MiB of it populated (8 KiB runs every 32 KiB)
	return ((px & 0xFCFCFCu) << 4) | ((((px & 0x030303u) * 0x10410u) >> 16) & 0x3Fu);
}

// byte offset of a colour's entry, = 2 * lut_index(px), in 5 VALU for the sparse form (and, mul, bfe, and, lshl_or):
// bit 15 of the product is always 0, so the 7-bit field at bit 15 is the in-cube index already doubled
__device__ __forceinline__ uint32_t lut_offset(uint32_t px)
{
	const uint32_t m = __umul24(px & 0x030303u, 0x10410u);       // full-rate 24-bit multiply (a 32-bit v_mul_lo is quarter rate)
	const uint32_t hi = px & 0xFCFCFCu;
	uint32_t lo, off;                                          // spelled out: the compiler turns this into 4 instructions otherwise
	asm("v_bfe_u32 %0, %1, 15, 7" : "=v"(lo) : "v"(m));
	asm("v_lshl_or_b32 %0, %1, 5, %2" : "=v"(off) : "v"(hi), "v"(lo));
	return off;
}

// ----------------------------------------------------------------------------------------------
// K0: exact colour -> entry table.  One thread per colour; the palette index is wave-uniform so
// the palette is read through the scalar cache.  Same argmin + tie rules as the reference:
// strict '<' (lowest index wins, src/agmv_utils.c:810), palette0 on '<=' (src/agmv_utils.c:885).
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void nearest_in(const uint32_t* __restrict__ pal, int r, int g, int b,
                                           uint32_t& best, uint32_t& idx)
{
	best = 3u * 255u * 255u + 1u;
	idx = 0;
#pragma unroll 8
	for (int i = 0; i < 256; i++) {
		uint32_t p = pal[i];
		int dr = r - (int)((p >> 16) & 0xff), dg = g - (int)((p >> 8) & 0xff), db = b - (int)(p & 0xff);
		uint32_t d = (uint32_t)(dr * dr + dg * dg + db * db);
		if (d < best) { best = d; idx = (uint32_t)i; }
	}
}

__global__ __launch_bounds__(256) void k_lut_build(const uint32_t* __restrict__ pal, int mode512,
                                                   uint16_t* __restrict__ lut)
{
	uint32_t c = blockIdx.x * 256u + threadIdx.x;
	int r = (int)(c >> 16), g = (int)((c >> 8) & 0xff), b = (int)(c & 0xff);
	uint32_t d0, i0;
	nearest_in(pal, r, g, b, d0, i0);
	uint32_t e = i0;
	if (mode512) {
		uint32_t d1, i1;
		nearest_in(pal + 256, r, g, b, d1, i1);
		if (!(d0 <= d1)) e = 0x100u | i1;
	}
	lut[lut_index(c)] = (uint16_t)e;
}

// K0b: bit (e2) of row (e1) = palette colours of entries e1 and e2 are within +-2 on R, G and B.
__device__ __forceinline__ bool within2(uint32_t a, uint32_t b)
{
	int dr = (int)((a >> 16) & 0xff) - (int)((b >> 16) & 0xff);
	int dg = (int)((a >> 8) & 0xff) - (int)((b >> 8) & 0xff);
	int db = (int)(a & 0xff) - (int)(b & 0xff);
	return (unsigned)(dr + 2) <= 4u && (unsigned)(dg + 2) <= 4u && (unsigned)(db + 2) <= 4u;
}

__global__ __launch_bounds__(256) void k_mtx_build(const uint32_t* __restrict__ pal, uint32_t* __restrict__ mtx)
{
	uint32_t t = blockIdx.x * 256u + threadIdx.x;     // 512 rows * MROW words
	if (t >= 512u * MROW) return;
	uint32_t row = t / MROW, word = t % MROW, bits = 0;
	if (word < 16) {
		uint32_t a = pal[row];
		for (uint32_t k = 0; k < 32; k++)
			bits |= (within2(a, pal[word * 32 + k]) ? 1u : 0u) << k;
	}
	mtx[t] = bits;
}

__global__ __launch_bounds__(256) void k_quantise(const uint32_t* __restrict__ pix, size_t n,
                                                  const uint16_t* __restrict__ lut, uint16_t* __restrict__ out)
{
	size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	size_t stride = (size_t)gridDim.x * 256;
	for (; i < n; i += stride) out[i] = lut[lut_index(pix[i])];
}

// K0c: pattern dithering in place (include/agmv.h, "pattern dithering", holds the definition).  One lane = one pixel, neighbouring
// lanes neighbouring pixels of a row: their colours are close, so their look-ups -- the early ones above all -- fall into the same
// 128-byte lines (4x4x4 cubes) of the table.  A pixel costs 16 DEPENDENT look-ups (candidate i is found at the pixel plus the error
// the candidates before it left), so the kernel is bound by their latency and wants every wave the CU can hold: 256 lanes, 4 KB of
// LDS, no array indexed at run time (the candidate loop and the sort are unrolled over 16 registers).  The palette and the sort keys
// of its 512 entries sit side by side in LDS: one 8-byte per-lane read per candidate.
constexpr int DITHER_T = 256;
constexpr int DITHER_WG_PER_CU = 8;                           // 32 waves per CU, the hardware's limit, when the registers allow it
constexpr unsigned long long DITHER_B4 = 0x5D7F91B36E4CA280ull;   // nibble (y & 3) * 4 + (x & 3) of the threshold matrix

__global__ __launch_bounds__(DITHER_T) void k_dither(uint32_t* __restrict__ pix, uint32_t w, uint32_t npx, uint32_t n_frames, int strength,
                                                     const uint16_t* __restrict__ lut, const uint32_t* __restrict__ pal)
{
	__shared__ uint2 s_tab[512];                               // .x colour of the entry, .y its key: luma * 512 + entry
	for (uint32_t e = threadIdx.x; e < 512u; e += DITHER_T) {
		const uint32_t c = pal[e] & 0xFFFFFFu;
		s_tab[e] = make_uint2(c, (299u * (c >> 16) + 587u * ((c >> 8) & 255u) + 114u * (c & 255u)) * 512u + e);
	}
	__syncthreads();
	const uint32_t stride = gridDim.x * DITHER_T;
	for (uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
		uint32_t* __restrict__ fp = pix + (size_t)f * npx;
		for (uint32_t p = blockIdx.x * DITHER_T + threadIdx.x; p < npx; p += stride) {   // p < 2^31, stride <= 2^24: no wrap
			const uint32_t px = fp[p];
			const int r = (int)((px >> 16) & 255u), g = (int)((px >> 8) & 255u), b = (int)(px & 255u);
			int ar = 0, ag = 0, ab = 0;                        // the error so far, |.| <= 16 * 255
			uint32_t k[16];
#pragma unroll
			for (int i = 0; i < 16; i++) {
				const int cr = min(max(r + (__mul24(ar, strength) >> 6), 0), 255);
				const int cg = min(max(g + (__mul24(ag, strength) >> 6), 0), 255);
				const int cb = min(max(b + (__mul24(ab, strength) >> 6), 0), 255);
				const uint32_t e = lut[lut_index((uint32_t)(cr << 16 | cg << 8 | cb))] & 511u;
				const uint2 t = s_tab[e];
				ar += r - (int)(t.x >> 16); ag += g - (int)((t.x >> 8) & 255u); ab += b - (int)(t.x & 255u);
				k[i] = t.y;
			}
			// the 16 keys in ascending order: Batcher's odd-even merge sort, 63 compare-exchanges on registers
#define CE(a, b) { const uint32_t lo_ = min(k[a], k[b]), hi_ = max(k[a], k[b]); k[a] = lo_; k[b] = hi_; }
			CE(0, 1) CE(2, 3) CE(4, 5) CE(6, 7) CE(8, 9) CE(10, 11) CE(12, 13) CE(14, 15)
			CE(0, 2) CE(1, 3) CE(4, 6) CE(5, 7) CE(8, 10) CE(9, 11) CE(12, 14) CE(13, 15)
			CE(1, 2) CE(5, 6) CE(9, 10) CE(13, 14) CE(0, 4) CE(1, 5) CE(2, 6) CE(3, 7)
			CE(8, 12) CE(9, 13) CE(10, 14) CE(11, 15) CE(2, 4) CE(3, 5) CE(10, 12) CE(11, 13)
			CE(1, 2) CE(3, 4) CE(5, 6) CE(9, 10) CE(11, 12) CE(13, 14) CE(0, 8) CE(1, 9)
			CE(2, 10) CE(3, 11) CE(4, 12) CE(5, 13) CE(6, 14) CE(7, 15) CE(4, 8) CE(5, 9)
			CE(6, 10) CE(7, 11) CE(2, 4) CE(3, 5) CE(6, 8) CE(7, 9) CE(10, 12) CE(11, 13)
			CE(1, 2) CE(3, 4) CE(5, 6) CE(7, 8) CE(9, 10) CE(11, 12) CE(13, 14)
#undef CE
			const uint32_t y = p / w, x = p - y * w;           // the position inside the frame
			const uint32_t t = (uint32_t)(DITHER_B4 >> (((y & 3u) * 4u + (x & 3u)) * 4u)) & 15u;
			uint32_t key = k[0];
#pragma unroll
			for (int i = 1; i < 16; i++) key = t == (uint32_t)i ? k[i] : key;
			fp[p] = s_tab[key & 511u].x;
		}
	}
}

// ----------------------------------------------------------------------------------------------
// K1: fused encode
// ----------------------------------------------------------------------------------------------
struct EncArgs {
	const uint32_t* pix;
	uint8_t* out;
	uint32_t* sizes;
	const uint16_t* lut;
	const uint32_t* mtx;
	unsigned long long* status;
	uint32_t* ctrl;
	const uint16_t* ientries_in;    // entries of the GOP's I-frame when the batch starts inside a GOP
	uint16_t* ientries_out;         // receives the entries of the batch's last I-frame (never the buffer read above)
	unsigned long long out_stride;
	uint32_t n_frames, w, h, bw, nblk, tpf, first_fc, phase, n_groups, last_iframe, total_tiles;
};

// decoupled look-back over the tiles of one frame (run by ONE wave; returns the exclusive
// prefix of `tile`).  Status words are single 8-byte {tag,value} granules read/written with
// relaxed agent-scope atomics (sc1), so no fence is needed (the data is the flag).
// Forward progress: tiles are handed out by a ticket counter, so every predecessor of a
// running tile is itself running or finished.  Spins are bounded; on timeout ctrl[1] is set.
// `pre` is the first window's status word, loaded one frame earlier (latency hidden).
__device__ __forceinline__ unsigned long long st_load(unsigned long long* st, int idx)
{
	return idx >= 0 ? __hip_atomic_load(st + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ST_PREFIX;
}

__device__ __forceinline__ uint32_t lookback(unsigned long long* st, int tile, int lane, uint32_t* ctrl,
                                             unsigned long long pre)
{
	uint32_t excl = 0;
	int j = tile - 1;
	unsigned long long v = pre;
	for (;;) {
		const int idx = j - lane;
		unsigned spins = 0;
		while (!__all((v >> 32) != 0)) {
			__builtin_amdgcn_s_sleep(1);
			if (++spins > (1u << 22)) {
				if (lane == 0) atomicExch(ctrl + 1, 1u);
				return excl;
			}
			v = st_load(st, idx);
		}
		const uint32_t val = (uint32_t)v;
		const unsigned long long pm = __ballot((v >> 32) == 2);
		if (pm) {
			const int first = __ffsll((long long)pm) - 1;
			excl += wave_sum(lane <= first ? val : 0u);
			return excl;
		}
		excl += wave_sum(val);
		j -= 64;
		v = st_load(st, j - lane);
	}
}

constexpr int WBLK = 64;                                       // blocks per wave = slice of the workgroup tile
constexpr size_t CTRL_BYTES = 1024;                            // dwords: [0] ticket, [1] error; the rest is spare here (the experiment builds kept as patches under profiles/ use [32..42])

// K1.  Barrier-free dataflow form.  One workgroup = one tile of ENC_T consecutive 4x4 blocks (ENC_WAVES waves x 64
// blocks), one lane = one block for classification/emission, carried through the <=4 frames of its GOP.  The stream of
// (tile, frame) items a workgroup processes is ONE software pipeline that runs across tile switches; the waves of a
// workgroup never meet at a barrier inside it -- they exchange single tagged LDS words:
//   item `it`, every wave:  (Q) quantise with lane = (block, row): wide row loads, each LUT gather instruction covers a
//                               64x4-pixel patch; entries transposed to lane = block through the wave's own stage slot
//                           prefetch of the next item's pixels (next frame, or the first frame of the NEXT tile, whose
//                               ticket was drawn one tile earlier)
//                           (C) classify FILL / COPY / NORMAL, wave scan of the byte lengths -> wsum[it][wave];
//                               the LAST wave to arrive (LDS counter) adds the tile up and publishes the aggregate
//                           (E) emit bytes into the wave's OWN stage slot (offsets inside the wave only)
//                           copy-out of item it-1 from its own slot, at gbase[it-1][wave]
//   item `it`, duty wave (rotating): decoupled look-back of item it-1 across tiles (status window prefetched ahead
//                               of the look-ups), then gbase[it-1][w] = tile offset + bytes of the lower waves.
// Waves therefore drift apart by up to ~1.5 items, and the phases (look-up issue, look-up wait, LDS, VALU) of the
// waves sharing a SIMD interleave instead of lining up behind a barrier.  Control words live in 8 slots (it & 7): a
// wave can finish item `it` only after gbase[it-1] exists (it waits for that word even when it has no bytes to copy),
// i.e. after EVERY wave has published wsum[it-1]; so when a slot is rewritten for item it+1 all waves have finished
// item it-2 and with it every read of item it-3's words (4 slots would do).
constexpr int DF_SLOTS = 8;
constexpr int WSLOT = 16 + WBLK * 33 + 16;                     // a wave's stage slot: front pad + worst case + tail pad
static_assert(WSLOT % 16 == 0 && WSLOT >= 16 + WBLK * 16 * 2, "slot alignment / transpose scratch");
constexpr int C_WSUM = 0;                                      // [slot][wave]      tag<<16 | bytes of the wave
constexpr int C_ARRIVE = C_WSUM + DF_SLOTS * ENC_WAVES;        // [slot]            waves that have published wsum
constexpr int C_TTOTAL = C_ARRIVE + DF_SLOTS;                  // [slot]            tag<<16 | bytes of the tile
constexpr int C_GBASE = C_TTOTAL + DF_SLOTS;                   // [slot][wave][2]   frame byte offset of the wave, tag
constexpr int C_TICKET = C_GBASE + DF_SLOTS * ENC_WAVES * 2;   // [slot][2]         ticket of tile sequence number s, s
constexpr int C_END = C_TICKET + DF_SLOTS * 2;
constexpr size_t ENC_LDS_EXTRA = 2 * ENC_WAVES * WSLOT + C_END * 4;

typedef uint16_t __attribute__((aligned(1))) u16u;          // byte-aligned 16/32-bit LDS stores (DS unaligned mode)
typedef uint32_t __attribute__((aligned(1))) u32u;
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) uint32_t lds_u32;   // explicit LDS pointers: ds_read / ds_write, never flat
__device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) { return *(const volatile lds_u32*)p; }
__device__ __forceinline__ void lds_st(uint32_t* p, uint32_t v) { *(volatile lds_u32*)p = v; }

// Stores the compiler does not track: hipcc guards the data registers of a store it knows about with s_waitcnt vmcnt(0) before
// they are written again, i.e. it waits for the write to be ACKNOWLEDGED (1-2 us for the status words, which go to the fabric)
// -- three such waits per item in the look-back / copy-out sequence.  The hardware reads the data of a 4- / 8-byte store when
// it issues it, and nothing in the wave waits for these stores, so they go out as asm (the compiler's waits for LOADS can only
// become longer by it, never shorter: the memory counter retires in order).
__device__ __forceinline__ void st_store_untracked(unsigned long long* p, unsigned long long v)
{
	asm volatile("global_store_dwordx2 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory");      // = a relaxed agent-scope atomic store
}
__device__ __forceinline__ void store32_untracked(uint32_t* p, uint32_t v)
{
	asm volatile("global_store_dword %0, %1, off" :: "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store8_untracked(uint8_t* p, uint32_t v)
{
	asm volatile("global_store_byte %0, %1, off" :: "v"(p), "v"(v) : "memory");
}
// wave_copy_own with untracked stores
__device__ __forceinline__ void wave_copy_own_u(const uint8_t* slot, uint8_t* gdst, uint32_t total, int lane)
{
	const uint32_t s = (uint32_t)((uintptr_t)gdst & 3u);
	uint32_t head = s ? 4u - s : 0u;
	if (head > total) head = total;
	const uint32_t nbody = (total - head) >> 2, tail = (total - head) & 3u;
	const uint8_t* sb = slot + 16 + head;
	uint8_t* gb = gdst + head;
	for (uint32_t d = lane; d < nbody; d += 64) store32_untracked((uint32_t*)(gb + 4u * d), *(const u32u*)(sb + 4u * d));
	if ((uint32_t)lane < head) store8_untracked(gdst + lane, slot[16 + lane]);
	const uint32_t tl = (uint32_t)lane - 8u;
	if (tl < tail) store8_untracked(gb + 4u * nbody + tl, sb[4u * nbody + tl]);
}
// look-back of k_encode's duty wave.  The common case -- every status word of the first window is published and one of them is a
// prefix -- is straight-line code on the window the caller loaded long ago (`pre`); anything else goes through the general
// loop above, out of line: inlined, its conditional reloads leave the compiler unsure whether a load is still pending at
// every later write of those registers, and it answers each with s_waitcnt vmcnt(0) -- which at that point also waits for
// the status / copy-out STORES in flight to be acknowledged (1-2 us each, three times per item).
__device__ __noinline__ uint32_t lookback_slow(unsigned long long* st, int tile, int lane, uint32_t* ctrl, unsigned long long pre)
{
	return lookback(st, tile, lane, ctrl, pre);
}
__device__ __forceinline__ uint32_t lookback_w(unsigned long long* st, int tile, int lane, uint32_t* ctrl, unsigned long long pre)
{
	const uint32_t tag = (uint32_t)(pre >> 32), val = (uint32_t)pre;
	const unsigned long long pm = __ballot(tag == 2u);
	if (__all(tag != 0u) && pm != 0) {
		const int first = __ffsll((long long)pm) - 1;
		return wave_sum(lane <= first ? val : 0u);
	}
	return lookback_slow(st, tile, lane, ctrl, pre);
}
// status word of segment idx without a branch around the load (idx < 0, before the frame, reads word 0)
__device__ __forceinline__ unsigned long long st_load_raw(unsigned long long* st, int idx)     // the caller substitutes ST_PREFIX for idx < 0
{
	return __hip_atomic_load(st + (idx >= 0 ? idx : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// wave-uniform bounded spin until the word at p satisfies (v >> shift) == tag; returns the word
__device__ __forceinline__ uint32_t lds_wait(const uint32_t* p, uint32_t tag, int shift, uint32_t* ctrl, int lane)
{
	uint32_t v = __builtin_amdgcn_readfirstlane(lds_ld(p));
	unsigned spins = 0;
	while ((v >> shift) != tag) {
		__builtin_amdgcn_s_sleep(1);
		if (++spins > (1u << 24)) {                          // a legitimate wait is microseconds; the bound is above the look-back's (1 << 22 polls of global memory), which this wait can transitively wait for
			if (lane == 0) atomicExch(ctrl + 1, 2u);
			break;
		}
		v = __builtin_amdgcn_readfirstlane(lds_ld(p));
	}
	return v;
}

// copy the `total` bytes staged at slot+16 to gdst (one wave): dword stores on GLOBAL-aligned dwords, read from the
// stage at byte-granular LDS addresses (DS unaligned mode); the <= 3 bytes before the first and after the last aligned
// dword (which share a dword with the neighbouring waves / tiles) go out as byte stores from eight lanes in one step
__device__ __forceinline__ void wave_copy_own(const uint8_t* slot, uint8_t* gdst, uint32_t total, int lane)
{
	const uint32_t s = (uint32_t)((uintptr_t)gdst & 3u);
	uint32_t head = s ? 4u - s : 0u;
	if (head > total) head = total;
	const uint32_t nbody = (total - head) >> 2, tail = (total - head) & 3u;
	const uint8_t* sb = slot + 16 + head;
	uint8_t* gb = gdst + head;
	for (uint32_t d = lane; d < nbody; d += 64) *(uint32_t*)(gb + 4u * d) = *(const u32u*)(sb + 4u * d);
	if ((uint32_t)lane < head) gdst[lane] = slot[16 + lane];
	const uint32_t tl = (uint32_t)lane - 8u;
	if (tl < tail) gb[4u * nbody + tl] = sb[4u * nbody + tl];
}

// The two block tests of one 4x4 block (entries packed two per register): acc1 collects one matrix bit per pixel
// against the block's top-left entry (row0), acc2 -- P-frames only -- against the I-frame's entry of the same pixel.
template <bool M512, bool PFRAME>
__device__ __forceinline__ void block_tests(const uint32_t (&ep)[8], const uint32_t (&ip)[8], const uint32_t* s_mtx,
                                            uint32_t row0, uint32_t& acc1, uint32_t& acc2, uint32_t& nesc)
{
	// (requesting all 16 / 32 matrix words before the first use -- 110 VGPRs instead of 96 -- measured the same: 0.723 vs
	//  0.728 ms per 256 frames; the LDS round trips of one wave are covered by the other three of its SIMD)
#pragma unroll
	for (int m = 0; m < 8; m++) {
		const uint32_t p = ep[m], a5 = (p >> 5) & 0x7ffu, b5 = p >> 21, bh = p >> 16;
		const uint32_t wa = s_mtx[row0 + a5], wb = s_mtx[row0 + b5];
		acc1 = __builtin_amdgcn_alignbit(wa >> (p & 31u), acc1, 1);
		acc1 = __builtin_amdgcn_alignbit(wb >> (bh & 31u), acc1, 1);
		if (M512) nesc += ((p & 0xffu) >= 127u ? 1u : 0u) + ((bh & 0xffu) >= 127u ? 1u : 0u);
		if (PFRAME) {
			const uint32_t q = ip[m];
			const uint32_t va = s_mtx[(q & 0xffffu) * MROW + a5], vb = s_mtx[(q >> 16) * MROW + b5];
			acc2 = __builtin_amdgcn_alignbit(va >> (p & 31u), acc2, 1);
			acc2 = __builtin_amdgcn_alignbit(vb >> (bh & 31u), acc2, 1);
		}
	}
}

struct EncGeo {
	uint32_t tile, wbase, wb_c, wbx, wby;                      // wave-uniform
	int f_lo, f_hi, path;
	uint32_t poff, p0b, qx0;                                   // per lane
	bool valid;
};

// ENTRIES: the input planes hold ENTRIES (one per 32-bit word, pal_num << 8 | index) instead of pixels -- the table look-ups
// are skipped and classification + emission run on the caller's entries (AGMV_AssembleIFrameBitstream /
// AGMV_AssemblePFrameBitstream on a given AGMV_ENTRY plane, src/agmv_encode.c:354-527).
typedef uint32_t px4 __attribute__((ext_vector_type(4)));   // a native vector (HIP's uint4 is a struct: asm cannot tie it to a register tuple)
template <bool M512, bool ENTRIES>
__global__ __launch_bounds__(ENC_T, ENC_WPE) void k_encode(EncArgs A)
{
	constexpr int NROWS = M512 ? 512 : 256;
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	uint32_t* s_mtx = (uint32_t*)smem;                         // NROWS * MROW dwords
	uint8_t* s_stage0 = smem + NROWS * MROW * 4;               // [2][ENC_WAVES] stage slots
	uint32_t* s_ctl = (uint32_t*)(s_stage0 + 2 * ENC_WAVES * WSLOT);

	const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const uint32_t npx = A.w * A.h;
	const uint32_t jb = lane >> 2, prow = lane & 3;            // quantise phase: lane = (block jb of 16, row prow)
	const __amdgpu_buffer_rsrc_t lut_rs = __builtin_amdgcn_make_buffer_rsrc((void*)A.lut, 0, (int)(LUT_ENTRIES * 2u), 0x00020000);

	for (int i = tid; i < NROWS * MROW; i += ENC_T) s_mtx[i] = A.mtx[i];
	for (int i = tid; i < C_END; i += ENC_T) s_ctl[i] = 0;
	__syncthreads();
	if (tid == 0) s_ctl[C_TICKET] = atomicAdd(A.ctrl, 1u);
	__syncthreads();                                           // the only workgroup barriers of the kernel

	auto locate = [&](const EncGeo& g, uint32_t B, uint32_t& qx, uint32_t& qy) {   // block index (>= wb_c) -> block column / row
		if (B >= A.nblk) B = A.nblk - 1;                       // blocks past the frame re-use the last valid one
		qx = g.wbx + (B - g.wb_c); qy = g.wby;
		while (qx >= A.bw) { qx -= A.bw; qy++; }
	};
	// tile-major ticket order: consecutive tickets are the SAME tile of different GOPs, so a tile's predecessors (same
	// GOP, lower tile) are n_groups tickets older -> mostly finished when the look-back reads them.
	// geometry: ONE integer division per wave (of its first block, wave-uniform); lane positions follow by adding and
	// wrapping at the end of a block row (no per-lane divisions)
	auto setup = [&](uint32_t t, EncGeo& g) {
		g.tile = t / A.n_groups;
		const uint32_t group = t - g.tile * A.n_groups;
		g.f_lo = group == 0 ? 0 : (int)(group * 4 - A.phase);
		g.f_hi = (int)(group * 4 - A.phase) + 4;
		if (g.f_hi > (int)A.n_frames) g.f_hi = (int)A.n_frames;
		g.wbase = g.tile * ENC_T + wave * WBLK;                // first block of this wave
		g.wb_c = g.wbase < A.nblk ? g.wbase : A.nblk - 1;
		g.wby = __builtin_amdgcn_readfirstlane(g.wb_c / A.bw); g.wbx = g.wb_c - g.wby * A.bw;
		// lane-as-block view (classification, emission, I-frame entry plane)
		const uint32_t blk = g.wbase + lane;
		g.valid = blk < A.nblk;
		uint32_t bx, by;
		locate(g, blk, bx, by);
		g.poff = by * 4 * A.w + bx * 4;                        // top-left pixel of the block
		// quantise view, lane = (block, row): load i (0..3) fetches row `prow` (16 bytes) of block wbase + 16i + jb, so
		// one instruction reads four 256-byte row segments of 16 adjacent blocks and each of its four pixel columns is
		// a 64x4-pixel patch for the LUT gather.  A wave inside one block row uses immediate offsets, one crossing a
		// single row boundary adds 3*w past it, anything else locates each of its four blocks.
		uint32_t qy0;
		locate(g, g.wbase + jb, g.qx0, qy0);
		g.p0b = ((qy0 * 4 + prow) * A.w + g.qx0 * 4) * 4u;
		g.path = (g.wbase + WBLK > A.nblk || g.wbx + WBLK > 2 * A.bw) ? 2 : (g.wbx + WBLK > A.bw ? 1 : 0);
	};
	auto load_frame = [&](const EncGeo& g, const uint32_t* fp, px4 (&dst)[4]) {
		const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)fp, 0, (int)(npx * 4u), 0x00020000);
		const uint32_t w3b = 12u * A.w;
		if (g.path == 0) {
#pragma unroll
			for (int i = 0; i < 4; i++) dst[i] = __builtin_bit_cast(px4, __builtin_amdgcn_raw_buffer_load_b128(rs, g.p0b + 256 * i, 0, ENC_PIXAUX));
		} else if (g.path == 1) {
#pragma unroll
			for (int i = 0; i < 4; i++)
				dst[i] = __builtin_bit_cast(px4, __builtin_amdgcn_raw_buffer_load_b128(rs, g.p0b + 256 * i + (g.qx0 + 16 * i >= A.bw ? w3b : 0u), 0, ENC_PIXAUX));
		} else {
#pragma unroll
			for (int i = 0; i < 4; i++) {
				uint32_t qx, qy;
				locate(g, g.wbase + jb + 16 * i, qx, qy);
				dst[i] = __builtin_bit_cast(px4, __builtin_amdgcn_raw_buffer_load_b128(rs, ((qy * 4 + prow) * A.w + qx * 4) * 4u, 0, ENC_PIXAUX));
			}
		}
	};

	// Two cursors walk the workgroup's sequence of (tile, frame) items: `cur` is the item being encoded, `pf` the item whose
	// pixels are requested next, ENC_PFDEPTH items ahead (every item's pixels are in flight for that many item times).  A
	// cursor that leaves its tile takes the ticket of the next one from the LDS slot of that tile's sequence number; wave 0
	// draws a tile's ticket when its OWN prefetch cursor enters the tile before it and publishes it behind its next look-ups.
	struct Cursor { EncGeo g; int f; uint32_t seq; bool have; };
	Cursor cur, pf;
	uint32_t tk = 0, tk_seq = 0;
	bool tk_pending = false;
	auto draw_ticket = [&](uint32_t for_seq) {
		if (wave == 0) {
			if (lane == 0) tk = atomicAdd(A.ctrl, 1u);
			tk_seq = for_seq; tk_pending = true;
		}
	};
	auto publish_ticket = [&]() {
		if (wave == 0 && tk_pending) {
			const uint32_t tkv = __builtin_amdgcn_readfirstlane(tk);
			if (lane == 0) {
				uint32_t* tw = &s_ctl[C_TICKET + (tk_seq & (DF_SLOTS - 1)) * 2];
				lds_st(tw, tkv);
				asm volatile("" ::: "memory");
				lds_st(tw + 1, tk_seq);
			}
			tk_pending = false;
		}
	};
	auto advance = [&](Cursor& c, bool lead) -> bool {         // to the next item; true when that is the first item of a tile
		if (c.f + 1 < c.g.f_hi) { c.f++; return false; }
		if (lead) publish_ticket();                            // wave 0 is about to wait for the ticket it drew itself
		const uint32_t* tw = &s_ctl[C_TICKET + ((c.seq + 1) & (DF_SLOTS - 1)) * 2];
		lds_wait(tw + 1, c.seq + 1, 0, A.ctrl, lane);
		asm volatile("" ::: "memory");
		const uint32_t nt = __builtin_amdgcn_readfirstlane(lds_ld(tw));
		c.seq++;
		c.have = nt < A.total_tiles;
		if (c.have) {
			setup(nt, c.g);
			c.f = c.g.f_lo;
			if (lead) draw_ticket(c.seq + 1);
		}
		return true;
	};
	{
		const uint32_t ticket = __builtin_amdgcn_readfirstlane(lds_ld(&s_ctl[C_TICKET]));
		cur.seq = 0; cur.f = 0;
		cur.have = ticket < A.total_tiles;
		if (cur.have) { setup(ticket, cur.g); cur.f = cur.g.f_lo; }
	}
	pf = cur;
	if (pf.have) draw_ticket(1);
	uint32_t it = 0;                                           // item number (tags / slots)
	bool new_tile = true;
	uint32_t ip[8];                                            // the GOP's I-frame entries of this block, two u16 per register
	px4 pxs[ENC_PFDEPTH][4];
#pragma unroll
	for (int d = 0; d < ENC_PFDEPTH; d++)
		if (pf.have) { load_frame(pf.g, A.pix + (size_t)pf.f * npx, pxs[d]); advance(pf, true); }
	bool have_prev = false;                                    // item it-1: tile, frame, bytes of this wave
	uint32_t p_tile = 0, p_len = 0;
	int p_f = 0;
	unsigned long long pre_next = ST_PREFIX;                   // the status window the NEXT item's duty wave will look back through

	auto body = [&](px4 (&px)[4]) -> bool {                 // one item: consumes px and refills it with the item ENC_PFDEPTH ahead
		EncGeo& g = cur.g;
		const int f = cur.f;
		const uint32_t slot = it & (DF_SLOTS - 1), tag = (it + 1) & 0xffffu;
		const uint32_t pslot = (it - 1) & (DF_SLOTS - 1), ptag = it & 0xffffu;
		// (L) the look-back of item it-1 is the duty of ONE wave (rotating).  Its status window was requested at the END of
		// item it-1, behind that item's pixel prefetch (pre_next): the status words bypass the caches -- a fabric round trip,
		// several times the latency of a table look-up -- and the memory counter retires in order, so requested here, ahead
		// of the look-ups, the window would hold back every entry of the duty wave, and with it gbase[] for all eight waves
		const bool duty = have_prev && wave == (int)(it % ENC_WAVES);
		const unsigned long long pre = pre_next;
		auto resolve_prev = [&]() {                            // tile offset of item it-1, usize of the frame, gbase[]
			unsigned long long* st = A.status + (size_t)p_f * A.tpf;
			uint32_t excl = 0;
			// (straight-line look-back on the window loaded earlier; the general loop is out of line -- inlined, its conditional
			//  reloads make the compiler drain the memory counter before gbase[] is published, i.e. the seven other waves of the
			//  workgroup would wait for the acknowledgement of this wave's status stores: a fabric round trip per item)
			if (p_tile != 0) excl = lookback_w(st, (int)p_tile, lane, A.ctrl, pre);
			const uint32_t tot = lds_wait(&s_ctl[C_TTOTAL + pslot], ptag, 16, A.ctrl, lane) & 0xffffu;
			// every wave of the tile has published its byte count (the tile total exists): exclusive scan over the waves.
			// gbase[] goes out FIRST: it is what the other waves wait for
			const uint32_t ws = lane < ENC_WAVES ? (lds_ld(&s_ctl[C_WSUM + pslot * ENC_WAVES + lane]) & 0xffffu) : 0u;
			uint32_t inc = ws;
			inc += dpp_or0<0x111, 0xF>(inc);                    // the waves sit in the first lanes of row 0
			if (ENC_WAVES > 2) inc += dpp_or0<0x112, 0xF>(inc);
			if (ENC_WAVES > 4) inc += dpp_or0<0x114, 0xF>(inc);
			if (ENC_WAVES > 8) inc += dpp_or0<0x118, 0xF>(inc);
			if (lane < ENC_WAVES) {
				uint32_t* gb = &s_ctl[C_GBASE + (pslot * ENC_WAVES + lane) * 2];
				lds_st(gb, excl + inc - ws);
				asm volatile("" ::: "memory");
				lds_st(gb + 1, it);
			}
			if (lane == 0) {
				if (p_tile != 0) st_store_untracked(st + p_tile, ST_PREFIX | (unsigned long long)(excl + tot));
				if (p_tile == A.tpf - 1) store32_untracked(A.sizes + p_f, excl + tot);   // usize of the frame
			}
		};
		auto copy_out_prev = [&]() {
			// EVERY wave waits here, also one with nothing to copy: this wait is what bounds the drift between the waves
			// (see the header comment) -- a wave of blocks past the end of the frame must not run rounds ahead and recycle
			// control slots the others still read
			const uint32_t* gb = &s_ctl[C_GBASE + (pslot * ENC_WAVES + wave) * 2];
			lds_wait(gb + 1, it, 0, A.ctrl, lane);
			asm volatile("" ::: "memory");
			if (p_len == 0) return;
			const uint32_t base = __builtin_amdgcn_readfirstlane(lds_ld(gb));
			wave_copy_own_u(s_stage0 + (((it - 1) & 1) * ENC_WAVES + wave) * WSLOT, A.out + (size_t)p_f * A.out_stride + base, p_len, lane);
		};

		if (!cur.have) {                                       // final drain: item it-1 is the last one
			if (have_prev) {
				if (duty) resolve_prev();
				copy_out_prev();
			}
			return false;
		}

		const bool is_i = ((A.first_fc + f) & 3u) == 0;
		uint8_t* wslot = s_stage0 + ((it & 1) * ENC_WAVES + wave) * WSLOT;   // free since this wave's copy-out of item it-2
		uint8_t* scratch = wslot + 16;
		if (new_tile) {
			if (((A.first_fc + g.f_lo) & 3u) != 0) {           // GOP started in an earlier batch
#pragma unroll
				for (int r = 0; r < 4; r++) {
					const uint2 q = *(const uint2*)(A.ientries_in + g.poff + r * A.w);
					ip[2 * r] = q.x; ip[2 * r + 1] = q.y;
				}
			} else {
#pragma unroll
				for (int m = 0; m < 8; m++) ip[m] = 0;
			}
		}
		// ---- the pixels of the item ENC_PFDEPTH ahead, into the registers this item's pixels leave
		auto prefetch_next = [&]() {
			asm volatile("" ::: "memory");
			publish_ticket();
			if (pf.have) { load_frame(pf.g, A.pix + (size_t)pf.f * npx, px); advance(pf, true); }
		};
#if ENC_PRIO
		__builtin_amdgcn_s_setprio(ENC_PRIO);
#endif
		uint32_t ep[8], e0, len;
		bool copy, fill;
		{
		// ---- (Q) colour -> entry through the exact table, lane = (block, row)
		uint32_t eq[16];
		const uint32_t pxv[16] = {px[0].x, px[0].y, px[0].z, px[0].w, px[1].x, px[1].y, px[1].z, px[1].w,
		                          px[2].x, px[2].y, px[2].z, px[2].w, px[3].x, px[3].y, px[3].z, px[3].w};
#pragma unroll
		for (int k = 0; k < 16; k++) {
			if (ENTRIES) eq[k] = pxv[k] & (M512 ? 0x1FFu : 0xFFu);
			else eq[k] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(lut_rs, lut_offset(pxv[k]), 0, ENC_LUTAUX);
		}
#if ENC_PRIO
		__builtin_amdgcn_s_setprio(0);
#endif
		// [block][pixel] u16 table in the wave's scratch; a lane writes its row: 8 bytes at i*512 + lane*8
#pragma unroll
		for (int i = 0; i < 4; i++) {
			uint2 q;
			q.x = eq[i * 4 + 0] | (eq[i * 4 + 1] << 16);
			q.y = eq[i * 4 + 2] | (eq[i * 4 + 3] << 16);
			*(uint2*)(scratch + i * 512 + lane * 8) = q;
		}
		if (duty) resolve_prev();
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		// ---- transpose: lane = block reads its 16 entries (32 contiguous bytes), kept PACKED two per register
		{
			const uint4 lo = *(const uint4*)(scratch + lane * 32), hi = *(const uint4*)(scratch + lane * 32 + 16);
			ep[0] = lo.x; ep[1] = lo.y; ep[2] = lo.z; ep[3] = lo.w; ep[4] = hi.x; ep[5] = hi.y; ep[6] = hi.z; ep[7] = hi.w;
		}
		// ---- (C) block tests. count1 = CompareIFrameBlock vs the top-left entry colour
		// (src/agmv_encode.c:302-352), count2 = ComparePFrameBlock vs the I-frame entries
		// (src/agmv_encode.c:240-300); one matrix bit per pixel (the shifter uses the low 5 bits of its amount).
		e0 = ep[0] & 0xffffu;
		const uint32_t row0 = e0 * MROW;
		uint32_t acc1 = 0, acc2 = 0, nesc = 0;
		// (the I / P choice is wave-uniform: unswitched by hand -- with the test inside the unrolled loop the compiler
		//  branches per entry pair and waits for each pair's two matrix words before it issues the next reads)
		if (is_i) block_tests<M512, false>(ep, ip, s_mtx, row0, acc1, acc2, nesc);
		else block_tests<M512, true>(ep, ip, s_mtx, row0, acc1, acc2, nesc);
		const uint32_t count1 = __popc(acc1), count2 = __popc(acc2);
		copy = !is_i && count2 >= COPY_COUNT;                  // COPY has priority, :465
		fill = !copy && count1 >= FILL_COUNT;
		if (copy) len = 1;
		else if (fill) len = M512 ? (2u + ((e0 & 0xffu) >= 127u ? 1u : 0u)) : 2u;
		else len = 17u + nesc;
		if (!g.valid) len = 0;
		}

		if (is_i) {                                            // iframe_entries = img_entry, :626-630
#pragma unroll
			for (int m = 0; m < 8; m++) ip[m] = ep[m];
			if (A.ientries_out && (uint32_t)f == A.last_iframe && g.valid) {
#pragma unroll
				for (int r = 0; r < 4; r++) {
					uint2 q;
					q.x = ep[2 * r]; q.y = ep[2 * r + 1];
					*(uint2*)(A.ientries_out + g.poff + r * A.w) = q;
				}
			}
		}

		// ---- byte offsets inside the wave; the last wave to arrive publishes the tile's aggregate
		const uint32_t incl = wave_incl_scan(len, lane);
		const uint32_t wtot = __builtin_amdgcn_readlane(incl, 63);
		uint32_t arrived = 0;
		if (lane == 63) {
			lds_st(&s_ctl[C_WSUM + slot * ENC_WAVES + wave], (tag << 16) | incl);
			asm volatile("" ::: "memory");
			arrived = atomicAdd(&s_ctl[C_ARRIVE + slot], 1u);
		}
		arrived = __builtin_amdgcn_readlane(arrived, 63);
		if (arrived == ENC_WAVES - 1) {
			const uint32_t ws = lane < ENC_WAVES ? (lds_ld(&s_ctl[C_WSUM + slot * ENC_WAVES + lane]) & 0xffffu) : 0u;
			const uint32_t total = wave_sum(ws);
			if (lane == 0) {
				lds_st(&s_ctl[C_ARRIVE + slot], 0u);
				__hip_atomic_store(A.status + (size_t)f * A.tpf + g.tile, (g.tile == 0 ? ST_PREFIX : ST_AGG) | total,
				                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				lds_st(&s_ctl[C_TTOTAL + slot], (tag << 16) | total);
			}
		}
		// ---- (E) emit this block's bytes into the wave's stage slot
		// Codes are built two at a time in packed 16-bit lanes and written as {code, index} byte PAIRS at byte-granular
		// LDS addresses (gfx950 runs DS in unaligned mode): when an entry has no escape byte its pair's second byte is
		// overwritten by the next pair, and the one byte a block may spill past its end is the next block's flag --
		// which is why the flags are written last.  The LDS unit executes a wave's writes in program order.
		if (g.valid) {
			uint8_t* sp = wslot + 16 + incl - len;
			if (!copy && !fill) {
				if (M512) {
					uint32_t n = 0;                                // escape bytes so far
#pragma unroll
					for (int m = 0; m < 8; m++) {
						const uint32_t p = ep[m], idx2 = p & 0x00FF00FFu;
						const u16x2 c2 = __builtin_elementwise_min(__builtin_bit_cast(u16x2, idx2), __builtin_bit_cast(u16x2, 0x007F007Fu));
						const uint32_t code2 = ((p >> 1) & 0x00800080u) | __builtin_bit_cast(uint32_t, c2);   // :395-401
						const uint32_t w = __builtin_amdgcn_perm(code2, p, 0x02060004u);   // code_lo, idx_lo, code_hi, idx_hi
						const uint32_t e2 = idx2 + 0x00810081u;    // bit 8 / bit 24: index >= 127
						*(u16u*)(sp + n + (1 + 2 * m)) = (uint16_t)w;
						n += (e2 >> 8) & 1u;
						*(u16u*)(sp + n + (2 + 2 * m)) = (uint16_t)(w >> 16);
						n += e2 >> 24;
					}
				} else {
#pragma unroll
					for (int m = 0; m < 4; m++)                    // :428-429
						*(u32u*)(sp + 1 + 4 * m) = __builtin_amdgcn_perm(ep[2 * m + 1], ep[2 * m], 0x06040200u);
				}
			} else if (fill) {
				if (M512) {
					const uint32_t idx = e0 & 0xffu, p7 = (e0 >> 1) & 0x80u;
					*(u16u*)(sp + 1) = (uint16_t)(p7 | (idx < 127u ? idx : 127u) | (idx << 8));   // :382-388
				} else {
					sp[1] = (uint8_t)e0;                           // :421
				}
			}
			asm volatile("" ::: "memory");
			sp[0] = copy ? COPY_FLAG : (fill ? FILL_FLAG : NORMAL_FLAG);
		}
		if (have_prev) copy_out_prev();
		prefetch_next();                                       // LAST in the item: any later wait of the item (the compiler places conservative ones at branch joins) would drain these loads -- requested right behind the entries they measured 0.98 against 0.72 ms per 256 frames

		// ---- next item
		have_prev = true; p_tile = g.tile; p_f = f; p_len = wtot;
		it++;
		pre_next = ST_PREFIX;
		if (wave == (int)(it % ENC_WAVES) && p_tile != 0) pre_next = st_load(A.status + (size_t)p_f * A.tpf, (int)p_tile - 1 - lane);
		new_tile = advance(cur, false);
		return true;
	};
	for (;;) {
#pragma unroll
		for (int d = 0; d < ENC_PFDEPTH; d++)
			if (!body(pxs[d])) goto done;
	}
done:;
}

// A spin of k_encode that ran into its bound leaves ctrl[1] != 0 and the kernel carries on with a wrong offset: the bytes of
// the batch are not to be used.  So that a caller who skips agmv_hip_check cannot take them for good ones, every size of
// the batch is then overwritten with 0xFFFFFFFF (no frame is that long: agmv_hip_max_usize < 2^32).
__global__ __launch_bounds__(64) void k_encode_verdict(const uint32_t* __restrict__ ctrl, uint32_t* __restrict__ sizes, uint32_t n_frames)
{
	if (ctrl[1] == 0) return;
	for (uint32_t f = threadIdx.x; f < n_frames; f += 64) sizes[f] = 0xFFFFFFFFu;
}

// E2 / E3 without the table: nearest colour / entry of n pixels by the reference's own search (src/agmv_utils.c:785-895).
// For the exported single-colour functions AGMV_FindNearestColor / AGMV_FindNearestEntry, whose palette argument changes from
// call to call: building a 2^24-entry table for one look-up would cost 2 ms.
__global__ __launch_bounds__(64) void k_nearest_direct(const uint32_t* __restrict__ pal, int mode512, const uint32_t* __restrict__ pix,
                                                       size_t n, uint16_t* __restrict__ out)
{
	const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
	if (i >= n) return;
	const uint32_t c = pix[i];
	const int r = (int)((c >> 16) & 0xff), g = (int)((c >> 8) & 0xff), b = (int)(c & 0xff);
	uint32_t d0, i0;
	nearest_in(pal, r, g, b, d0, i0);
	uint32_t e = i0;
	if (mode512) {
		uint32_t d1, i1;
		nearest_in(pal + 256, r, g, b, d1, i1);
		if (!(d0 <= d1)) e = 0x100u | i1;
	}
	out[i] = (uint16_t)e;
}

// E5 / E6 on 16 colour pairs: how many pairs are within +-2 on R, G and B (the predicate of AGMV_CompareIFrameBlock /
// AGMV_ComparePFrameBlock, src/agmv_encode.c:293, :345), for the exported single-block helpers.
__global__ __launch_bounds__(64) void k_within2_count(const uint32_t* __restrict__ ab, uint32_t* __restrict__ out)
{
	const int lane = threadIdx.x;
	const bool in = lane < 16 && within2(ab[lane], ab[16 + lane]);
	const unsigned long long m = __ballot(in);
	if (lane == 0) out[0] = (uint32_t)__popcll(m);
}

// ----------------------------------------------------------------------------------------------
// C-ABI
// ----------------------------------------------------------------------------------------------
// ----------------------------------------------------------------------------------------------
// Palette tables (colour -> entry table, +-2 bit matrix, palette) are read-only once built and identical for every
// context that holds the same palette on the same device -- the sequence drivers open two worker contexts per device
// besides the caller's.  They are shared: one 512 MiB allocation and one 2 ms table build per (device, palette).
// ----------------------------------------------------------------------------------------------
struct lut_share {
	int device, mode512, refs;
	uint32_t pal[512];
	uint16_t* d_lut;
	uint32_t* d_mtx;
	uint32_t* d_pal;
	hipEvent_t built;               // recorded behind the build kernels; a context on another stream waits for it
	lut_share* next;
};
static pthread_mutex_t g_lut_mu = PTHREAD_MUTEX_INITIALIZER;
static lut_share* g_luts = nullptr;

static void lut_release(lut_share* sh)                        // (device of the share is current)
{
	if (!sh) return;
	pthread_mutex_lock(&g_lut_mu);
	if (--sh->refs == 0) {
		for (lut_share** pp = &g_luts; *pp; pp = &(*pp)->next)
			if (*pp == sh) { *pp = sh->next; break; }
		(void)hipFree(sh->d_lut); (void)hipFree(sh->d_mtx); (void)hipFree(sh->d_pal);
		if (sh->built) (void)hipEventDestroy(sh->built);
		free(sh);
	}
	pthread_mutex_unlock(&g_lut_mu);
}

extern "C" int agmv_hip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" void agmv_hip_destroy(agmv_hip_ctx* c);
extern "C" agmv_hip_ctx* agmv_hip_create(int device)
{
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) {
		agmv_hip_err("agmv_hip: no HIP device available (%s); the AGMV hot path has no CPU fallback",
		             e == hipSuccess ? "device count 0" : hipGetErrorString(e));
		return nullptr;
	}
	if (device < 0 || device >= n) {
		agmv_hip_err("agmv_hip: device %d out of range (0..%d)", device, n - 1);
		return nullptr;
	}
	CKP(hipSetDevice(device));
	agmv_hip_ctx* c = (agmv_hip_ctx*)calloc(1, sizeof(*c));
	if (!c) { agmv_hip_err("agmv_hip: out of host memory"); return nullptr; }
	c->device = device;
	hipDeviceProp_t prop;
	hipError_t e2 = hipMalloc(&c->d_ctrl, CTRL_BYTES);
	// agmv_hip_check reads the error word on a context that has not encoded yet: hipMalloc hands back recycled memory as it is
	if (e2 == hipSuccess) e2 = hipMemset(c->d_ctrl, 0, CTRL_BYTES);
	if (e2 == hipSuccess) e2 = hipStreamSynchronize(nullptr);
	if (e2 == hipSuccess) e2 = hipGetDeviceProperties(&prop, device);
	if (e2 != hipSuccess) {                                    // nothing half-built is left behind
		agmv_hip_hip_failed("agmv_hip_create", e2, __FILE_NAME__, __LINE__);
		agmv_hip_destroy(c);
		return nullptr;
	}
	c->n_cu = prop.multiProcessorCount;
	// persistent grid of k_encode = the workgroups that are resident at once (2 per CU: 69 KB of LDS each)
	{
		int per_cu = 0;
		const size_t lds = (size_t)512 * MROW * 4 + ENC_LDS_EXTRA;
		(void)hipFuncSetAttribute((const void*)k_encode<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_encode<true, false>, ENC_T, lds) != hipSuccess || per_cu < 1) per_cu = 2;
		if (getenv("AGMV_HIP_DEBUG")) fprintf(stderr, "agmv_hip: k_encode: %d workgroup(s) of %d lanes resident per CU (%zu B of LDS each), %d CUs\n", per_cu, ENC_T, lds, c->n_cu);
		c->enc_grid = prop.multiProcessorCount * per_cu;
	}
	return c;
}

extern "C" void agmv_hip_destroy(agmv_hip_ctx* c)
{
	if (!c) return;
	(void)hipSetDevice(c->device);
	lut_release(c->share);
	(void)hipFree(c->d_ctrl);
	(void)hipFree(c->d_status); (void)hipFree(c->d_ient_tmp);
	(void)hipFree(c->d_nn_pal); (void)hipFree(c->d_nn_pix); (void)hipFree(c->d_nn_ent);
	if (c->ev_enc) (void)hipEventDestroy(c->ev_enc);
	for (int i = 0; i < 8; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
	for (int i = 0; i < c->ev_seq_cap; i++) (void)hipEventDestroy(c->ev_seq[i]);
	free(c->ev_seq);
	for (int k = 0; k < AREA_KINDS; k++) if (c->ws[k]) c->ws_free[k](c->ws[k]);
	free(c);
}

void* agmv_hip_area(agmv_hip_ctx* c, agmv_hip_area_kind kind, size_t bytes, void (*destroy)(void*))
{
	if (!c->ws[kind]) {
		if (!(c->ws[kind] = calloc(1, bytes))) { agmv_hip_err("agmv_hip: out of host memory"); return nullptr; }
		c->ws_free[kind] = destroy;
	}
	return c->ws[kind];
}

void agmv_hip_ev_mark(agmv_hip_ctx* c, int which, hipStream_t s)
{
	if (!c->timing) return;
	if (which >= 2 && !(which & 1)) c->ev_seq_n[which / 2 - 1] = 0;   // a start mark: this interval is ev[which], ev[which + 1] again
	(void)hipEventRecord(c->ev[which], s);
}

int agmv_hip_ev_mark_seq(agmv_hip_ctx* c, int i, hipStream_t s)
{
	if (!c->timing) return 0;
	if (i >= c->ev_seq_cap) {
		const int cap = i + 1 > 2 * c->ev_seq_cap ? i + 1 : 2 * c->ev_seq_cap;
		hipEvent_t* p = (hipEvent_t*)realloc(c->ev_seq, (size_t)cap * sizeof(hipEvent_t));
		if (!p) return agmv_hip_err("agmv_hip: out of host memory");
		c->ev_seq = p;
		for (; c->ev_seq_cap < cap; c->ev_seq_cap++) CK(hipEventCreate(&p[c->ev_seq_cap]));
	}
	CK(hipEventRecord(c->ev_seq[i], s));
	if (i > 0 && !(i & 1)) c->ev_seq_n[0] = c->ev_seq_n[1] = c->ev_seq_n[2] = i / 2;   // behind a range's k_fixup: i / 2 whole ranges
	return 0;
}

extern "C" int agmv_hip_enable_timing(agmv_hip_ctx* c, int on)
{
	if (!c) return -1;
	CK(hipSetDevice(c->device));
	if (on && !c->ev[0]) for (int i = 0; i < 8; i++) CK(hipEventCreate(&c->ev[i]));
	c->timing = on ? 1 : 0;
	return 0;
}

/* duration in ms of the last launch of kernel group `which` (0 = k_encode, 1 = the parser kernels,
   2 = k_decode + k_fixup, 3 = the whole of agmv_hip_parse_decode_frames_dev / agmv_hip_decode_bitstreams_dev), measured with HIP events on the
   stream it ran on; synchronises on the stop event.  agmv_hip_decode_bitstreams_dev ran groups 1 and 2 once per range, with one mark
   per boundary: 1 and 2 are the sums over the ranges of that call, 3 is the sum of both (no time lies between its intervals) */
extern "C" float agmv_hip_last_kernel_ms(agmv_hip_ctx* c, int which)
{
	float ms = -1.0f;
	if (!c || !c->timing || which < 0 || which > 3) return -1.0f;
	if (const int n = which ? c->ev_seq_n[which - 1] : 0) {    // agmv_hip_decode_bitstreams_dev: n ranges, a mark per boundary
		const hipEvent_t* e = c->ev_seq;
		if (hipEventSynchronize(e[2 * n]) != hipSuccess) return -1.0f;
		double sum[2] = {0.0, 0.0};                             // parser: [2k] -> [2k + 1]; k_decode + k_fixup: [2k + 1] -> [2k + 2]
		for (int i = 0; i < 2 * n; i++) {
			float part = 0.0f;
			if (hipEventElapsedTime(&part, e[i], e[i + 1]) != hipSuccess) return -1.0f;
			sum[i & 1] += part;
		}
		if (which < 3) return (float)sum[which - 1];
		// the intervals share their marks, so the call is exactly their sum: rounded UP, so that groups 1 and 2 as returned
		// never add up to more than group 3
		const double whole = (double)(float)sum[0] + (double)(float)sum[1];
		ms = (float)whole;
		return (double)ms < whole ? nextafterf(ms, INFINITY) : ms;
	}
	if (hipEventSynchronize(c->ev[2 * which + 1]) != hipSuccess) return -1.0f;
	if (hipEventElapsedTime(&ms, c->ev[2 * which], c->ev[2 * which + 1]) != hipSuccess) return -1.0f;
	return ms;
}

int agmv_hip_enter(agmv_hip_ctx* c, bool palette)
{
	if (!c) return agmv_hip_err("agmv_hip: NULL context");
	if (palette && !c->have_palette) return agmv_hip_err("agmv_hip: agmv_hip_set_palette was not called");
	CK(hipSetDevice(c->device));
	return 0;
}

extern "C" int agmv_hip_set_palette(agmv_hip_ctx* c, const uint32_t p0[256], const uint32_t p1[256], int mode512, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	hipStream_t s = (hipStream_t)stream;
	uint32_t pal[512];
	memcpy(pal, p0, 1024);
	if (p1) memcpy(pal + 256, p1, 1024); else memset(pal + 256, 0, 1024);
	mode512 = mode512 ? 1 : 0;
	pthread_mutex_lock(&g_lut_mu);
	lut_share* sh = nullptr;
	for (lut_share* q = g_luts; q; q = q->next)
		if (q->device == c->device && q->mode512 == mode512 && memcmp(q->pal, pal, sizeof(pal)) == 0) { sh = q; break; }
	int rc = 0;
	if (sh) sh->refs++;
	else {
		sh = (lut_share*)calloc(1, sizeof(*sh));
		hipError_t e = sh ? hipSuccess : hipErrorOutOfMemory;
		if (e == hipSuccess) e = hipMalloc(&sh->d_lut, (size_t)LUT_ENTRIES * sizeof(uint16_t));
		if (e == hipSuccess) e = hipMalloc(&sh->d_mtx, 512 * MROW * sizeof(uint32_t));
		if (e == hipSuccess) e = hipMalloc(&sh->d_pal, 512 * sizeof(uint32_t));
		if (e == hipSuccess) e = hipEventCreateWithFlags(&sh->built, hipEventDisableTiming);
		if (e == hipSuccess) e = hipMemcpyAsync(sh->d_pal, pal, sizeof(pal), hipMemcpyHostToDevice, s);
		if (e == hipSuccess) e = hipStreamSynchronize(s);       // pal[] is a stack buffer
		if (e == hipSuccess) {
			hipLaunchKernelGGL(k_lut_build, dim3(LUT_COLOURS / 256), dim3(256), 0, s, sh->d_pal, mode512, sh->d_lut);
			e = hipGetLastError();
		}
		if (e == hipSuccess) {
			hipLaunchKernelGGL(k_mtx_build, dim3((512 * MROW + 255) / 256), dim3(256), 0, s, sh->d_pal, sh->d_mtx);
			e = hipGetLastError();
		}
		if (e == hipSuccess) e = hipEventRecord(sh->built, s);
		if (e != hipSuccess) {
			rc = agmv_hip_hip_failed("agmv_hip_set_palette", e, __FILE_NAME__, __LINE__);
			if (sh) { (void)hipFree(sh->d_lut); (void)hipFree(sh->d_mtx); (void)hipFree(sh->d_pal); if (sh->built) (void)hipEventDestroy(sh->built); free(sh); }
			sh = nullptr;
		} else {
			sh->device = c->device; sh->mode512 = mode512; sh->refs = 1;
			memcpy(sh->pal, pal, sizeof(pal));
			sh->next = g_luts; g_luts = sh;
		}
	}
	pthread_mutex_unlock(&g_lut_mu);
	if (rc) return rc;
	if (hipStreamWaitEvent(s, sh->built, 0) != hipSuccess) { lut_release(sh); return agmv_hip_hip_failed("hipStreamWaitEvent", hipErrorUnknown, __FILE_NAME__, __LINE__); }   // built on another context's stream?
	lut_share* old_sh = c->share;
	c->share = sh; c->d_lut = sh->d_lut; c->d_mtx = sh->d_mtx; c->d_pal = sh->d_pal;
	c->mode512 = mode512;
	c->have_palette = 1;
	if (old_sh) {                                             // work of this context still in flight may read the old tables
		CK(hipDeviceSynchronize());
		lut_release(old_sh);
	}
	return 0;
}

extern "C" int agmv_hip_quantise_dev(agmv_hip_ctx* c, const uint32_t* d_pix, size_t n, uint16_t* d_entries, void* stream)
{
	if (agmv_hip_enter(c, true)) return -1;
	if (n == 0) return 0;
	size_t blocks = (n + 255) / 256;
	if (blocks > 8192) blocks = 8192;
	hipLaunchKernelGGL(k_quantise, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_pix, n, c->d_lut, d_entries);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_dither_frames_async(agmv_hip_ctx* c, uint32_t strength, uint32_t* d_pix, uint32_t w, uint32_t h, uint32_t n_frames,
                                            void* stream)
{
	if (agmv_hip_enter(c, true)) return -1;
	if (!d_pix || ((uintptr_t)d_pix & 3u)) return agmv_hip_err("agmv_hip: dither: d_pix must be a 4-byte aligned device pointer");
	if (strength < 1 || strength > 64) return agmv_hip_err("agmv_hip: dither: strength must be 1 .. 64 (got %u)", strength);
	if (w == 0 || h == 0) return agmv_hip_err("agmv_hip: dither: width/height must be non-zero (got %ux%u)", w, h);
	// the index inside a frame is 32 bits wide and steps past the end once; the frame's base is a 64-bit offset
	if ((uint64_t)w * h >= (1ull << 31)) return agmv_hip_err("agmv_hip: dither: a frame must have fewer than 2^31 pixels (got %ux%u)", w, h);
	if (n_frames == 0) return 0;
	const uint32_t npx = w * h, cap = (uint32_t)(c->n_cu * DITHER_WG_PER_CU);
	uint32_t gx = (npx + DITHER_T - 1) / DITHER_T, gy = 1;
	if (gx > cap) gx = cap;
	else { gy = cap / gx; if (gy > n_frames) gy = n_frames; if (gy > 65535u) gy = 65535u; }
	hipLaunchKernelGGL(k_dither, dim3(gx, gy), dim3(DITHER_T), 0, (hipStream_t)stream, d_pix, w, npx, n_frames, (int)strength, c->d_lut, c->d_pal);
	CK(hipGetLastError());
	return 0;
}

int agmv_hip_check_geometry(uint32_t w, uint32_t h)
{
	if (w == 0 || h == 0 || (w & 3u) || (h & 3u))
		return agmv_hip_err("agmv_hip: width/height must be non-zero multiples of 4 (got %ux%u); "
		                    "the reference's block loops have no edge handling (src/agmv_encode.c:365-366)", w, h);
	if ((uint64_t)w * h >= (1ull << 31)) return agmv_hip_err("agmv_hip: frame too large");
	return 0;
}

static int encode_dev(agmv_hip_ctx* c, const uint32_t* d_pix, uint32_t n_frames, uint32_t w, uint32_t h,
                      uint32_t first_fc, uint8_t* d_out, size_t out_stride, uint32_t* d_sizes,
                      uint16_t* d_ientries, void* stream, bool entries)
{
	if (agmv_hip_enter(c, true)) return -1;
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (n_frames == 0) return 0;
	if (out_stride < agmv_hip_max_usize(w, h, c->mode512))
		return agmv_hip_err("agmv_hip: out_stride %zu < agmv_hip_max_usize %zu", out_stride, agmv_hip_max_usize(w, h, c->mode512));
	if (((uintptr_t)d_pix & 15u) || ((uintptr_t)d_out & 3u)) return agmv_hip_err("agmv_hip: d_pix must be 16-byte and d_out 4-byte aligned");
	hipStream_t s = (hipStream_t)stream;
	EncArgs A;
	memset(&A, 0, sizeof(A));
	A.pix = d_pix; A.out = d_out; A.sizes = d_sizes; A.lut = c->d_lut; A.mtx = c->d_mtx; A.ientries_in = d_ientries; A.ientries_out = d_ientries;
	A.out_stride = out_stride;
	A.n_frames = n_frames; A.w = w; A.h = h; A.bw = w / 4; A.nblk = (w / 4) * (h / 4);
	A.tpf = (A.nblk + ENC_T - 1) / ENC_T;   // tiles of ENC_T blocks per frame
	A.first_fc = first_fc; A.phase = first_fc & 3u;
	A.n_groups = (n_frames + A.phase + 3) / 4;
	A.total_tiles = A.n_groups * A.tpf;
	if (A.phase != 0 && !d_ientries)
		return agmv_hip_err("agmv_hip: batch starts inside a GOP (frame_count %u) but no I-frame entries were supplied", first_fc);
	A.last_iframe = 0xffffffffu;
	for (int64_t f = (int64_t)n_frames - 1; f >= 0; f--)
		if (((first_fc + (uint32_t)f) & 3u) == 0) { A.last_iframe = (uint32_t)f; break; }
	size_t need = (size_t)n_frames * A.tpf;
	CK(agmv_hip_dev_grow(&c->d_status, &c->status_cap, need));
	A.status = c->d_status; A.ctrl = c->d_ctrl;
	// A batch that starts inside a GOP READS the caller's entry plane (its first tiles) and, if it also holds an I-frame,
	// WRITES the plane (other tiles of the same positions, running at the same time): the new entries go to a scratch
	// plane and are copied over the caller's when the kernel is done.
	const bool ient_both = d_ientries && A.phase != 0 && A.last_iframe != 0xffffffffu;
	const size_t npx_e = (size_t)w * h;
	if (ient_both) {
		CK(agmv_hip_dev_grow(&c->d_ient_tmp, &c->ient_cap, npx_e));
		A.ientries_out = c->d_ient_tmp;
	}
	// the look-back status and the control words belong to the context: an encode on another stream waits for the previous one
	if (!c->ev_enc) CK(hipEventCreateWithFlags(&c->ev_enc, hipEventDisableTiming));
	if (c->have_enc && c->enc_stream != s) CK(hipStreamWaitEvent(s, c->ev_enc, 0));
	CK(hipMemsetAsync(c->d_status, 0, need * sizeof(unsigned long long), s));
	CK(hipMemsetAsync(c->d_ctrl, 0, CTRL_BYTES, s));
	uint32_t grid = (uint32_t)c->enc_grid;
	if (grid > A.total_tiles) grid = A.total_tiles;
	if (const char* e = getenv("AGMV_ENC_GRID")) {             // tuning / test aid: at most n workgroups, each running more tiles.  Never more than are resident (the ticket order's forward progress)
		const long n = atol(e);
		if (n > 0 && (unsigned long)n < grid) grid = (uint32_t)n;
	}
	if (getenv("AGMV_HIP_DEBUG")) fprintf(stderr, "agmv_hip: k_encode: grid of %u workgroup(s) for %u tile(s)\n", grid, A.total_tiles);
	const size_t lds = (size_t)(c->mode512 ? 512 : 256) * MROW * 4 + ENC_LDS_EXTRA;
	void (*kern)(EncArgs) = c->mode512 ? (entries ? k_encode<true, true> : k_encode<true, false>)
	                                   : (entries ? k_encode<false, true> : k_encode<false, false>);
	CK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	agmv_hip_ev_mark(c, 0, s);
	hipLaunchKernelGGL(kern, dim3(grid), dim3(ENC_T), lds, s, A);
	agmv_hip_ev_mark(c, 1, s);
	CK(hipGetLastError());
	hipLaunchKernelGGL(k_encode_verdict, dim3(1), dim3(64), 0, s, c->d_ctrl, d_sizes, n_frames);
	CK(hipGetLastError());
	if (ient_both) CK(hipMemcpyAsync(d_ientries, c->d_ient_tmp, npx_e * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
	CK(hipEventRecord(c->ev_enc, s));
	c->enc_stream = s; c->have_enc = 1;
	return 0;
}

extern "C" int agmv_hip_encode_frames_dev(agmv_hip_ctx* c, const uint32_t* d_pix, uint32_t n_frames, uint32_t w, uint32_t h,
                                          uint32_t first_fc, uint8_t* d_out, size_t out_stride, uint32_t* d_sizes,
                                          uint16_t* d_ientries, void* stream)
{
	return encode_dev(c, d_pix, n_frames, w, h, first_fc, d_out, out_stride, d_sizes, d_ientries, stream, false);
}

extern "C" int agmv_hip_encode_entries_dev(agmv_hip_ctx* c, const uint32_t* d_entries, uint32_t n_frames, uint32_t w, uint32_t h,
                                           uint32_t first_fc, uint8_t* d_out, size_t out_stride, uint32_t* d_sizes,
                                           uint16_t* d_ientries, void* stream)
{
	return encode_dev(c, d_entries, n_frames, w, h, first_fc, d_out, out_stride, d_sizes, d_ientries, stream, true);
}

extern "C" int agmv_hip_check(agmv_hip_ctx* c, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	uint32_t ctrl[4] = {0, 0, 0, 0};
	CK(hipStreamSynchronize((hipStream_t)stream));
	CK(hipMemcpy(ctrl, c->d_ctrl, 16, hipMemcpyDeviceToHost));
	if (ctrl[1]) { agmv_hip_err("agmv_hip: look-back timed out inside k_encode (device error word %u)", ctrl[1]); return -2; }
	return 0;
}

static int encode_host(agmv_hip_ctx* c, const uint32_t* h_pix, uint32_t n_frames, uint32_t w, uint32_t h,
                       uint32_t first_fc, uint8_t* h_out, size_t out_stride, uint32_t* h_sizes, uint16_t* h_ient, bool entries)
{
	if (agmv_hip_enter(c, true)) return -1;
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (n_frames == 0) return 0;
	const size_t npx = (size_t)w * h;
	uint32_t *d_pix = nullptr, *d_sizes = nullptr;
	uint8_t* d_out = nullptr;
	uint16_t* d_ient = nullptr;
	int rc = -1;
	do {
		if (hipMalloc(&d_pix, npx * 4 * n_frames) != hipSuccess || hipMalloc(&d_out, out_stride * n_frames) != hipSuccess ||
		    hipMalloc(&d_sizes, 4 * (size_t)n_frames) != hipSuccess || (h_ient && hipMalloc(&d_ient, npx * 2) != hipSuccess)) {
			agmv_hip_err("agmv_hip: device allocation failed"); break;
		}
		if (hipMemcpy(d_pix, h_pix, npx * 4 * n_frames, hipMemcpyHostToDevice) != hipSuccess) { agmv_hip_err("agmv_hip: H2D failed"); break; }
		if (h_ient && hipMemcpy(d_ient, h_ient, npx * 2, hipMemcpyHostToDevice) != hipSuccess) { agmv_hip_err("agmv_hip: H2D failed"); break; }
		if (encode_dev(c, d_pix, n_frames, w, h, first_fc, d_out, out_stride, d_sizes, d_ient, nullptr, entries)) break;
		if (agmv_hip_check(c, nullptr)) break;
		if (hipMemcpy(h_sizes, d_sizes, 4 * (size_t)n_frames, hipMemcpyDeviceToHost) != hipSuccess) { agmv_hip_err("agmv_hip: D2H failed"); break; }
		bool ok = true;
		for (uint32_t f = 0; f < n_frames && ok; f++)
			ok = hipMemcpy(h_out + (size_t)f * out_stride, d_out + (size_t)f * out_stride, h_sizes[f], hipMemcpyDeviceToHost) == hipSuccess;
		if (!ok) { agmv_hip_err("agmv_hip: D2H failed"); break; }
		if (h_ient && hipMemcpy(h_ient, d_ient, npx * 2, hipMemcpyDeviceToHost) != hipSuccess) { agmv_hip_err("agmv_hip: D2H failed"); break; }
		rc = 0;
	} while (0);
	(void)hipFree(d_pix); (void)hipFree(d_out); (void)hipFree(d_sizes); (void)hipFree(d_ient);
	return rc;
}

extern "C" int agmv_hip_encode_frames(agmv_hip_ctx* c, const uint32_t* h_pix, uint32_t n_frames, uint32_t w, uint32_t h,
                                      uint32_t first_fc, uint8_t* h_out, size_t out_stride, uint32_t* h_sizes, uint16_t* h_ient)
{
	return encode_host(c, h_pix, n_frames, w, h, first_fc, h_out, out_stride, h_sizes, h_ient, false);
}

extern "C" int agmv_hip_encode_entries(agmv_hip_ctx* c, const uint32_t* h_entries, uint32_t n_frames, uint32_t w, uint32_t h,
                                       uint32_t first_fc, uint8_t* h_out, size_t out_stride, uint32_t* h_sizes, uint16_t* h_ient)
{
	return encode_host(c, h_entries, n_frames, w, h, first_fc, h_out, out_stride, h_sizes, h_ient, true);
}

extern "C" int agmv_hip_within2_count(agmv_hip_ctx* c, const uint32_t a[16], const uint32_t b[16])
{
	if (agmv_hip_enter(c)) return -1;
	if (!c->d_nn_pal) CK(hipMalloc(&c->d_nn_pal, 512 * sizeof(uint32_t)));
	uint32_t ab[32], n = 0;
	memcpy(ab, a, 64); memcpy(ab + 16, b, 64);
	CK(hipMemcpy(c->d_nn_pal, ab, sizeof(ab), hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_within2_count, dim3(1), dim3(64), 0, nullptr, c->d_nn_pal, c->d_nn_pal + 32);
	CK(hipGetLastError());
	CK(hipMemcpy(&n, c->d_nn_pal + 32, 4, hipMemcpyDeviceToHost));
	return (int)n;
}

extern "C" int agmv_hip_nearest(agmv_hip_ctx* c, const uint32_t p0[256], const uint32_t p1[256], int mode512,
                                const uint32_t* h_pix, size_t n, uint16_t* h_entries)
{
	if (agmv_hip_enter(c)) return -1;
	if (n == 0) return 0;
	if (!c->d_nn_pal) CK(hipMalloc(&c->d_nn_pal, 512 * sizeof(uint32_t)));
	if (n > c->nn_cap) {                                       // pixels and entries share the capacity
		const size_t cap = n < 256 ? 256 : n;
		c->nn_cap = 0;
		CK(agmv_hip_dev_grow(&c->d_nn_pix, nullptr, cap));
		CK(agmv_hip_dev_grow(&c->d_nn_ent, nullptr, cap));
		c->nn_cap = cap;
	}
	uint32_t pal[512];
	memcpy(pal, p0, 1024);
	if (mode512 && p1) memcpy(pal + 256, p1, 1024); else memset(pal + 256, 0, 1024);
	CK(hipMemcpy(c->d_nn_pal, pal, sizeof(pal), hipMemcpyHostToDevice));
	CK(hipMemcpy(c->d_nn_pix, h_pix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_nearest_direct, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, c->d_nn_pal, mode512 ? 1 : 0, c->d_nn_pix, n, c->d_nn_ent);
	CK(hipGetLastError());
	CK(hipMemcpy(h_entries, c->d_nn_ent, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
	return 0;
}

// ----------------------------------------------------------------------------------------------
// The exchange step of the GOP-sharded encoder (usize per frame, then the variable-length bitstreams to the
// root): a rank's frames leave as ONE contiguous message -- the used bytes of every slab row back to back, frame f at
// offsets[f] -- and arrive in a slab again.  k_pack_scan: offsets = exclusive sums of the sizes (one workgroup);
// k_pack_copy: rows <-> message, a few workgroups per frame striding over 16 KB chunks.  The unaligned side (the message)
// is addressed byte-granularly with dword accesses: gfx950 runs global memory in unaligned mode.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_scan(const uint32_t* __restrict__ sizes, uint32_t n, unsigned long long* __restrict__ offsets)
{
	__shared__ unsigned long long s_w[4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned long long run = 0;
	for (uint32_t i0 = 0; i0 < n; i0 += 256) {
		const uint32_t i = i0 + threadIdx.x;
		const uint32_t v = i < n ? sizes[i] : 0u;
		const uint32_t incl = wave_incl_scan(v, lane);
		if (lane == 63) s_w[wave] = incl;
		__syncthreads();
		unsigned long long base = run;
		for (int k = 0; k < wave; k++) base += s_w[k];
		if (i < n) offsets[i] = base + incl - v;
		run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
		__syncthreads();
	}
	if (threadIdx.x == 0) offsets[n] = run;
}

constexpr uint32_t PACK_CHUNK = 16384;
template <bool UNPACK>
__global__ __launch_bounds__(256) void k_pack_copy(uint8_t* __restrict__ slab, unsigned long long stride, const uint32_t* __restrict__ sizes,
                                                   const unsigned long long* __restrict__ offsets, uint8_t* __restrict__ msg, uint32_t n_frames)
{
	for (uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
		const uint32_t size = sizes[f];
		uint8_t* row = slab + (size_t)f * stride;                  // 256-byte aligned (agmv_hip_max_usize)
		uint8_t* m = msg + offsets[f];                             // any alignment
		for (uint32_t c = blockIdx.x * PACK_CHUNK; c < size; c += gridDim.x * PACK_CHUNK) {
			const uint32_t len = min(PACK_CHUNK, size - c), nd = len >> 2;
			for (uint32_t d = threadIdx.x; d < nd; d += 256) {
				if (UNPACK) *(uint32_t*)(row + c + 4u * d) = *(const u32u*)(m + c + 4u * d);
				else *(u32u*)(m + c + 4u * d) = *(const uint32_t*)(row + c + 4u * d);
			}
			const uint32_t t = 4u * nd + threadIdx.x;              // the <= 3 bytes behind the last whole dword
			if (t < len) {
				if (UNPACK) row[c + t] = m[c + t]; else m[c + t] = row[c + t];
			}
		}
	}
}

static int pack_launch(agmv_hip_ctx* c, bool unpack, uint8_t* d_slab, size_t stride, const uint32_t* d_sizes, uint32_t n_frames,
                       uint8_t* d_msg, unsigned long long* d_offsets, hipStream_t s)
{
	if (!d_slab || !d_sizes || !d_msg || !d_offsets) return agmv_hip_err("agmv_hip: pack/unpack: NULL argument");
	if (stride & 3u) return agmv_hip_err("agmv_hip: pack/unpack: the slab stride must be a multiple of 4 (agmv_hip_max_usize is)");
	hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(256), 0, s, d_sizes, n_frames, d_offsets);
	CK(hipGetLastError());
	uint32_t gx = (uint32_t)((stride / 8 + PACK_CHUNK - 1) / PACK_CHUNK);   // chunks of a frame whose stream is an eighth of the worst case
	if (gx < 1) gx = 1;
	uint32_t gy = n_frames;
	if ((size_t)gx * gy > 65536u) { gy = 65536u / gx; if (gy < 1) gy = 1; }
	if (unpack) hipLaunchKernelGGL(k_pack_copy<true>, dim3(gx, gy), dim3(256), 0, s, d_slab, (unsigned long long)stride, d_sizes, d_offsets, d_msg, n_frames);
	else        hipLaunchKernelGGL(k_pack_copy<false>, dim3(gx, gy), dim3(256), 0, s, d_slab, (unsigned long long)stride, d_sizes, d_offsets, d_msg, n_frames);
	CK(hipGetLastError());
	(void)c;
	return 0;
}

extern "C" int agmv_hip_pack_frames_dev(agmv_hip_ctx* c, const uint8_t* d_slab, size_t stride, const uint32_t* d_sizes, uint32_t n_frames,
                                        uint8_t* d_msg, unsigned long long* d_offsets, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0) return 0;
	return pack_launch(c, false, (uint8_t*)d_slab, stride, d_sizes, n_frames, d_msg, d_offsets, (hipStream_t)stream);
}

extern "C" int agmv_hip_unpack_frames_dev(agmv_hip_ctx* c, const uint8_t* d_msg, const uint32_t* d_sizes, uint32_t n_frames,
                                          uint8_t* d_slab, size_t stride, unsigned long long* d_offsets, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0) return 0;
	return pack_launch(c, true, d_slab, stride, d_sizes, n_frames, (uint8_t*)d_msg, d_offsets, (hipStream_t)stream);
}

// ---- streams, pinned staging and asynchronous copies for C hosts (the pipelined drivers of agmv_pipeline.c) ----
extern "C" void* agmv_hip_stream_create(agmv_hip_ctx* c)
{
	if (agmv_hip_enter(c)) return nullptr;
	hipStream_t s = nullptr;
	CKP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
	return (void*)s;
}
extern "C" void agmv_hip_stream_destroy(agmv_hip_ctx* c, void* stream)
{
	if (!c || !stream) return;
	(void)hipSetDevice(c->device);
	(void)hipStreamDestroy((hipStream_t)stream);
}
extern "C" int agmv_hip_stream_sync(agmv_hip_ctx* c, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	CK(hipStreamSynchronize((hipStream_t)stream));
	return 0;
}
extern "C" void* agmv_hip_event_create(agmv_hip_ctx* c)
{
	if (agmv_hip_enter(c)) return nullptr;
	hipEvent_t e = nullptr;
	if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { agmv_hip_err("agmv_hip: hipEventCreate failed"); return nullptr; }
	return (void*)e;
}
extern "C" void agmv_hip_event_destroy(agmv_hip_ctx* c, void* ev)
{
	if (!c || !ev) return;
	(void)hipSetDevice(c->device);
	(void)hipEventDestroy((hipEvent_t)ev);
}
extern "C" int agmv_hip_event_record(agmv_hip_ctx* c, void* ev, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	CK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
	return 0;
}
extern "C" int agmv_hip_stream_wait_event(agmv_hip_ctx* c, void* stream, void* ev)
{
	if (agmv_hip_enter(c)) return -1;
	CK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
	return 0;
}
extern "C" void* agmv_hip_host_alloc(size_t bytes)
{
	void* p = nullptr;
	if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { agmv_hip_err("agmv_hip: hipHostMalloc(%zu) failed", bytes); return nullptr; }
	return p;
}
extern "C" void agmv_hip_host_free(void* h) { if (h) (void)hipHostFree(h); }
extern "C" void* agmv_hip_malloc_on(agmv_hip_ctx* c, size_t bytes)
{
	if (agmv_hip_enter(c)) return nullptr;
	void* p = nullptr;
	if (hipMalloc(&p, bytes) != hipSuccess) { agmv_hip_err("agmv_hip: hipMalloc(%zu) failed on device %d", bytes, c->device); return nullptr; }
	return p;
}
extern "C" void agmv_hip_free_on(agmv_hip_ctx* c, void* d) { if (c && d) { (void)hipSetDevice(c->device); (void)hipFree(d); } }
extern "C" int agmv_hip_memcpy_async(agmv_hip_ctx* c, void* dst, const void* src, size_t n, int kind, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
	CK(hipMemcpyAsync(dst, src, n, k, (hipStream_t)stream));
	return 0;
}
extern "C" int agmv_hip_memset_async(agmv_hip_ctx* c, void* d, int v, size_t n, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	CK(hipMemsetAsync(d, v, n, (hipStream_t)stream));
	return 0;
}
extern "C" int agmv_hip_ctx_device(agmv_hip_ctx* c) { return c ? c->device : -1; }

extern "C" void* agmv_hip_malloc(size_t bytes)
{
	void* p = nullptr;
	if (hipMalloc(&p, bytes) != hipSuccess) { agmv_hip_err("agmv_hip: hipMalloc(%zu) failed", bytes); return nullptr; }
	return p;
}
extern "C" void agmv_hip_free(void* d) { if (d) (void)hipFree(d); }
extern "C" int agmv_hip_memcpy_h2d(void* d, const void* h, size_t n) { CK(hipMemcpy(d, h, n, hipMemcpyHostToDevice)); return 0; }
extern "C" int agmv_hip_memcpy_d2h(void* h, const void* d, size_t n) { CK(hipMemcpy(h, d, n, hipMemcpyDeviceToHost)); return 0; }
extern "C" int agmv_hip_memset(void* d, int v, size_t n) { CK(hipMemset(d, v, n)); return 0; }
extern "C" int agmv_hip_sync(void) { CK(hipDeviceSynchronize()); return 0; }
