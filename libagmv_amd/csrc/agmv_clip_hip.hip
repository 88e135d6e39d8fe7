// libagmv_amd/csrc/agmv_clip_hip.hip -- the clip front end: what a caller does to a clip in GPU memory before it reaches
// the codec of agmv_hip.hip (include/agmv_hip.h from "helpers on the caller side of the path" to agmv_hip_scale_area_dev), and
// what it asks of one that came back from it (agmv_hip_scale_frames_async, agmv_hip_measure_frames_async).
//
//   k_synth / k_interp        the synthetic test clip, the PDIFS midpoint frame
//   k_histogram*              palette histogram; hist_add_runs is the one statement of the run-length atomics
//   k_similarity*             grey-equality counts of consecutive frames
//   k_gather*                 the nearest scale as a table look-up; gather_frames is the body of the XRGB32 and byte-layout forms
//   k_view                    every step-th frame of an XRGB32 clip and a window of each, copied into a packed clip
//   k_view_src                the same of a clip in any other layout, converted on the way: the encoder's view of its source
//   k_time                    such a view at another frame rate: the exact box filter in time, or the frame under the centre
//   k_stabilise               opt-in: still blocks of the P-frames of a batch replaced by their GOP's I-frame's, in place
//   k_deblock                 opt-in: the block edges of a decoded clip smoothed, one lane per 4x4 cell around a block corner
//   k_pix_* / k_yuv_*         the byte layouts and NV12 / I420 to and from XRGB32
//   k_scale_area              the exact box-filter downscale of a clip in any of the seven layouts
//   k_scale_up*               a decoded XRGB32 clip written at a target size, nearest or bilinear, in any of the seven layouts
//   k_measure                 a decoded XRGB32 clip against its reference in any of the seven layouts: SSE, block-mean SSE, SSIM
//   k_scale_up* <PF_T32/16>   ... or as a normalised float tensor clip (a table look-up per channel);  k_tensor_to_xrgb  the way back
// Each family has an XRGB32 form, one for the byte layouts (PF_RGB24 .. PF_RGB8P) and one templated on the YUV layout; on the
// host CLIP_LAUNCH is the one place where a format value becomes a kernel's template argument.
// Integer/byte work only (k_tensor_to_xrgb: two float32 operations per element); every kernel is an HBM stream, except k_measure,
// which its divisions and moments bind.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "agmv_hip_impl.h"
#include "../../include/agmv_hip_deblock.h"
#include "../../include/agmv_hip_stabilise.h"
#include "../../include/agmv_hip_time.h"
#include "../../include/agmv_hip_view.h"
#include "../../include/agmv_hip_view_source.h"

// ----------------------------------------------------------------------------------------------
// caller-side helpers: synthetic clip, PDIFS midpoint, palette histogram
// ----------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z)
{
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// agmv_synth_v1 (integer-only, also stated in agmv_synth.c and tests/synth.py)
__host__ __device__ __forceinline__ uint32_t synth_pixel(uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t t, uint64_t seed)
{
	const uint64_t te = x < W / 4 ? 0 : t;                     // region A: static
	if (y >= 3 * H / 4) {                                      // region B: flat 32x32 tiles
		uint64_t tileid = ((uint64_t)(y / 32) << 40) | ((uint64_t)(x / 32) << 20) | (te / 8);
		return (uint32_t)(splitmix64(seed ^ tileid) & 0xFFFFFFu);
	}
	const uint64_t h = splitmix64(seed ^ (te * 0x9E3779B97F4A7C15ull) ^ (((uint64_t)y << 32) | x));
	uint32_t r = (uint32_t)(((uint64_t)x * 255 / (W - 1) + 2 * te) & 255);
	uint32_t g = (uint32_t)(((uint64_t)y * 255 / (H - 1) + te) & 255);
	uint32_t b = (uint32_t)((((uint64_t)x + y) / 2 + 3 * te) & 255);
	if ((h & 15) == 0) { r ^= (uint32_t)(h >> 8) & 7; g ^= (uint32_t)(h >> 16) & 7; b ^= (uint32_t)(h >> 24) & 7; }
	return r << 16 | g << 8 | b;
}

__global__ __launch_bounds__(256) void k_synth(uint32_t* __restrict__ pix, uint32_t W, uint32_t H, uint32_t t0,
                                               uint32_t n_frames, uint64_t seed)
{
	const size_t npx = (size_t)W * H, total = npx * n_frames;
	size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	const size_t stride = (size_t)gridDim.x * 256;
	for (; i < total; i += stride) {
		uint32_t f = (uint32_t)(i / npx);
		uint32_t p = (uint32_t)(i - (size_t)f * npx);
		pix[i] = synth_pixel(W, H, p % W, p / W, t0 + f, seed);
	}
}

// AGMV_InterpFrame, src/agmv_utils.c:949-969: c1 + ((c2 - c1) >> 1) per channel, arithmetic shift
__global__ __launch_bounds__(256) void k_interp(uint32_t* __restrict__ out, const uint32_t* __restrict__ f1,
                                                const uint32_t* __restrict__ f2, size_t n)
{
	size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	const size_t stride = (size_t)gridDim.x * 256;
	for (; i < n; i += stride) {
		uint32_t a = f1[i], b = f2[i];
		int r1 = (a >> 16) & 0xff, g1 = (a >> 8) & 0xff, b1 = a & 0xff;
		int r2 = (b >> 16) & 0xff, g2 = (b >> 8) & 0xff, b2 = b & 0xff;
		int r = r1 + ((r2 - r1) >> 1), g = g1 + ((g2 - g1) >> 1), bb = b1 + ((b2 - b1) >> 1);
		out[i] = (uint32_t)(r << 16 | g << 8 | bb);
	}
}

// AGMV_QuantizeColor, src/agmv_utils.c:695-742
__device__ __forceinline__ uint32_t quantize_color(uint32_t c, int quality)
{
	uint32_t r = (c >> 16) & 0xff, g = (c >> 8) & 0xff, b = c & 0xff;
	if (quality == 2) return (r >> 3) << 12 | (g >> 2) << 6 | (b >> 2);     // MID
	if (quality == 3) return (r >> 3) << 11 | (g >> 2) << 5 | (b >> 3);     // LOW
	return (r >> 2) << 13 | (g >> 2) << 7 | (b >> 1);                       // HIGH / default
}

// The run-length atomics of every histogram kernel, for one code per lane.  Lanes hold consecutive pixels; neighbours mostly
// fall into the same bin, so each RUN of equal codes over the wave's live lanes (a prefix of the wave) adds its length with
// one atomic (flat or static areas: one atomic per 64 pixels).  Every lane of the wave calls it.
__device__ __forceinline__ void hist_add_runs(uint32_t* __restrict__ hist, uint32_t c, bool live, int lane)
{
	const uint32_t prev = __shfl_up(c, 1, 64);
	const bool leader = live && (lane == 0 || c != prev);
	const unsigned long long lead = __ballot(leader), alive = __ballot(live);
	if (leader) {
		const unsigned long long rest = lane == 63 ? 0ull : lead >> (lane + 1);
		const uint32_t end = rest ? (uint32_t)lane + 1u + (uint32_t)__builtin_ctzll(rest) : (uint32_t)__popcll(alive);
		atomicAdd(hist + c, end - (uint32_t)lane);
	}
}

__global__ __launch_bounds__(256) void k_histogram(const uint32_t* __restrict__ pix, size_t n, int quality,
                                                   uint32_t* __restrict__ hist)
{
	const int lane = threadIdx.x & 63;
	const size_t stride = (size_t)gridDim.x * 256;
	for (size_t i0 = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63); i0 < n; i0 += stride) {
		const size_t i = i0 + lane;
		const bool live = i < n;
		hist_add_runs(hist, live ? quantize_color(pix[i], quality) : 0xFFFFFFFFu, live, lane);
	}
}

// The grey-equality count behind AGMV_EncodeVideo's frame skipping, AGMV_CompareFrameSimilarity (src/agmv_utils.c:920-947):
// counts[f] = number of positions at which frames f and f + 1 have the same grey, grey = (R + G + B) / 3 in integers (equal to
// the reference's (u8)((r + g + b) / 3.0f) for all 766 sums).  A streaming reduction: a lane owns 8 pixel positions (two
// 16-byte loads per frame, each coalesced over the wave) and walks them through ALL frames, keeping the greys of the frame
// before in two registers, so every frame is read once per launch, not once per pair.  The loads of frame f + 1 are issued
// before frame f is compared.  Per pair the lane's count goes through the wave (__shfl_xor), then one LDS atomic per wave into
// the block's slot of the pair, and the block flushes its slots with one global atomic per pair every SIM_SEG pairs.
#define SIM_SEG 1024

__device__ __forceinline__ uint32_t sim_greys(uint4 v)        // the greys of 4 pixels, one per byte; bits >= 24 are ignored
{
	const uint32_t a = (((v.x >> 16) & 0xff) + ((v.x >> 8) & 0xff) + (v.x & 0xff)) / 3u;
	const uint32_t b = (((v.y >> 16) & 0xff) + ((v.y >> 8) & 0xff) + (v.y & 0xff)) / 3u;
	const uint32_t c = (((v.z >> 16) & 0xff) + ((v.z >> 8) & 0xff) + (v.z & 0xff)) / 3u;
	const uint32_t d = (((v.w >> 16) & 0xff) + ((v.w >> 8) & 0xff) + (v.w & 0xff)) / 3u;
	return a | b << 8 | c << 16 | d << 24;
}

__device__ __forceinline__ uint32_t sim_equal_bytes(uint32_t a, uint32_t b)
{
	const uint32_t x = a ^ b;
	return ((x & 0xffu) == 0) + ((x & 0xff00u) == 0) + ((x & 0xff0000u) == 0) + ((x & 0xff000000u) == 0);
}

// pixels p .. p + 3 of a frame of npx pixels, 0 where there is none.  vec: npx % 4 == 0 and the clip is 16-byte aligned, so
// every frame is, and p < npx implies p + 3 < npx
__device__ __forceinline__ uint4 sim_load(const uint32_t* __restrict__ fr, size_t p, size_t npx, bool vec)
{
	if (vec) return p < npx ? *reinterpret_cast<const uint4*>(fr + p) : make_uint4(0, 0, 0, 0);
	uint4 v;
	v.x = p < npx ? fr[p] : 0; v.y = p + 1 < npx ? fr[p + 1] : 0; v.z = p + 2 < npx ? fr[p + 2] : 0; v.w = p + 3 < npx ? fr[p + 3] : 0;
	return v;
}

__global__ __launch_bounds__(256) void k_similarity(const uint32_t* __restrict__ pix, uint32_t n_frames, size_t npx, int vec,
                                                    uint32_t* __restrict__ counts)
{
	__shared__ uint32_t s_cnt[SIM_SEG];
	const size_t pa = ((size_t)blockIdx.x * 512 + threadIdx.x) * 4, pb = pa + 1024;
	// positions of this lane behind the frame's end read as 0 in every frame: they always compare equal and are taken off again
	const uint32_t dead = (uint32_t)(pa >= npx ? 4 : (pa + 4 > npx ? pa + 4 - npx : 0)) + (uint32_t)(pb >= npx ? 4 : (pb + 4 > npx ? pb + 4 - npx : 0));
	const uint32_t n_pairs = n_frames - 1;
	uint32_t ga = sim_greys(sim_load(pix, pa, npx, vec)), gb = sim_greys(sim_load(pix, pb, npx, vec));
	uint4 na = sim_load(pix + npx, pa, npx, vec), nb = sim_load(pix + npx, pb, npx, vec);
	for (uint32_t seg = 0; seg < n_pairs; seg += SIM_SEG) {
		const uint32_t n_seg = n_pairs - seg < SIM_SEG ? n_pairs - seg : SIM_SEG;
		for (uint32_t k = threadIdx.x; k < n_seg; k += 256) s_cnt[k] = 0;
		__syncthreads();
		for (uint32_t k = 0; k < n_seg; k++) {
			const uint32_t f = seg + k + 1;                    // the later frame of pair seg + k: its pixels are in na, nb
			const uint4 ca = na, cb = nb;
			if (f + 1 < n_frames) {
				const uint32_t* nx = pix + (size_t)(f + 1) * npx;
				na = sim_load(nx, pa, npx, vec); nb = sim_load(nx, pb, npx, vec);
			}
			const uint32_t ha = sim_greys(ca), hb = sim_greys(cb);
			uint32_t c = sim_equal_bytes(ga, ha) + sim_equal_bytes(gb, hb) - dead;
			ga = ha; gb = hb;
			for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
			if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[k], c);
		}
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < n_seg; k += 256) if (s_cnt[k]) atomicAdd(counts + seg + k, s_cnt[k]);
		__syncthreads();
	}
}

// the GBA / NDS nearest scale as a gather: dst[f][k] = src[f][index[k]], 0 where the table says "no source pixel" (0xFFFFFFFF;
// an index outside the source frame reads as that too).  The table holds every quirk of the host scaler (agmv_pipeline.c).
// The body of the three gather kernels: read(f, i) is pixel i < src_px of frame f as 0x00RRGGBB.
template <class Read> __device__ __forceinline__ void gather_frames(const uint32_t* __restrict__ index, size_t n_out, uint32_t n_frames, size_t src_px,
                                                                    uint32_t* __restrict__ dst, Read read)
{
	const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= n_out) return;
	const uint32_t i = index[k];
	const bool live = i != 0xFFFFFFFFu && (size_t)i < src_px;
	for (uint32_t f = 0; f < n_frames; f++) dst[(size_t)f * n_out + k] = live ? read(f, i) : 0u;
}

__global__ __launch_bounds__(256) void k_gather(const uint32_t* __restrict__ src, size_t src_px, uint32_t n_frames,
                                                const uint32_t* __restrict__ index, size_t n_out, uint32_t* __restrict__ dst)
{
	gather_frames(index, n_out, n_frames, src_px, dst, [&](uint32_t f, uint32_t i) { return src[(size_t)f * src_px + i]; });
}

// A view of an XRGB32 clip (agmv_hip_view_frames_async): dst[j][r][c] = src[first + j * step][y + r][x + c], whole words.  A
// streaming copy: a lane owns the 4 consecutive pixels c0 .. c0 + 3 of one output row, blockIdx.x runs over the gpr groups of the h
// rows of a frame, blockIdx.y strides over the frames.  LD4: x, src_w and the source's address are multiples of 4 pixels, so the
// group is one 16-byte load that stays inside its source row (x + c0 + 4 <= src_w); ST4: w and the destination's address are, so
// every group is whole and one 16-byte store.  Every other group goes word by word over its `live` pixels.
template <bool LD4, bool ST4>
__global__ __launch_bounds__(256) void k_view(const uint32_t* __restrict__ src, uint32_t src_w, size_t src_px, uint32_t first, uint32_t step, uint32_t count,
                                              uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t gpr, uint32_t* __restrict__ dst)
{
	const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (item >= (size_t)h * gpr) return;
	const uint32_t r = (uint32_t)(item / gpr), c0 = (uint32_t)(item - (size_t)r * gpr) * 4u;
	const uint32_t live = w - c0 < 4u ? w - c0 : 4u;
	const size_t in_frame = (size_t)(y + r) * src_w + x + c0, out_frame = (size_t)r * w + c0, dst_px = (size_t)w * h;
	for (uint32_t j = blockIdx.y; j < count; j += gridDim.y) {
		const uint32_t* s = src + ((size_t)first + (size_t)j * step) * src_px + in_frame;
		uint32_t* d = dst + (size_t)j * dst_px + out_frame;
		uint4 v = make_uint4(0, 0, 0, 0);
		if (LD4) v = *(const uint4*)s;
		else {
			v.x = s[0];
			if (live > 1) v.y = s[1];
			if (live > 2) v.z = s[2];
			if (live > 3) v.w = s[3];
		}
		if (ST4) *(uint4*)d = v;
		else {
			d[0] = v.x;
			if (live > 1) d[1] = v.y;
			if (live > 2) d[2] = v.z;
			if (live > 3) d[3] = v.w;
		}
	}
}

// Temporal stabilisation in place (agmv_hip_stabilise_frames_async; include/agmv.h, "temporal stabilisation", holds the rule).  One
// lane owns one 4x4 block of one GOP: blockIdx.x runs over the frame's blocks in row-major order, so a wave's row load is 64
// consecutive blocks = 1 KiB wherever a block row is that long, and a narrow frame still fills its waves; blockIdx.y strides over the
// GOPs whose I-frame the batch holds.  stab_gop<NP> is the straight-line body for a GOP with NP P-frames in the batch: the four
// 16-byte row loads of the anchor and the 4 * NP of the P-frames are all issued before the first use, then the decisions, then four
// 16-byte stores per still block.  The decision works on two kinds of masked words, R and B of a pixel (p & 0x00FF00FF) and the
// G of two neighbours in the same two byte places: the sum of the 48 differences is 24 byte SADs, and the max test keeps two
// 16-bit fields per word, u = 0x8000 + s + a - p and v = 0x8000 + s - a + p (0 < u, v < 2^16: no borrow crosses a field, and
// u + v is a constant word, so v costs one subtraction), whose bits 15 are all set exactly when every |a - p| <= s.
constexpr int STAB_T = 256;
#define STAB_GRID_GOPS 65535u     // the GOPs a launch spreads over blockIdx.y; a longer batch takes further trips round the GOP loop

typedef uint32_t stab_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t stab_u32x8 __attribute__((ext_vector_type(8)));     // two rows of a block

template <bool VEC> __device__ __forceinline__ stab_u32x4 stab_load(const uint32_t* p)
{
	if (VEC) return *reinterpret_cast<const stab_u32x4*>(p);
	return stab_u32x4{p[0], p[1], p[2], p[3]};
}

template <bool VEC> __device__ __forceinline__ void stab_store(uint32_t* p, stab_u32x4 v)
{
	if (VEC) *reinterpret_cast<stab_u32x4*>(p) = v;
	else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
}

// rows r and r + 1 of a block, two 16-byte loads
template <bool VEC> __device__ __forceinline__ stab_u32x8 stab_load2(const uint32_t* p, uint32_t w)
{
	return __builtin_shufflevector(stab_load<VEC>(p), stab_load<VEC>(p + w), 0, 1, 2, 3, 4, 5, 6, 7);
}

// 4 pixels of a row as their 6 masked words: R.B of each pixel, then G of pixels 0|1 and 2|3
__device__ __forceinline__ void stab_split(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t m[6])
{
	m[0] = x & 0x00FF00FFu; m[1] = y & 0x00FF00FFu; m[2] = z & 0x00FF00FFu; m[3] = w & 0x00FF00FFu;
	m[4] = ((x >> 8) & 0xFFu) | ((y << 8) & 0x00FF0000u);
	m[5] = ((z >> 8) & 0xFFu) | ((w << 8) & 0x00FF0000u);
}

__device__ __forceinline__ void stab_split2(stab_u32x8 v, uint32_t m[2][6])
{
	stab_split(v[0], v[1], v[2], v[3], m[0]);
	stab_split(v[4], v[5], v[6], v[7], m[1]);
}

// frames fa (the anchor) and fa + (j + 1) * npx, j < NP, at this lane's block; returns bit j set where P-frame j was replaced.
// F[f][i] holds rows 2i and 2i + 1 of frame f of the GOP.  The empty asm statement takes every loaded register as an operand:
// whatever reads a pixel comes behind it, and every load in front of it (left alone, hipcc holds the last frame's loads back
// until the first frame is decided).
template <bool VEC, int NP>
__device__ __forceinline__ uint32_t stab_gop(uint32_t* fa, size_t npx, uint32_t w, uint32_t s)
{
	stab_u32x8 F[NP + 1][2];
#pragma unroll
	for (int f = 0; f <= NP; f++) {
		F[f][0] = stab_load2<VEC>(fa + (size_t)f * npx, w);
		F[f][1] = stab_load2<VEC>(fa + (size_t)f * npx + (size_t)2 * w, w);
	}
	if constexpr (NP == 1) asm volatile("" : "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[1][0]), "+v"(F[1][1]));
	if constexpr (NP == 2) asm volatile("" : "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[1][0]), "+v"(F[1][1]), "+v"(F[2][0]), "+v"(F[2][1]));
	if constexpr (NP == 3)
		asm volatile("" : "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[1][0]), "+v"(F[1][1]), "+v"(F[2][0]), "+v"(F[2][1]), "+v"(F[3][0]), "+v"(F[3][1]));
	const uint32_t K = 0x80008000u + s * 0x00010001u, C = 2u * K;     // (C modulo 2^32: u + v of a word, whose top carry v never has)
	uint32_t am[2][2][6], out = 0;
	stab_split2(F[0][0], am[0]);
	stab_split2(F[0][1], am[1]);
#pragma unroll
	for (int j = 0; j < NP; j++) {
		uint32_t sum = 0, ok = 0x80008000u;
#pragma unroll
		for (int i = 0; i < 2; i++) {
			uint32_t pm[2][6];
			stab_split2(F[j + 1][i], pm);
#pragma unroll
			for (int k = 0; k < 12; k++) {
				const uint32_t a = am[i][k / 6][k % 6], p = pm[k / 6][k % 6], u = a + K - p;
				sum = __builtin_amdgcn_sad_u8(a, p, sum);
				ok &= u & (C - u);
			}
		}
		if ((ok & 0x80008000u) == 0x80008000u && sum <= 12u * s) out |= 1u << j;
	}
	F[0][0] &= 0x00FFFFFFu;
	F[0][1] &= 0x00FFFFFFu;
#pragma unroll
	for (int j = 0; j < NP; j++)
		if (out & (1u << j)) {
#pragma unroll
			for (int i = 0; i < 2; i++) {
				uint32_t* d = fa + (size_t)(j + 1) * npx + (size_t)(2 * i) * w;
				stab_store<VEC>(d, __builtin_shufflevector(F[0][i], F[0][i], 0, 1, 2, 3));
				stab_store<VEC>(d + w, __builtin_shufflevector(F[0][i], F[0][i], 4, 5, 6, 7));
			}
		}
	return out;
}

// lead: the frames in front of the batch's first I-frame; n_gops: the GOPs of the batch that have a P-frame in it.  The count
// of replaced blocks: ballot and popcount per wave and P-frame, the waves' sums through LDS, one 64-bit atomic per workgroup.
// Three waves per SIMD: the 16 loaded rows are 64 registers and the anchor's masked words 24 more; a bound of four waves spills.
template <bool VEC>
__global__ __launch_bounds__(STAB_T, 3) void k_stabilise(uint32_t* __restrict__ pix, uint32_t w, uint32_t bw, uint32_t nblk, size_t npx, uint32_t n_frames,
                                                      uint32_t lead, uint32_t n_gops, uint32_t s, unsigned long long* __restrict__ replaced)
{
	__shared__ uint32_t s_cnt[STAB_T / 64];
	const uint32_t b = blockIdx.x * STAB_T + threadIdx.x;
	const bool live = b < nblk;
	const uint32_t by = b / bw, bx = b - by * bw;
	const size_t in_frame = (size_t)by * 4u * w + (size_t)bx * 4u;
	uint32_t count = 0;                                        // of this wave, the same in all its lanes
	for (uint32_t g = blockIdx.y; g < n_gops; g += gridDim.y) {
		const uint32_t a = lead + 4u * g, after = n_frames - 1u - a;      // the anchor; the batch's frames behind it, >= 1
		uint32_t got = 0;
		if (live) {
			uint32_t* fa = pix + (size_t)a * npx + in_frame;
			if (after >= 3u) got = stab_gop<VEC, 3>(fa, npx, w, s);
			else if (after == 2u) got = stab_gop<VEC, 2>(fa, npx, w, s);
			else got = stab_gop<VEC, 1>(fa, npx, w, s);
		}
		count += (uint32_t)__popcll(__ballot(got & 1u)) + (uint32_t)__popcll(__ballot(got & 2u)) + (uint32_t)__popcll(__ballot(got & 4u));
	}
	if (!replaced) return;
	if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = count;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long total = 0;
		for (int i = 0; i < STAB_T / 64; i++) total += s_cnt[i];
		if (total) atomicAdd(replaced, total);
	}
}

// Deblocking a decoded clip (agmv_hip_deblock_frames_async; include/agmv.h, "deblocking", holds the rule).  The 4x4 cell offset by
// (2, 2) around a block corner -- pixels 4i-2 .. 4i+1 x 4j-2 .. 4j+1, clipped at the frame's rim -- holds every pixel of the lines
// that cross it in either stage, so its 16 output pixels are a function of its 16 input pixels, and the (w/4 + 1) x (h/4 + 1) cells
// partition the frame.  One lane owns one cell of one frame: blockIdx.x runs over the frame's cells in row-major order, blockIdx.y
// strides over the frames, so a workgroup adds its counts once for all its frames.  Four unconditional row loads are issued before the
// first use (a rim cell clamps its rows into the frame and loads the frame's first or last four columns, so no load hangs on a
// branch), both stages run in registers, four row stores.  An interior cell's row starts 8 bytes off a 16-byte boundary of the clip: it
// is ONE 16-byte access at 8-byte alignment (half the memory instructions of two 8-byte ones, and a wave's 64 rows are one
// contiguous KiB either way); a rim cell in x stores the 8-byte half that exists.  A clip that is only 4-byte aligned takes word
// accesses to the same words, as written; hipcc is free to merge them, and does.  The pixels see no LDS and no barrier; the counts are summed per wave by shuffles, per workgroup
// through 32 bytes of LDS behind the last frame, and added with one 64-bit atomic per counter and workgroup.
constexpr int DBK_T = 256;
#define DBK_GRID_BLOCKS 16384u    // the workgroups a launch aims at: blockIdx.y spreads the frames over at most this many / gridDim.x rows ...
#define DBK_GRID_FRAMES 65535u    // ... and never more than the axis holds; a longer clip takes further trips round the frame loop

typedef uint32_t dbk_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dbk_u32x4 __attribute__((ext_vector_type(4)));

template <bool VEC> __device__ __forceinline__ void dbk_load4(const uint32_t* p, uint32_t* c)
{
	if (VEC) {
		dbk_u32x4 v;                                           // 16 bytes at 8-byte alignment: one global_load_dwordx4
		__builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 16);
		c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
	} else { c[0] = p[0]; c[1] = p[1]; c[2] = p[2]; c[3] = p[3]; }
}

template <bool VEC> __device__ __forceinline__ void dbk_store2(uint32_t* p, const uint32_t* c)
{
	if (VEC) *reinterpret_cast<dbk_u32x2*>(p) = dbk_u32x2{c[0], c[1]};
	else { p[0] = c[0]; p[1] = c[1]; }
}

template <bool VEC> __device__ __forceinline__ void dbk_store4(uint32_t* p, const uint32_t* c)
{
	if (VEC) {
		const dbk_u32x4 v = {c[0], c[1], c[2], c[3]};
		__builtin_memcpy(__builtin_assume_aligned(p, 8), &v, 16);
	} else { p[0] = c[0]; p[1] = c[1]; p[2] = c[2]; p[3] = c[3]; }
}

// bits 15 and 31 of the result are set where the 16-bit fields of a and b (each 0 .. 255) differ by at most t; K = 0x80008000 + t * 0x00010001.
// u = K + a - b and v = K - a + b stay inside (0, 2^16) per field, so no borrow crosses a field, and v = 2K - u modulo 2^32.
__device__ __forceinline__ uint32_t dbk_near(uint32_t a, uint32_t b, uint32_t K)
{
	const uint32_t u = a + K - b;
	return u & (2u * K - u);
}

// one line p1 p0 | q0 q1 of one stage, in place.  R and B are worked on in the two 16-bit fields of x & 0x00FF00FF, G in the low
// field of a word of its own: the largest intermediate, 7 * 510 + 510 + 8, fits a field.
__device__ __forceinline__ void dbk_line(uint32_t& P1, uint32_t& P0, uint32_t& Q0, uint32_t& Q1, bool on, uint32_t Ks, uint32_t Kq, uint32_t& weak, uint32_t& strong)
{
	const uint32_t M = 0x00FF00FFu, TOP = 0x80008000u;
	const uint32_t p1r = P1 & M, p0r = P0 & M, q0r = Q0 & M, q1r = Q1 & M;
	const uint32_t p1g = (P1 >> 8) & 0xFFu, p0g = (P0 >> 8) & 0xFFu, q0g = (Q0 >> 8) & 0xFFu, q1g = (Q1 >> 8) & 0xFFu;
	const uint32_t step = dbk_near(p0r, q0r, Ks) & dbk_near(p0g, q0g, Ks);
	const uint32_t side = dbk_near(p1r, p0r, Kq) & dbk_near(p1g, p0g, Kq) & dbk_near(q1r, q0r, Kq) & dbk_near(q1g, q0g, Kq);
	const bool filt = on && ((P0 ^ Q0) & 0x00FFFFFFu) != 0 && (step & TOP) == TOP;
	const bool st = filt && (side & TOP) == TOP, wk = filt && !st;
	const uint32_t ar = p1r + p0r, br = q0r + q1r, ag = p1g + p0g, bg = q0g + q1g;
	const uint32_t r8 = 0x00080008u, r2 = 0x00020002u;
	uint32_t n1r = p1r, n0r = p0r, m0r = q0r, m1r = q1r, n1g = p1g, n0g = p0g, m0g = q0g, m1g = q1g;
	if (st) {
		n1r = ((7u * ar + br + r8) >> 4) & M; n1g = (7u * ag + bg + 8u) >> 4;
		n0r = ((5u * ar + 3u * br + r8) >> 4) & M; n0g = (5u * ag + 3u * bg + 8u) >> 4;
		m0r = ((3u * ar + 5u * br + r8) >> 4) & M; m0g = (3u * ag + 5u * bg + 8u) >> 4;
		m1r = ((ar + 7u * br + r8) >> 4) & M; m1g = (ag + 7u * bg + 8u) >> 4;
	} else if (wk) {
		n0r = ((ar + p0r + q0r + r2) >> 2) & M; n0g = (ag + p0g + q0g + 2u) >> 2;
		m0r = ((br + q0r + p0r + r2) >> 2) & M; m0g = (bg + q0g + p0g + 2u) >> 2;
	}
	P1 = (P1 & 0xFF000000u) | n1r | (n1g << 8);
	P0 = (P0 & 0xFF000000u) | n0r | (n0g << 8);
	Q0 = (Q0 & 0xFF000000u) | m0r | (m0g << 8);
	Q1 = (Q1 & 0xFF000000u) | m1r | (m1g << 8);
	weak += wk;
	strong += st;
}

// the cell: stage 1 on its rows, stage 2 on its columns.  top / bottom: rows 0, 1 / 2, 3 lie in the frame; left / right: columns 0, 1 / 2, 3.
// A rim cell has only the edges that exist, and its pixels outside the frame are never looked at.
__device__ __forceinline__ void dbk_cell(uint32_t c[4][4], bool top, bool bottom, bool left, bool right, uint32_t Ks, uint32_t Kq, uint32_t& weak, uint32_t& strong)
{
#pragma unroll
	for (int r = 0; r < 4; r++) dbk_line(c[r][0], c[r][1], c[r][2], c[r][3], left && right && (r < 2 ? top : bottom), Ks, Kq, weak, strong);
#pragma unroll
	for (int k = 0; k < 4; k++) dbk_line(c[0][k], c[1][k], c[2][k], c[3][k], top && bottom && (k < 2 ? left : right), Ks, Kq, weak, strong);
}

// cw = w/4 + 1 cells per cell row, ncell of them in a frame; bw = w/4 and bh = h/4 are the last cell column and row.  src == dst is
// allowed (a lane reads its cell before it writes it, and no other lane touches it), so neither is __restrict__.
template <bool VEC>
__global__ __launch_bounds__(DBK_T) void k_deblock(const uint32_t* src, uint32_t* dst, uint32_t w, uint32_t cw, uint32_t bh, uint32_t ncell, size_t npx,
                                                   uint32_t n_frames, uint32_t s, unsigned long long* counts)
{
	__shared__ uint32_t s_cnt[DBK_T / 64][2];
	const uint32_t b = blockIdx.x * DBK_T + threadIdx.x;
	const bool live = b < ncell;
	const uint32_t cy = b / cw, cx = b - cy * cw;
	const bool top = cy > 0, bottom = cy < bh, left = cx > 0, right = cx < cw - 1u;
	// the cell's first pixel, (4 cx - 2, 4 cy - 2): outside the frame for a rim cell, whose rows and halves there are never touched
	const ptrdiff_t in_frame = ((ptrdiff_t)cy * 4 - 2) * (ptrdiff_t)w + ((ptrdiff_t)cx * 4 - 2);
	// where the loads go: rows 4 cy - 2 + r clamped to 0 .. h - 1, columns from 4 cx - 2, or 0 / w - 4 for the left / right rim
	uint32_t row[4];
#pragma unroll
	for (int r = 0; r < 4; r++) { const int y = (int)cy * 4 - 2 + r; row[r] = y < 0 ? 0u : (uint32_t)y > bh * 4u - 1u ? bh * 4u - 1u : (uint32_t)y; }
	const uint32_t col = !left ? 0u : right ? cx * 4u - 2u : w - 4u;
	const uint32_t Ks = 0x80008000u + s * 0x00010001u, Kq = 0x80008000u + (s >> 2) * 0x00010001u;
	uint32_t weak = 0, strong = 0;
	if (live)
		for (uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
			uint32_t* out = dst + (size_t)f * npx + in_frame;
			// four unconditional row loads, back to back: a row outside the frame is clamped into it (loaded, never looked at), and
			// a rim cell in x loads the frame's first or last four columns, which hold its half
			uint32_t v[4][4], c[4][4];
#pragma unroll
			for (int r = 0; r < 4; r++) dbk_load4<VEC>(src + (size_t)f * npx + (size_t)row[r] * w + col, v[r]);
			// every loaded register is an operand: what reads a pixel comes behind this, every load in front of it
			asm volatile("" : "+v"(v[0][0]), "+v"(v[0][1]), "+v"(v[0][2]), "+v"(v[0][3]), "+v"(v[1][0]), "+v"(v[1][1]), "+v"(v[1][2]), "+v"(v[1][3]),
			             "+v"(v[2][0]), "+v"(v[2][1]), "+v"(v[2][2]), "+v"(v[2][3]), "+v"(v[3][0]), "+v"(v[3][1]), "+v"(v[3][2]), "+v"(v[3][3]));
#pragma unroll
			for (int r = 0; r < 4; r++) {
				c[r][0] = right ? v[r][0] : v[r][2]; c[r][1] = right ? v[r][1] : v[r][3];
				c[r][2] = left ? v[r][2] : v[r][0]; c[r][3] = left ? v[r][3] : v[r][1];
			}
			dbk_cell(c, top, bottom, left, right, Ks, Kq, weak, strong);
#pragma unroll
			for (int r = 0; r < 4; r++)
				if (r < 2 ? top : bottom) {
					uint32_t* p = out + (ptrdiff_t)r * w;
					if (left && right) dbk_store4<VEC>(p, c[r]);
					else if (left) dbk_store2<VEC>(p, c[r]);
					else dbk_store2<VEC>(p + 2, c[r] + 2);
				}
		}
	if (!counts) return;
#pragma unroll
	for (int d = 32; d; d >>= 1) { weak += __shfl_xor(weak, d); strong += __shfl_xor(strong, d); }
	if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6][0] = weak; s_cnt[threadIdx.x >> 6][1] = strong; }
	__syncthreads();
	if (threadIdx.x < 2) {                                     // lane 0: the weak lines, lane 1: the strong ones
		unsigned long long total = 0;
		for (int i = 0; i < DBK_T / 64; i++) total += s_cnt[i][threadIdx.x];
		if (total) atomicAdd(counts + threadIdx.x, total);
	}
}

// ---- clips in the caller's pixel layout (AGMV_PIXFMT of include/agmv.h: the values 2 .. 5; XRGB32 = 1 goes to the kernels above) ----
// A frame of fpx pixels is fr[fpx][3] bytes R,G,B (RGB24) or B,G,R (BGR24), fr[fpx][4] bytes R,G,B,A (RGBA32), or three planes
// of fpx bytes R, G, B (RGB8P).  The kernels below are HBM streams.  Where every frame (and plane) starts on a 16-byte
// boundary a lane owns 16 consecutive pixels: three 16-byte loads (four for RGBA32), which the wave issues over one contiguous
// 3 (4) KiB, and four 16-byte stores.  Otherwise (`wide` / `vec` 0: a clip at an odd byte offset, a frame size that is no multiple
// of 16) and for the last partial group of 16 of a frame the same kernel goes pixel by pixel through byte loads.
#define PF_XRGB32 1
#define PF_RGB24 2
#define PF_BGR24 3
#define PF_RGBA32 4
#define PF_RGB8P 5

typedef uint32_t pf_u32x4 __attribute__((ext_vector_type(4)));
template <int FMT> struct pf_raw { pf_u32x4 v[FMT == PF_RGBA32 ? 4 : 3]; };      // 16 pixels as they lie in memory

// pixel k of a frame as 0x00RRGGBB, byte by byte (fmt is a constant in the templates)
__device__ __forceinline__ uint32_t pf_read(int fmt, const uint8_t* __restrict__ fr, size_t fpx, size_t k)
{
	if (fmt == PF_RGB8P) return (uint32_t)fr[k] << 16 | (uint32_t)fr[fpx + k] << 8 | fr[2 * fpx + k];
	const uint8_t* p = fr + (fmt == PF_RGBA32 ? 4 : 3) * k;
	return fmt == PF_BGR24 ? (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0] : (uint32_t)p[0] << 16 | (uint32_t)p[1] << 8 | p[2];
}

__device__ __forceinline__ void pf_write(int fmt, uint8_t* __restrict__ fr, size_t fpx, size_t k, uint32_t x)
{
	const uint8_t r = (uint8_t)(x >> 16), g = (uint8_t)(x >> 8), b = (uint8_t)x;
	if (fmt == PF_RGB8P) { fr[k] = r; fr[fpx + k] = g; fr[2 * fpx + k] = b; return; }
	uint8_t* p = fr + (fmt == PF_RGBA32 ? 4 : 3) * k;
	p[0] = fmt == PF_BGR24 ? b : r; p[1] = g; p[2] = fmt == PF_BGR24 ? r : b;
	if (fmt == PF_RGBA32) p[3] = 0xFF;
}

// pixels p .. p + 15 of a frame whose rows of 16 pixels are 16-byte aligned; NT: the bytes are used once
template <int FMT, bool NT> __device__ __forceinline__ pf_raw<FMT> pf_load16(const uint8_t* __restrict__ fr, size_t fpx, size_t p)
{
	pf_raw<FMT> r;
#pragma unroll
	for (int j = 0; j < (FMT == PF_RGBA32 ? 4 : 3); j++) {
		const pf_u32x4* a = reinterpret_cast<const pf_u32x4*>(FMT == PF_RGB8P ? fr + (size_t)j * fpx + p : fr + (FMT == PF_RGBA32 ? 4 : 3) * p + 16 * j);
		r.v[j] = NT ? __builtin_nontemporal_load(a) : *a;
	}
	return r;
}

// pixel i (a constant once the caller's loop is unrolled) of such a group as 0x00RRGGBB
template <int FMT> __device__ __forceinline__ uint32_t pf_pixel(const pf_raw<FMT>& r, int i)
{
	if (FMT == PF_RGB8P) {
		const int s = (i & 3) * 8;
		return ((r.v[0][i >> 2] >> s) & 0xffu) << 16 | ((r.v[1][i >> 2] >> s) & 0xffu) << 8 | ((r.v[2][i >> 2] >> s) & 0xffu);
	}
	if (FMT == PF_RGBA32) {
		const uint32_t w = r.v[i >> 2][i & 3];
		return (w & 0xffu) << 16 | (w & 0xff00u) | ((w >> 16) & 0xffu);
	}
	const int o = 3 * i, w = o >> 2, s = (o & 3) * 8;                  // the pixel's three bytes start at byte o of the 48
	uint32_t v = r.v[w >> 2][w & 3] >> s;
	if (s > 8) v |= r.v[(w + 1) >> 2][(w + 1) & 3] << (32 - s);
	v &= 0xffffffu;                                                  // first byte in bits 0..7: BGR24 is 0x00RRGGBB as it lies
	return FMT == PF_BGR24 ? v : (v & 0xffu) << 16 | (v & 0xff00u) | v >> 16;
}

// the inverse: 16 pixels 0x..RRGGBB (x[j] = pixels 4j .. 4j + 3) as they lie in a frame of FMT
template <int FMT> __device__ __forceinline__ pf_raw<FMT> pf_pack16(const pf_u32x4 x[4])
{
	pf_raw<FMT> r;
#pragma unroll
	for (int w = 0; w < (FMT == PF_RGBA32 ? 16 : 12); w++) {
		uint32_t word = 0;
		if (FMT == PF_RGBA32) {
			const uint32_t c = x[w >> 2][w & 3];
			word = ((c >> 16) & 0xffu) | (c & 0xff00u) | (c & 0xffu) << 16 | 0xff000000u;
		} else {
#pragma unroll
			for (int b = 0; b < 4; b++) {
				const int o = 4 * w + b;                                 // byte o of the 48
				const int i = FMT == PF_RGB8P ? o & 15 : o / 3, ch = FMT == PF_RGB8P ? o >> 4 : o % 3;    // its pixel and channel (0 = first in memory)
				const int sh = FMT == PF_BGR24 ? 8 * ch : 16 - 8 * ch;
				word |= ((x[i >> 2][i & 3] >> sh) & 0xffu) << (8 * b);
			}
		}
		r.v[w >> 2][w & 3] = word;
	}
	return r;
}

// d_dst[f][k] = pixel k of frame f, k < npx <= fpx.  A thread's group of 16 pixels is g; one frame takes bpf blocks.
template <int FMT> __global__ __launch_bounds__(256) void k_pix_to_xrgb(const uint8_t* __restrict__ src, size_t fpx, size_t frame_bytes, size_t npx,
                                                                        uint32_t bpf, int wide, uint32_t* __restrict__ dst)
{
	const uint32_t f = blockIdx.x / bpf;
	const size_t g = (size_t)(blockIdx.x - f * bpf) * 256 + threadIdx.x, p = g * 16;
	const uint8_t* fr = src + (size_t)f * frame_bytes;
	uint32_t* out = dst + (size_t)f * npx;
	if (wide && p + 16 <= npx) {
		const pf_raw<FMT> r = pf_load16<FMT, true>(fr, fpx, p);
#pragma unroll
		for (int j = 0; j < 4; j++) {
			pf_u32x4 o;
#pragma unroll
			for (int i = 0; i < 4; i++) o[i] = pf_pixel<FMT>(r, 4 * j + i);
			*reinterpret_cast<pf_u32x4*>(out + p + 4 * j) = o;
		}
	} else if (wide) {                                                 // the last, partial group of the frame
		for (int i = 0; i < 16; i++) if (p + i < npx) out[p + i] = pf_read(FMT, fr, fpx, p + i);
	} else {                                                           // lanes on consecutive pixels: the wave's 1024, 64 at a time
		const size_t w0 = (g & ~(size_t)63) * 16 + (threadIdx.x & 63);
		for (int i = 0; i < 16; i++) if (w0 + 64 * i < npx) out[w0 + 64 * i] = pf_read(FMT, fr, fpx, w0 + 64 * i);
	}
}

// d_dst frame f = src[f][0 .. npx) in FMT (whole frames of npx pixels); nothing outside those frames is written
template <int FMT> __global__ __launch_bounds__(256) void k_pix_from_xrgb(const uint32_t* __restrict__ src, size_t npx, size_t frame_bytes, uint32_t bpf,
                                                                          int wide, uint8_t* __restrict__ dst)
{
	const uint32_t f = blockIdx.x / bpf;
	const size_t g = (size_t)(blockIdx.x - f * bpf) * 256 + threadIdx.x, p = g * 16;
	const uint32_t* in = src + (size_t)f * npx;
	uint8_t* fr = dst + (size_t)f * frame_bytes;
	if (wide && p + 16 <= npx) {
		pf_u32x4 x[4];
#pragma unroll
		for (int j = 0; j < 4; j++) x[j] = __builtin_nontemporal_load(reinterpret_cast<const pf_u32x4*>(in + p + 4 * j));
		const pf_raw<FMT> r = pf_pack16<FMT>(x);
#pragma unroll
		for (int j = 0; j < (FMT == PF_RGBA32 ? 4 : 3); j++)
			*reinterpret_cast<pf_u32x4*>(FMT == PF_RGB8P ? fr + (size_t)j * npx + p : fr + (FMT == PF_RGBA32 ? 4 : 3) * p + 16 * j) = r.v[j];
	} else if (wide) {
		for (int i = 0; i < 16; i++) if (p + i < npx) pf_write(FMT, fr, npx, p + i, in[p + i]);
	} else {
		const size_t w0 = (g & ~(size_t)63) * 16 + (threadIdx.x & 63);
		for (int i = 0; i < 16; i++) if (w0 + 64 * i < npx) pf_write(FMT, fr, npx, w0 + 64 * i, in[w0 + 64 * i]);
	}
}

// k_gather on a source in fmt: only the pixels the table names are read
__global__ __launch_bounds__(256) void k_gather_fmt(const uint8_t* __restrict__ src, int fmt, size_t src_px, size_t frame_bytes, uint32_t n_frames,
                                                    const uint32_t* __restrict__ index, size_t n_out, uint32_t* __restrict__ dst)
{
	gather_frames(index, n_out, n_frames, src_px, dst, [&](uint32_t f, uint32_t i) { return pf_read(fmt, src + (size_t)f * frame_bytes, src_px, i); });
}

// k_histogram over the first npx pixels of each frame of a clip in FMT.  A wave takes 1024 pixels of one frame in 16 slices of
// 64 consecutive pixels, so that neighbouring lanes hold neighbouring pixels as in k_histogram and runs stay long.  Wide, the
// wave's 3 (4) KiB go through LDS as they lie in memory (each lane's 16-byte loads stored at their place, the pixels of a
// partial last group byte by byte) and a slice reads its pixels from there; byte-wise a slice reads global memory directly.
template <int FMT> __global__ __launch_bounds__(256) void k_histogram_fmt(const uint8_t* __restrict__ src, size_t fpx, size_t frame_bytes, size_t npx,
                                                                          uint32_t bpf, int wide, int quality, uint32_t* __restrict__ hist)
{
	__shared__ pf_u32x4 s_px[4][256];                              // per wave 4 KiB: 1024 pixels (RGB8P: planes 1024 bytes apart)
	const int lane = threadIdx.x & 63;
	const uint32_t f = blockIdx.x / bpf;
	const size_t g = (size_t)(blockIdx.x - f * bpf) * 256 + threadIdx.x, p = g * 16;
	const size_t w0 = (g & ~(size_t)63) * 16;                      // the wave's first pixel
	const uint8_t* fr = src + (size_t)f * frame_bytes;
	if (wide) {
		uint8_t* sw = reinterpret_cast<uint8_t*>(s_px[threadIdx.x >> 6]);
		if (p + 16 <= npx) {
			const pf_raw<FMT> r = pf_load16<FMT, false>(fr, fpx, p);
#pragma unroll
			for (int j = 0; j < (FMT == PF_RGBA32 ? 4 : 3); j++)
				*reinterpret_cast<pf_u32x4*>(FMT == PF_RGB8P ? sw + 1024 * j + 16 * lane : sw + (FMT == PF_RGBA32 ? 64 : 48) * lane + 16 * j) = r.v[j];
		} else {
			for (int i = 0; i < 16; i++) if (p + i < npx) pf_write(FMT, sw, 1024, 16 * lane + i, pf_read(FMT, fr, fpx, p + i));
		}
		__syncthreads();
		for (int i = 0; i < 16; i++) {
			const bool live = w0 + 64 * i + lane < npx;
			hist_add_runs(hist, live ? quantize_color(pf_read(FMT, sw, 1024, 64 * i + lane), quality) : 0xFFFFFFFFu, live, lane);
		}
	} else {
		for (int i = 0; i < 16; i++) {
			const size_t k = w0 + 64 * i + lane;
			const bool live = k < npx;
			hist_add_runs(hist, live ? quantize_color(pf_read(FMT, fr, fpx, k), quality) : 0xFFFFFFFFu, live, lane);
		}
	}
}

// k_similarity on a clip in FMT (frames npx pixels apart): the same walk through all frames and the same slots, with 16 pixel
// positions per lane: three (four) 16-byte loads per frame, the greys of the frame before in four registers.  vec: npx % 16 == 0
// and the clip is 16-byte aligned.  Without it the loads are byte loads and deliver the greys at once (in v[0]).
__device__ __forceinline__ uint32_t sim_grey(uint32_t x) { return (((x >> 16) & 0xff) + ((x >> 8) & 0xff) + (x & 0xff)) / 3u; }

template <int FMT> __device__ __forceinline__ pf_raw<FMT> sim_load16(const uint8_t* __restrict__ fr, size_t p, size_t npx, bool vec)
{
	pf_raw<FMT> r;
	if (vec && p < npx) return pf_load16<FMT, false>(fr, npx, p);
#pragma unroll
	for (int j = 0; j < (FMT == PF_RGBA32 ? 4 : 3); j++) r.v[j] = 0;
	if (!vec) {
#pragma unroll
		for (int i = 0; i < 16; i++) if (p + i < npx) r.v[0][i >> 2] |= sim_grey(pf_read(FMT, fr, npx, p + i)) << (8 * (i & 3));
	}
	return r;
}

template <int FMT> __device__ __forceinline__ pf_u32x4 sim_greys16(const pf_raw<FMT>& r, bool vec)
{
	if (!vec) return r.v[0];
	pf_u32x4 g = 0;
#pragma unroll
	for (int i = 0; i < 16; i++) g[i >> 2] |= sim_grey(pf_pixel<FMT>(r, i)) << (8 * (i & 3));
	return g;
}

template <int FMT> __global__ __launch_bounds__(256) void k_similarity_fmt(const uint8_t* __restrict__ pix, uint32_t n_frames, size_t npx, size_t frame_bytes,
                                                                           int vec, uint32_t* __restrict__ counts)
{
	__shared__ uint32_t s_cnt[SIM_SEG];
	const size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
	// positions of this lane behind the frame's end read as 0 in every frame: they always compare equal and are taken off again
	const uint32_t dead = (uint32_t)(p >= npx ? 16 : (p + 16 > npx ? p + 16 - npx : 0));
	const uint32_t n_pairs = n_frames - 1;
	pf_u32x4 g = sim_greys16<FMT>(sim_load16<FMT>(pix, p, npx, vec), vec);
	pf_raw<FMT> nx = sim_load16<FMT>(pix + frame_bytes, p, npx, vec);
	for (uint32_t seg = 0; seg < n_pairs; seg += SIM_SEG) {
		const uint32_t n_seg = n_pairs - seg < SIM_SEG ? n_pairs - seg : SIM_SEG;
		for (uint32_t k = threadIdx.x; k < n_seg; k += 256) s_cnt[k] = 0;
		__syncthreads();
		for (uint32_t k = 0; k < n_seg; k++) {
			const uint32_t f = seg + k + 1;                    // the later frame of pair seg + k: its pixels are in nx
			const pf_raw<FMT> cur = nx;
			if (f + 1 < n_frames) nx = sim_load16<FMT>(pix + (size_t)(f + 1) * frame_bytes, p, npx, vec);
			const pf_u32x4 h = sim_greys16<FMT>(cur, vec);
			uint32_t c = sim_equal_bytes(g[0], h[0]) + sim_equal_bytes(g[1], h[1]) + sim_equal_bytes(g[2], h[2]) + sim_equal_bytes(g[3], h[3]) - dead;
			g = h;
			for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
			if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[k], c);
		}
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < n_seg; k += 256) if (s_cnt[k]) atomicAdd(counts + seg + k, s_cnt[k]);
		__syncthreads();
	}
}

// ---- clips in 8-bit YUV 4:2:0 (AGMV_PIXFMT_NV12 = 16, AGMV_PIXFMT_I420 = 17 of include/agmv.h, which holds the definition) ----
// A frame of w x h pixels is [h][w] bytes Y, then with cw = (w + 1) / 2, ch = (h + 1) / 2 either [ch][cw][2] bytes U,V (NV12) or
// [ch][cw] bytes U and [ch][cw] bytes V (I420).  Pixel (x, y) takes its chroma from (x >> 1, y >> 1).  The matrix is data: six
// (reading) or ten (writing) integers the host picks from the flags in fmt; the only template axis is the layout.  The kernels are
// HBM streams.  Wide (w a multiple of 16, every frame on a 16-byte boundary) a lane owns a patch of 16 x 2 pixels: two 16-byte
// luma loads and the 16 chroma bytes both rows share (I420: 8 + 8), 32 pixels.  Everything else -- another w, a clip at an odd
// offset, the odd last row, a pixel count that ends inside a patch -- goes pixel by pixel in the same kernel.
#define PF_NV12 16
#define PF_I420 17

typedef uint32_t pf_u32x2 __attribute__((ext_vector_type(2)));
struct yuv_rd { int ky, yo, rv, gu, gv, bu; };
struct yuv_wr { int yr, yg, yb, yo, ur, ug, ub, vr, vg, vb; };
struct yuv_terms { int r, g, b; };                                 // what one chroma sample adds to its (up to) 2 x 2 pixels, rounding included
struct yuv_raw { pf_u32x4 y0, y1, c; };                            // a patch as it lies in memory; c: 8 pairs U,V (NV12), 8 U then 8 V (I420)

__device__ __forceinline__ int yuv_clip8(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ yuv_terms yuv_chroma(const yuv_rd& m, int u, int v)
{
	const int d = u - 128, e = v - 128;
	yuv_terms t;
	t.r = m.rv * e + 128; t.g = 128 - m.gu * d - m.gv * e; t.b = m.bu * d + 128;
	return t;
}

__device__ __forceinline__ uint32_t yuv_pixel(const yuv_rd& m, int y, const yuv_terms& t)
{
	const int c = m.ky * (y - m.yo);
	return (uint32_t)yuv_clip8((c + t.r) >> 8) << 16 | (uint32_t)yuv_clip8((c + t.g) >> 8) << 8 | (uint32_t)yuv_clip8((c + t.b) >> 8);
}

// pixel (x, y) of a frame as 0x00RRGGBB, byte by byte
template <int FMT> __device__ __forceinline__ uint32_t yuv_read(const uint8_t* __restrict__ fr, uint32_t w, uint32_t h, uint32_t x, uint32_t y, const yuv_rd& m)
{
	const size_t cw = (w + 1) >> 1, ch = (h + 1) >> 1, ci = (size_t)(y >> 1) * cw + (x >> 1);
	const uint8_t* c = fr + (size_t)w * h;
	const int u = FMT == PF_NV12 ? c[2 * ci] : c[ci], v = FMT == PF_NV12 ? c[2 * ci + 1] : c[cw * ch + ci];
	return yuv_pixel(m, fr[(size_t)y * w + x], yuv_chroma(m, u, v));
}

// the patch at column x0 (a multiple of 16) of rows 2 * py and (row1) 2 * py + 1, w a multiple of 16 and fr 16-byte aligned
template <int FMT, bool NT> __device__ __forceinline__ yuv_raw yuv_load_patch(const uint8_t* __restrict__ fr, uint32_t w, uint32_t h, uint32_t x0, uint32_t py, bool row1)
{
	yuv_raw r;
	const size_t cw = w >> 1, ch = (h + 1) >> 1;
	const pf_u32x4* a = reinterpret_cast<const pf_u32x4*>(fr + (size_t)2 * py * w + x0);
	const pf_u32x4* b = reinterpret_cast<const pf_u32x4*>(fr + ((size_t)2 * py + 1) * w + x0);
	r.y0 = NT ? __builtin_nontemporal_load(a) : *a;
	r.y1 = 0;
	if (row1) r.y1 = NT ? __builtin_nontemporal_load(b) : *b;
	if (FMT == PF_NV12) {
		const pf_u32x4* c = reinterpret_cast<const pf_u32x4*>(fr + (size_t)w * h + (size_t)py * w + x0);
		r.c = NT ? __builtin_nontemporal_load(c) : *c;
	} else {
		const pf_u32x2* u = reinterpret_cast<const pf_u32x2*>(fr + (size_t)w * h + (size_t)py * cw + (x0 >> 1));
		const pf_u32x2* v = reinterpret_cast<const pf_u32x2*>(fr + (size_t)w * h + cw * ch + (size_t)py * cw + (x0 >> 1));
		const pf_u32x2 uu = NT ? __builtin_nontemporal_load(u) : *u, vv = NT ? __builtin_nontemporal_load(v) : *v;
		r.c[0] = uu[0]; r.c[1] = uu[1]; r.c[2] = vv[0]; r.c[3] = vv[1];
	}
	return r;
}

// chroma sample j (a constant once the caller's loop is unrolled) of a patch
template <int FMT> __device__ __forceinline__ yuv_terms yuv_patch_chroma(const yuv_raw& r, int j, const yuv_rd& m)
{
	if (FMT == PF_NV12) return yuv_chroma(m, (r.c[j >> 1] >> (16 * (j & 1))) & 0xff, (r.c[j >> 1] >> (16 * (j & 1) + 8)) & 0xff);
	return yuv_chroma(m, (r.c[j >> 2] >> (8 * (j & 3))) & 0xff, (r.c[2 + (j >> 2)] >> (8 * (j & 3))) & 0xff);
}

// d_dst[f][k] = pixel k (raster order) of frame f, k < npx <= w * h.  Wide a thread's patch is g; byte-wise the wave takes 2048
// consecutive pixels, 64 at a time.  One frame takes bpf blocks.
template <int FMT> __global__ __launch_bounds__(256) void k_yuv_to_xrgb(const uint8_t* __restrict__ src, uint32_t w, uint32_t h, size_t frame_bytes, uint32_t npx,
                                                                        uint32_t bpf, int wide, yuv_rd m, uint32_t* __restrict__ dst)
{
	const uint32_t f = blockIdx.x / bpf, g = (blockIdx.x - f * bpf) * 256 + threadIdx.x;
	const uint8_t* fr = src + (size_t)f * frame_bytes;
	uint32_t* out = dst + (size_t)f * npx;
	if (wide) {
		const uint32_t ppr = w >> 4, py = g / ppr, x0 = (g - py * ppr) * 16;
		if (2 * py >= h) return;
		const uint32_t k0 = 2 * py * w + x0;
		if (2 * py + 1 < h && k0 + w + 16 <= npx) {
			const yuv_raw r = yuv_load_patch<FMT, true>(fr, w, h, x0, py, true);
#pragma unroll
			for (int q = 0; q < 4; q++) {                          // pixels 4q .. 4q + 3 of both rows: chroma samples 2q, 2q + 1
				const yuv_terms ta = yuv_patch_chroma<FMT>(r, 2 * q, m), tb = yuv_patch_chroma<FMT>(r, 2 * q + 1, m);
				pf_u32x4 o0, o1;
#pragma unroll
				for (int i = 0; i < 4; i++) {
					o0[i] = yuv_pixel(m, (r.y0[q] >> (8 * i)) & 0xff, i < 2 ? ta : tb);
					o1[i] = yuv_pixel(m, (r.y1[q] >> (8 * i)) & 0xff, i < 2 ? ta : tb);
				}
				*reinterpret_cast<pf_u32x4*>(out + k0 + 4 * q) = o0;
				*reinterpret_cast<pf_u32x4*>(out + k0 + w + 4 * q) = o1;
			}
		} else {                                                   // the odd last row, or the count ends in this patch
			for (uint32_t r = 0; r < 2 && 2 * py + r < h; r++)
				for (uint32_t i = 0; i < 16; i++) if (k0 + r * w + i < npx) out[k0 + r * w + i] = yuv_read<FMT>(fr, w, h, x0 + i, 2 * py + r, m);
		}
	} else {
		const uint32_t k0 = (g & ~63u) * 32 + (threadIdx.x & 63);
		for (int i = 0; i < 32; i++) {
			const uint32_t k = k0 + 64 * i;
			if (k < npx) out[k] = yuv_read<FMT>(fr, w, h, k % w, k / w, m);
		}
	}
}

__device__ __forceinline__ uint32_t yuv_luma(const yuv_wr& m, uint32_t x)
{
	const int r = (x >> 16) & 0xff, g = (x >> 8) & 0xff, b = x & 0xff;
	return (uint32_t)yuv_clip8(((m.yr * r + m.yg * g + m.yb * b + 128) >> 8) + m.yo);
}

// U | V << 8 of the mean colour (sums over cnt = 1 << sh pixels)
__device__ __forceinline__ uint32_t yuv_uv(const yuv_wr& m, int sr, int sg, int sb, int sh)
{
	const int half = (1 << sh) >> 1, r = (sr + half) >> sh, g = (sg + half) >> sh, b = (sb + half) >> sh;
	return (uint32_t)yuv_clip8(((m.ur * r + m.ug * g + m.ub * b + 128) >> 8) + 128) |
	       (uint32_t)yuv_clip8(((m.vr * r + m.vg * g + m.vb * b + 128) >> 8) + 128) << 8;
}

// chroma sample (cx, cy) of a frame from the pixels of its 2 x 2 block that exist, byte by byte
template <int FMT> __device__ __forceinline__ void yuv_put_chroma(const uint32_t* __restrict__ in, uint8_t* __restrict__ fr, uint32_t w, uint32_t h, uint32_t cx,
                                                                  uint32_t cy, const yuv_wr& m)
{
	const uint32_t x = 2 * cx, y = 2 * cy, nx = x + 1 < w ? 2 : 1, ny = y + 1 < h ? 2 : 1;
	const size_t cw = (w + 1) >> 1, ch = (h + 1) >> 1, ci = (size_t)cy * cw + cx;
	int sr = 0, sg = 0, sb = 0;
	for (uint32_t j = 0; j < ny; j++)
		for (uint32_t i = 0; i < nx; i++) {
			const uint32_t p = in[(size_t)(y + j) * w + x + i];
			sr += (p >> 16) & 0xff; sg += (p >> 8) & 0xff; sb += p & 0xff;
		}
	const uint32_t uv = yuv_uv(m, sr, sg, sb, (nx == 2) + (ny == 2));
	uint8_t* c = fr + (size_t)w * h;
	if (FMT == PF_NV12) { c[2 * ci] = (uint8_t)uv; c[2 * ci + 1] = (uint8_t)(uv >> 8); }
	else { c[ci] = (uint8_t)uv; c[cw * ch + ci] = (uint8_t)(uv >> 8); }
}

// quarter q (a constant once the caller's loop is unrolled) of a patch of 16 x 2 pixels as it lies in a frame of FMT: a, b = the
// pixels 4q .. 4q + 3 of its two rows as 0x..RRGGBB.  The quarters of a patch are packed in order, 0 first.
template <int FMT> __device__ __forceinline__ void yuv_pack_quarter(yuv_raw& r, int q, const pf_u32x4& a, const pf_u32x4& b, const yuv_wr& m)
{
	uint32_t ya = 0, yb = 0;
#pragma unroll
	for (int i = 0; i < 4; i++) { ya |= yuv_luma(m, a[i]) << (8 * i); yb |= yuv_luma(m, b[i]) << (8 * i); }
	r.y0[q] = ya; r.y1[q] = yb;
	uint32_t uv[2];
#pragma unroll
	for (int j = 0; j < 2; j++) {
		const uint32_t p0 = a[2 * j], p1 = a[2 * j + 1], p2 = b[2 * j], p3 = b[2 * j + 1];
		uv[j] = yuv_uv(m, (int)(((p0 >> 16) & 0xff) + ((p1 >> 16) & 0xff) + ((p2 >> 16) & 0xff) + ((p3 >> 16) & 0xff)),
		               (int)(((p0 >> 8) & 0xff) + ((p1 >> 8) & 0xff) + ((p2 >> 8) & 0xff) + ((p3 >> 8) & 0xff)),
		               (int)((p0 & 0xff) + (p1 & 0xff) + (p2 & 0xff) + (p3 & 0xff)), 2);
	}
	if (FMT == PF_NV12) r.c[q] = uv[0] | uv[1] << 16;              // samples 2q, 2q + 1 as U,V,U,V
	else {                                                     // U of samples 2q, 2q + 1 into byte 2q of the 8 U, V likewise
		const uint32_t u2 = (uv[0] & 0xff) | (uv[1] & 0xff) << 8, v2 = (uv[0] >> 8) | (uv[1] >> 8) << 8;
		if (q & 1) { r.c[q >> 1] |= u2 << 16; r.c[2 + (q >> 1)] |= v2 << 16; } else { r.c[q >> 1] = u2; r.c[2 + (q >> 1)] = v2; }
	}
}

// the whole patch from registers: a[j], b[j] = pixels 4j .. 4j + 3 of its two rows
template <int FMT> __device__ __forceinline__ yuv_raw yuv_pack_patch(const pf_u32x4 a[4], const pf_u32x4 b[4], const yuv_wr& m)
{
	yuv_raw r;
#pragma unroll
	for (int q = 0; q < 4; q++) yuv_pack_quarter<FMT>(r, q, a[q], b[q], m);
	return r;
}

// ... stored at column x0 (a multiple of 16) of rows 2 * py and 2 * py + 1, w a multiple of 16 and fr 16-byte aligned
template <int FMT> __device__ __forceinline__ void yuv_store_patch(uint8_t* __restrict__ fr, uint32_t w, uint32_t h, uint32_t x0, uint32_t py, const yuv_raw& r)
{
	const size_t npx = (size_t)w * h, k0 = (size_t)2 * py * w + x0;
	*reinterpret_cast<pf_u32x4*>(fr + k0) = r.y0;
	*reinterpret_cast<pf_u32x4*>(fr + k0 + w) = r.y1;
	if (FMT == PF_NV12) *reinterpret_cast<pf_u32x4*>(fr + npx + (size_t)py * w + x0) = r.c;
	else {
		const size_t cw = w >> 1, ch = (h + 1) >> 1;
		pf_u32x2 u, v;
		u[0] = r.c[0]; u[1] = r.c[1]; v[0] = r.c[2]; v[1] = r.c[3];
		*reinterpret_cast<pf_u32x2*>(fr + npx + (size_t)py * cw + (x0 >> 1)) = u;
		*reinterpret_cast<pf_u32x2*>(fr + npx + cw * ch + (size_t)py * cw + (x0 >> 1)) = v;
	}
}

// d_dst frame f = src[f][0 .. w * h) written as YUV (whole frames); nothing outside those frames is written
template <int FMT> __global__ __launch_bounds__(256) void k_yuv_from_xrgb(const uint32_t* __restrict__ src, uint32_t w, uint32_t h, size_t frame_bytes, uint32_t bpf,
                                                                          int wide, yuv_wr m, uint8_t* __restrict__ dst)
{
	const uint32_t f = blockIdx.x / bpf, g = (blockIdx.x - f * bpf) * 256 + threadIdx.x, npx = w * h;
	const uint32_t* in = src + (size_t)f * npx;
	uint8_t* fr = dst + (size_t)f * frame_bytes;
	if (wide) {
		const uint32_t ppr = w >> 4, py = g / ppr, x0 = (g - py * ppr) * 16;
		if (2 * py >= h) return;
		const uint32_t k0 = 2 * py * w + x0;
		if (2 * py + 1 < h) {
			yuv_raw r;
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const pf_u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const pf_u32x4*>(in + k0 + 4 * q));
				const pf_u32x4 b = __builtin_nontemporal_load(reinterpret_cast<const pf_u32x4*>(in + k0 + w + 4 * q));
				yuv_pack_quarter<FMT>(r, q, a, b, m);
			}
			yuv_store_patch<FMT>(fr, w, h, x0, py, r);
		} else {                                                   // the odd last row: means over two pixels
			for (uint32_t i = 0; i < 16; i++) fr[k0 + i] = (uint8_t)yuv_luma(m, in[k0 + i]);
			for (uint32_t j = 0; j < 8; j++) yuv_put_chroma<FMT>(in, fr, w, h, (x0 >> 1) + j, py, m);
		}
	} else {                                                       // lanes on consecutive pixels; the pixel at the even corner of a block writes its chroma
		const uint32_t k0 = (g & ~63u) * 32 + (threadIdx.x & 63);
		for (int i = 0; i < 32; i++) {
			const uint32_t k = k0 + 64 * i;
			if (k >= npx) break;
			const uint32_t y = k / w, x = k - y * w;
			fr[k] = (uint8_t)yuv_luma(m, in[k]);
			if (!((x | y) & 1)) yuv_put_chroma<FMT>(in, fr, w, h, x >> 1, y >> 1, m);
		}
	}
}

// k_gather on a YUV source: only the pixels the table names, and their chroma, are read.  (Not through gather_frames: with
// the division by w inside the reader the compiler no longer strength-reduces the loop's addresses.)
template <int FMT> __global__ __launch_bounds__(256) void k_yuv_gather(const uint8_t* __restrict__ src, uint32_t w, uint32_t h, size_t frame_bytes, uint32_t n_frames,
                                                                       const uint32_t* __restrict__ index, size_t n_out, yuv_rd m, uint32_t* __restrict__ dst)
{
	const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= n_out) return;
	const uint32_t i = index[k];
	const bool live = i != 0xFFFFFFFFu && i < w * h;
	const uint32_t y = live ? i / w : 0, x = live ? i - y * w : 0;
	for (uint32_t f = 0; f < n_frames; f++) dst[(size_t)f * n_out + k] = live ? yuv_read<FMT>(src + (size_t)f * frame_bytes, w, h, x, y, m) : 0u;
}

// k_histogram over the first npx pixels (raster order) of each frame of a YUV clip, with the codes and the run-length atomics of
// k_histogram_fmt.  Wide a wave takes 64 patches: each lane's loads go to LDS at their place (1 KiB of row 0, of row 1 and of
// chroma per wave) and the wave then walks the 2048 pixels 64 at a time -- 4 patches of one row, lane l on column l & 15 of patch
// l >> 4 -- so neighbouring lanes hold neighbouring pixels and runs stay long.  Byte-wise a slice of 64 consecutive pixels reads
// global memory directly.
template <int FMT> __global__ __launch_bounds__(256) void k_yuv_histogram(const uint8_t* __restrict__ src, uint32_t w, uint32_t h, size_t frame_bytes, uint32_t npx,
                                                                          uint32_t bpf, int wide, int quality, yuv_rd m, uint32_t* __restrict__ hist)
{
	__shared__ pf_u32x4 s_px[4][3][64];
	const int lane = threadIdx.x & 63;
	const uint32_t f = blockIdx.x / bpf, g = (blockIdx.x - f * bpf) * 256 + threadIdx.x;
	const uint8_t* fr = src + (size_t)f * frame_bytes;
	if (wide) {
		const uint32_t ppr = w >> 4;
		{
			const uint32_t py = g / ppr, x0 = (g - py * ppr) * 16;
			yuv_raw r;
			r.y0 = 0; r.y1 = 0; r.c = 0;
			if (2 * py < h && 2 * py * w + x0 < npx) r = yuv_load_patch<FMT, false>(fr, w, h, x0, py, 2 * py + 1 < h);
			s_px[threadIdx.x >> 6][0][lane] = r.y0; s_px[threadIdx.x >> 6][1][lane] = r.y1; s_px[threadIdx.x >> 6][2][lane] = r.c;
		}
		__syncthreads();
		const uint8_t* sy = reinterpret_cast<const uint8_t*>(s_px[threadIdx.x >> 6][0]);     // rows 1024 bytes apart, chroma behind them
		const uint8_t* sc = sy + 2048;
		uint32_t gp = (g & ~63u) + (lane >> 4), py = gp / ppr, xq = gp - py * ppr;              // this lane's patch of the first four
		for (int q = 0; q < 16; q++) {
			const int at = 64 * q + lane, cs = at >> 1;                                        // byte of the wave's row, chroma sample of the wave's 512
			const int u = FMT == PF_NV12 ? sc[2 * cs] : sc[16 * (cs >> 3) + (cs & 7)], v = FMT == PF_NV12 ? sc[2 * cs + 1] : sc[16 * (cs >> 3) + 8 + (cs & 7)];
			const yuv_terms t = yuv_chroma(m, u, v);
			for (uint32_t r = 0; r < 2; r++) {
				const bool live = 2 * py + r < h && (2 * py + r) * w + xq * 16 + (lane & 15) < npx;
				hist_add_runs(hist, live ? quantize_color(yuv_pixel(m, sy[1024 * r + at], t), quality) : 0xFFFFFFFFu, live, lane);
			}
			xq += 4;
			while (xq >= ppr) { xq -= ppr; py++; }
		}
	} else {
		const uint32_t k0 = (g & ~63u) * 32 + lane;
		for (int i = 0; i < 32; i++) {
			const uint32_t k = k0 + 64 * i;
			const bool live = k < npx;
			hist_add_runs(hist, live ? quantize_color(yuv_read<FMT>(fr, w, h, k % w, k / w, m), quality) : 0xFFFFFFFFu, live, lane);
		}
	}
}

// k_similarity on a YUV clip: the same walk through all frames and the same slots.  A lane owns a patch of up to 16 x 2 pixel
// positions (the grid is ceil(w / 16) x ceil(h / 2) patches): per frame two 16-byte luma loads and the chroma both rows share,
// the greys of the frame before in eight registers.  Without `wide` the patch is read byte by byte into the same registers.
// Positions of the patch behind the frame's edge have grey 0 in every frame: they always compare equal and are taken off again.
template <int FMT> __device__ __forceinline__ yuv_raw sim_yuv_load(const uint8_t* __restrict__ fr, uint32_t w, uint32_t h, uint32_t x0, uint32_t py, uint32_t nx,
                                                                    bool row1, bool wide)
{
	yuv_raw r;
	r.y0 = 0; r.y1 = 0; r.c = 0;
	if (nx == 0) return r;
	if (wide) return yuv_load_patch<FMT, false>(fr, w, h, x0, py, row1);
	const size_t cw = (w + 1) >> 1, ch = (h + 1) >> 1;
	const uint8_t *a = fr + (size_t)2 * py * w + x0, *c = fr + (size_t)w * h + (FMT == PF_NV12 ? 2 : 1) * ((size_t)py * cw + (x0 >> 1));
#pragma unroll
	for (int i = 0; i < 16; i++) if ((uint32_t)i < nx) {
		r.y0[i >> 2] |= (uint32_t)a[i] << (8 * (i & 3));
		if (row1) r.y1[i >> 2] |= (uint32_t)a[w + i] << (8 * (i & 3));
	}
#pragma unroll
	for (int j = 0; j < 8; j++) if ((uint32_t)(2 * j) < nx) {
		if (FMT == PF_NV12) r.c[j >> 1] |= ((uint32_t)c[2 * j] | (uint32_t)c[2 * j + 1] << 8) << (16 * (j & 1));
		else { r.c[j >> 2] |= (uint32_t)c[j] << (8 * (j & 3)); r.c[2 + (j >> 2)] |= (uint32_t)c[cw * ch + j] << (8 * (j & 3)); }
	}
	return r;
}

struct yuv_greys { pf_u32x4 a, b; };                               // one grey per byte: row 0, row 1

template <int FMT> __device__ __forceinline__ yuv_greys sim_yuv_greys(const yuv_raw& r, const yuv_rd& m, const pf_u32x4& live, bool row1)
{
	yuv_greys g;
	g.a = 0; g.b = 0;
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const yuv_terms t = yuv_patch_chroma<FMT>(r, j, m);
#pragma unroll
		for (int i = 2 * j; i < 2 * j + 2; i++) {
			g.a[i >> 2] |= sim_grey(yuv_pixel(m, (r.y0[i >> 2] >> (8 * (i & 3))) & 0xff, t)) << (8 * (i & 3));
			g.b[i >> 2] |= sim_grey(yuv_pixel(m, (r.y1[i >> 2] >> (8 * (i & 3))) & 0xff, t)) << (8 * (i & 3));
		}
	}
	g.a &= live;
	if (row1) g.b &= live; else g.b = 0;
	return g;
}

template <int FMT> __global__ __launch_bounds__(256) void k_yuv_similarity(const uint8_t* __restrict__ pix, uint32_t n_frames, uint32_t w, uint32_t h, size_t frame_bytes,
                                                                           int wide, yuv_rd m, uint32_t* __restrict__ counts)
{
	__shared__ uint32_t s_cnt[SIM_SEG];
	const uint32_t ppr = (w + 15) >> 4, g = blockIdx.x * 256 + threadIdx.x, py = g / ppr, x0 = (g - py * ppr) * 16;
	const uint32_t nx = 2 * py < h ? (w - x0 < 16 ? w - x0 : 16) : 0;     // columns of this lane's patch that exist
	const bool row1 = nx && 2 * py + 1 < h;
	const uint32_t dead = 32 - nx * (row1 ? 2 : 1);
	pf_u32x4 live;
#pragma unroll
	for (int q = 0; q < 4; q++) live[q] = nx >= 4u * q + 4 ? 0xFFFFFFFFu : (nx > 4u * q ? (1u << (8 * (nx - 4 * q))) - 1 : 0u);
	const uint32_t n_pairs = n_frames - 1;
	yuv_greys gp = sim_yuv_greys<FMT>(sim_yuv_load<FMT>(pix, w, h, x0, py, nx, row1, wide), m, live, row1);
	yuv_raw nxt = sim_yuv_load<FMT>(pix + frame_bytes, w, h, x0, py, nx, row1, wide);
	for (uint32_t seg = 0; seg < n_pairs; seg += SIM_SEG) {
		const uint32_t n_seg = n_pairs - seg < SIM_SEG ? n_pairs - seg : SIM_SEG;
		for (uint32_t k = threadIdx.x; k < n_seg; k += 256) s_cnt[k] = 0;
		__syncthreads();
		for (uint32_t k = 0; k < n_seg; k++) {
			const uint32_t f = seg + k + 1;                    // the later frame of pair seg + k: its patch is in nxt
			const yuv_raw cur = nxt;
			if (f + 1 < n_frames) nxt = sim_yuv_load<FMT>(pix + (size_t)(f + 1) * frame_bytes, w, h, x0, py, nx, row1, wide);
			const yuv_greys gh = sim_yuv_greys<FMT>(cur, m, live, row1);
			uint32_t c = sim_equal_bytes(gp.a[0], gh.a[0]) + sim_equal_bytes(gp.a[1], gh.a[1]) + sim_equal_bytes(gp.a[2], gh.a[2]) + sim_equal_bytes(gp.a[3], gh.a[3]) +
			             sim_equal_bytes(gp.b[0], gh.b[0]) + sim_equal_bytes(gp.b[1], gh.b[1]) + sim_equal_bytes(gp.b[2], gh.b[2]) + sim_equal_bytes(gp.b[3], gh.b[3]) - dead;
			gp = gh;
			for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
			if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[k], c);
		}
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < n_seg; k += 256) if (s_cnt[k]) atomicAdd(counts + seg + k, s_cnt[k]);
		__syncthreads();
	}
}

// ---- exact box-filter downscale of a clip in any of the seven layouts (AGMV_SCALE_AREA of include/agmv.h, which defines it) ----
// On an axis source pixel i covers [i * dw, (i + 1) * dw) and target pixel X covers [X * sw, (X + 1) * sw): a source pixel is dw
// units long, lies in at most two target columns, and the weights of a target column sum to sw.  A scatter: a workgroup owns one
// (frame, target row Y, tile of SC_TILE target columns) at a time and walks the source rows that overlap Y.  A lane takes a group
// of 16 consecutive pixels of one source row -- groups are cut at multiples of 16 of the pixel's index in the FRAME, so that on a
// clip whose frames (and planes) start on 16-byte boundaries a group that lies inside the row is read with the 16-byte loads of
// k_pix_to_xrgb / k_yuv_to_xrgb (YUV: 16 luma bytes and the 16 chroma bytes of row j >> 1, which needs sw % 16 == 0); the groups
// at a row's head and tail, and every group of any other clip, go pixel by pixel through the layout's byte reader.  The lane folds
// wx * channel of its pixels per target column in registers and adds wy * that into the tile's accumulators in LDS once per
// column it touches (integer adds: any order gives the same sum).  After the barrier each lane finishes its columns --
// (sum + area / 2) / area, exact in 32 bits because 255 * sw * sh + sw * sh / 2 < 2^32 for sw * sh <= 2^24 -- clears them for the
// next item and stores the row.  No float, no global atomic.  Items are walked with a grid stride: any number of frames.
#define SC_TILE 1024

struct ScaleArgs {
	const uint8_t* src;
	uint32_t* dst;
	size_t frame_bytes;
	unsigned long long items;                                      // n_frames * dh * tiles
	uint32_t sw, sh, dw, dh, tiles;
	int wide, small;                                               // 16-byte loads allowed; sw * dw < 2^32
	yuv_rd m;
};

// 16 pixels of one source row as they lie in memory: p0 is their index in the frame (a multiple of 16), j their row
template <int FMT> struct sc_group {
	static constexpr bool YUV = FMT >= PF_NV12;
	static constexpr int NV = YUV ? 2 : (FMT == PF_XRGB32 || FMT == PF_RGBA32 ? 4 : 3);
	pf_u32x4 v[NV];                                                // YUV: luma, then chroma as yuv_raw::c holds it

	__device__ __forceinline__ void load(const uint8_t* __restrict__ fr, uint32_t w, uint32_t h, uint32_t p0, uint32_t j)
	{
		if constexpr (YUV) {
			const uint32_t x0 = p0 - j * w;
			const uint8_t* c = fr + (size_t)w * h;
			v[0] = *reinterpret_cast<const pf_u32x4*>(fr + p0);
			if constexpr (FMT == PF_NV12) v[1] = *reinterpret_cast<const pf_u32x4*>(c + (size_t)(j >> 1) * w + x0);
			else {
				const size_t cw = w >> 1, ch = (h + 1) >> 1, o = (size_t)(j >> 1) * cw + (x0 >> 1);
				const pf_u32x2 uu = *reinterpret_cast<const pf_u32x2*>(c + o), vv = *reinterpret_cast<const pf_u32x2*>(c + cw * ch + o);
				v[1][0] = uu[0]; v[1][1] = uu[1]; v[1][2] = vv[0]; v[1][3] = vv[1];
			}
		} else if constexpr (NV == 4) {
#pragma unroll
			for (int k = 0; k < 4; k++) v[k] = *reinterpret_cast<const pf_u32x4*>(fr + 4 * (size_t)p0 + 16 * k);
		} else {
			const pf_raw<FMT> r = pf_load16<FMT, false>(fr, (size_t)w * h, p0);
#pragma unroll
			for (int k = 0; k < 3; k++) v[k] = r.v[k];
		}
	}

	// pixel i (a constant once the caller's loop is unrolled) as 0x00RRGGBB
	__device__ __forceinline__ uint32_t pixel(int i, const yuv_rd& m) const
	{
		if constexpr (YUV) {
			yuv_raw r;
			r.y0 = v[0]; r.y1 = v[0]; r.c = v[1];
			return yuv_pixel(m, (v[0][i >> 2] >> (8 * (i & 3))) & 0xff, yuv_patch_chroma<FMT>(r, i >> 1, m));
		} else if constexpr (FMT == PF_XRGB32) {
			return v[i >> 2][i & 3] & 0xffffffu;
		} else {
			pf_raw<FMT> r;
#pragma unroll
			for (int k = 0; k < NV; k++) r.v[k] = v[k];
			return pf_pixel<FMT>(r, i);
		}
	}
};

// pixel (x, j) of a frame as 0x00RRGGBB through the layout's byte reader
template <int FMT> __device__ __forceinline__ uint32_t sc_read(const uint8_t* __restrict__ fr, uint32_t w, uint32_t h, uint32_t x, uint32_t j, const yuv_rd& m)
{
	if constexpr (FMT >= PF_NV12) return yuv_read<FMT>(fr, w, h, x, j, m);
	else if constexpr (FMT == PF_XRGB32) return reinterpret_cast<const uint32_t*>(fr)[(size_t)j * w + x] & 0xffffffu;
	else return pf_read(FMT, fr, (size_t)w * h, (size_t)j * w + x);
}

// a lane's walk along a source row: it stands t units into target column X and holds the sums of wx * channel for that column
struct sc_run { uint32_t X, t, r, g, b; };

__device__ __forceinline__ void sc_flush(uint32_t (*acc)[SC_TILE], const sc_run& s, uint32_t wy, uint32_t X0, uint32_t X1)
{
	if (s.X >= X0 && s.X < X1) {
		atomicAdd(&acc[0][s.X - X0], s.r * wy); atomicAdd(&acc[1][s.X - X0], s.g * wy); atomicAdd(&acc[2][s.X - X0], s.b * wy);
	}
}

// the next source pixel, colour c: min(dw, what is left of column X) units go to X, the rest opens column X + 1
__device__ __forceinline__ void sc_step(uint32_t (*acc)[SC_TILE], sc_run& s, uint32_t c, uint32_t sw, uint32_t dw, uint32_t wy, uint32_t X0, uint32_t X1)
{
	const uint32_t r = (c >> 16) & 0xff, g = (c >> 8) & 0xff, b = c & 0xff, w1 = min(dw, sw - s.t);
	s.r += w1 * r; s.g += w1 * g; s.b += w1 * b; s.t += w1;
	if (s.t == sw) {
		sc_flush(acc, s, wy, X0, X1);
		s.X++; s.t = dw - w1;
		s.r = s.t * r; s.g = s.t * g; s.b = s.t * b;
	}
}

template <int FMT> __global__ __launch_bounds__(256) void k_scale_area(ScaleArgs A)
{
	__shared__ uint32_t s_acc[3][SC_TILE];
	const uint32_t sw = A.sw, sh = A.sh, dw = A.dw, dh = A.dh, area = sw * sh, per = dh * A.tiles;
	for (uint32_t k = threadIdx.x; k < 3 * SC_TILE; k += 256) (&s_acc[0][0])[k] = 0;
	__syncthreads();
	for (unsigned long long item = blockIdx.x; item < A.items; item += gridDim.x) {
		const uint32_t f = (uint32_t)(item / per), rem = (uint32_t)(item - (unsigned long long)f * per), Y = rem / A.tiles, tile = rem - Y * A.tiles;
		const uint32_t X0 = tile * SC_TILE, X1 = min(X0 + SC_TILE, dw);
		// the source columns that touch the tile, the source rows that touch Y
		const uint32_t i_lo = (uint32_t)((unsigned long long)X0 * sw / dw), i_hi = (uint32_t)(((unsigned long long)X1 * sw + dw - 1) / dw);
		const unsigned long long y_lo = (unsigned long long)Y * sh, y_hi = y_lo + sh;
		const uint32_t j0 = (uint32_t)(y_lo / dh), j1 = (uint32_t)((y_hi + dh - 1) / dh);
		const uint32_t ng = ((i_hi - i_lo + 15) >> 4) + 1, n_task = (j1 - j0) * ng;
		const uint8_t* fr = A.src + (size_t)f * A.frame_bytes;
		for (uint32_t task = threadIdx.x; task < n_task; task += 256) {
			const uint32_t jr = task / ng, j = j0 + jr, row0 = j * sw, lo = row0 + i_lo, hi = row0 + i_hi;
			const uint32_t p0 = ((lo >> 4) + (task - jr * ng)) << 4;
			if (p0 >= hi) continue;
			const uint32_t a = max(p0, lo), b = min(p0 + 16, hi);      // the group's pixels of this row and tile
			const unsigned long long r_lo = (unsigned long long)j * dh;
			const uint32_t wy = (uint32_t)(min(r_lo + dh, y_hi) - max(r_lo, y_lo));
			sc_run s;
			if (A.small) { const uint32_t u = (a - row0) * dw; s.X = u / sw; s.t = u - s.X * sw; }
			else { const unsigned long long u = (unsigned long long)(a - row0) * dw; s.X = (uint32_t)(u / sw); s.t = (uint32_t)(u - (unsigned long long)s.X * sw); }
			s.r = s.g = s.b = 0;
			if (A.wide && b - a == 16) {
				sc_group<FMT> grp;
				grp.load(fr, sw, sh, p0, j);
#pragma unroll
				for (int i = 0; i < 16; i++) sc_step(s_acc, s, grp.pixel(i, A.m), sw, dw, wy, X0, X1);
			} else {
				for (uint32_t p = a; p < b; p++) sc_step(s_acc, s, sc_read<FMT>(fr, sw, sh, p - row0, j, A.m), sw, dw, wy, X0, X1);
			}
			if (s.t) sc_flush(s_acc, s, wy, X0, X1);
		}
		__syncthreads();
		uint32_t* out = A.dst + ((size_t)f * dh + Y) * dw + X0;
		for (uint32_t k = threadIdx.x; k < X1 - X0; k += 256) {
			const uint32_t r = (s_acc[0][k] + area / 2) / area, g = (s_acc[1][k] + area / 2) / area, b = (s_acc[2][k] + area / 2) / area;
			s_acc[0][k] = 0; s_acc[1][k] = 0; s_acc[2][k] = 0;
			out[k] = r << 16 | g << 8 | b;
		}
		__syncthreads();
	}
}

// ---- a view of a clip in the caller's layout (agmv_hip_view_source_async of include/agmv_hip_view_source.h) ----
// dst[j][r][c] = P(first + j * step)[y + r][x + c], P(k) being frame k as k_pix_to_xrgb / k_yuv_to_xrgb give it.  A streaming
// convert-copy: a lane owns the 16 consecutive pixels c0 .. c0 + 15 of one output row (YUV: of the rows 2i and 2i + 1 of the window,
// the patch of yuv_load_patch), blockIdx.x runs over the gpr groups of the rows (row pairs) of a window, blockIdx.y strides over
// the frames.  ld: the groups of the window's rows start on 16-byte boundaries of the source (YUV: and y is even, so both rows of
// a patch share a chroma row): a group whose 16 source pixels lie inside its source row is read through pf_load16 /
// yuv_load_patch, non-temporal.  st: w is a multiple of 4 and dst is 16-byte aligned: a group is 1 .. 4 whole 16-byte stores per row.
// A group that was loaded whole is converted whole and then stored; the pixel-by-pixel form makes and stores four pixels at a time.
// Every other group goes pixel by pixel over its `live` pixels through sc_read, to the same words.
struct ViewSrcArgs {
	const uint8_t* src;
	uint32_t* dst;
	size_t frame_bytes;                                            // of a source frame
	uint32_t sw, sh, first, step, count, x, y, w, h, gpr;
	int ld, st;
	yuv_rd m;
};

// pixels 4q .. 4q + 3 of a lane's group, those below `live`, to d: one 16-byte store (st: all four are live), else word by word
__device__ __forceinline__ void view_src_store4(uint32_t* __restrict__ d, int q, const pf_u32x4& o, uint32_t live, int st)
{
	if (st) *reinterpret_cast<pf_u32x4*>(d + 4 * q) = o;
	else {
#pragma unroll
		for (int i = 0; i < 4; i++) if (4u * q + i < live) d[4 * q + i] = o[i];
	}
}

template <int FMT> __global__ __launch_bounds__(256) void k_view_src(ViewSrcArgs A)
{
	constexpr bool YUV = FMT >= PF_NV12;
	const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (item >= (size_t)(YUV ? (A.h + 1) >> 1 : A.h) * A.gpr) return;
	const uint32_t ri = (uint32_t)(item / A.gpr), c0 = (uint32_t)(item - (size_t)ri * A.gpr) * 16u, r = YUV ? 2 * ri : ri;
	const uint32_t live = A.w - c0 < 16u ? A.w - c0 : 16u, sx = A.x + c0, sy = A.y + r;
	const bool row1 = YUV && r + 1 < A.h, ld = A.ld && sx + 16 <= A.sw;
	for (uint32_t j = blockIdx.y; j < A.count; j += gridDim.y) {
		const uint8_t* fr = A.src + ((size_t)A.first + (size_t)j * A.step) * A.frame_bytes;
		uint32_t* d = A.dst + ((size_t)j * A.h + r) * A.w + c0;
		if (ld) {
			if constexpr (YUV) {
				const yuv_raw p = yuv_load_patch<FMT, true>(fr, A.sw, A.sh, sx, sy >> 1, row1);
				pf_u32x4 o0[4], o1[4];
#pragma unroll
				for (int q = 0; q < 4; q++) {                          // pixels 4q .. 4q + 3 of both rows: chroma samples 2q, 2q + 1
					const yuv_terms ta = yuv_patch_chroma<FMT>(p, 2 * q, A.m), tb = yuv_patch_chroma<FMT>(p, 2 * q + 1, A.m);
#pragma unroll
					for (int i = 0; i < 4; i++) {
						o0[q][i] = yuv_pixel(A.m, (p.y0[q] >> (8 * i)) & 0xff, i < 2 ? ta : tb);
						o1[q][i] = yuv_pixel(A.m, (p.y1[q] >> (8 * i)) & 0xff, i < 2 ? ta : tb);
					}
				}
#pragma unroll
				for (int q = 0; q < 4; q++) if (4u * q < live) view_src_store4(d, q, o0[q], live, A.st);
				if (row1) {
#pragma unroll
					for (int q = 0; q < 4; q++) if (4u * q < live) view_src_store4(d + A.w, q, o1[q], live, A.st);
				}
			} else {
				const pf_raw<FMT> p = pf_load16<FMT, true>(fr, (size_t)A.sw * A.sh, (size_t)sy * A.sw + sx);
				pf_u32x4 o[4];
#pragma unroll
				for (int i = 0; i < 16; i++) o[i >> 2][i & 3] = pf_pixel<FMT>(p, i);
#pragma unroll
				for (int q = 0; q < 4; q++) if (4u * q < live) view_src_store4(d, q, o[q], live, A.st);
			}
		} else {
			for (uint32_t rr = 0; rr < (row1 ? 2u : 1u); rr++) {
#pragma unroll
				for (int q = 0; q < 4; q++) {
					if (4u * q >= live) break;
					pf_u32x4 o;
#pragma unroll
					for (int i = 0; i < 4; i++) o[i] = 4u * q + i < live ? sc_read<FMT>(fr, A.sw, A.sh, sx + 4 * q + i, sy + rr, A.m) : 0u;
					view_src_store4(d + (size_t)rr * A.w, q, o, live, A.st);
				}
			}
		}
	}
}

// ---- a view of a clip at another frame rate (agmv_hip_time_frames_async of include/agmv_hip_time.h; AGMV_RATE of include/agmv.h has the rule) ----
// dst[jj] = frame j = j0 + jj of R, the view V (k_view_src's dst) resampled in time sn : dn.  k_view_src's ownership: a lane owns 16
// consecutive pixels of one output row, blockIdx.x runs over the groups of a window's rows, blockIdx.y strides over the output
// frames.  For YUV a lane owns a patch of 8 x 2: the 96 sums of 16 x 2 pixels beside two taps' bytes and the conversion's
// temporaries took every register a lane can have (256 VGPRs and 86 AGPRs, one wave per SIMD), the 48 of 8 x 2 leave room for three.
// Per output frame the taps k0 .. k1 of V and their weights are uniform over the workgroup: AREA
// k0 = (j sn) div dn .. k1 = ((j + 1) sn - 1) div dn with the overlap of [k dn, (k + 1) dn) and [j sn, (j + 1) sn) as weight, NEAREST
// the one tap ((2j + 1) sn) div (2 dn) at weight sn -- the same loop.  Per tap a lane whose source pixels lie inside their row on
// a 16-byte boundary (YUV: 8-byte; ld says the frames allow it; the lane checks its own offset, which is the same in every frame)
// reads them through pf_load16, or as the halves of yuv_load_patch's vectors, non-temporal: a frame has weight in at most two
// outputs.  The next tap's loads are issued before the current tap is accumulated.  Every other lane goes pixel by pixel through
// sc_read.  Three 32-bit sums per pixel take weight * channel in RGB, after the layout's reading rule: 255 * sn + sn / 2 < 2^32 for
// sn <= 65535.  Then (sum + sn / 2) / sn by the uniform divisor, packed, bits 24 .. 31 zero, stored as k_view_src stores.
struct TimeArgs {
	const uint8_t* src;
	uint32_t* dst;
	size_t frame_bytes;                                            // of a source frame
	uint32_t sw, sh, first, step, x, y, w, h, gpr, sn, dn, j0, count;
	int nearest, ld, st;
	yuv_rd m;
};

struct yuv_half { pf_u32x2 y0, y1, c; };                           // a patch of 8 x 2 as it lies in memory; c: 4 pairs U,V (NV12), 4 U then 4 V (I420)

// a lane's pixels of one tap as they lie in memory: 16 of a row (XRGB32 lies as RGBA32 does, four words to a vector), YUV 8 x 2
template <int FMT> struct time_raw {
	static constexpr bool YUV = FMT >= PF_NV12;
	std::conditional_t<YUV, yuv_half, pf_raw<FMT == PF_XRGB32 ? PF_RGBA32 : FMT>> v;

	// YUV: sx a multiple of 8, sy even, sw a multiple of 8 and the frame 16-byte aligned; else the conditions of pf_load16
	__device__ __forceinline__ void load(const uint8_t* __restrict__ fr, uint32_t sw, uint32_t sh, uint32_t sx, uint32_t sy, bool row1)
	{
		if constexpr (YUV) {
			const size_t cw = sw >> 1, ch = (sh + 1) >> 1, py = sy >> 1;
			const uint8_t* c = fr + (size_t)sw * sh;
			v.y0 = __builtin_nontemporal_load(reinterpret_cast<const pf_u32x2*>(fr + (size_t)sy * sw + sx));
			v.y1 = 0;
			if (row1) v.y1 = __builtin_nontemporal_load(reinterpret_cast<const pf_u32x2*>(fr + ((size_t)sy + 1) * sw + sx));
			if constexpr (FMT == PF_NV12) v.c = __builtin_nontemporal_load(reinterpret_cast<const pf_u32x2*>(c + py * sw + sx));
			else {
				v.c[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(c + py * cw + (sx >> 1)));
				v.c[1] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(c + cw * ch + py * cw + (sx >> 1)));
			}
		} else v = pf_load16<FMT == PF_XRGB32 ? PF_RGBA32 : FMT, true>(fr, (size_t)sw * sh, (size_t)sy * sw + sx);
	}

	// pixel i of row rr (constants once the caller's loops are unrolled) as 0x00RRGGBB
	__device__ __forceinline__ uint32_t pixel(int rr, int i, const yuv_rd& m) const
	{
		if constexpr (YUV) {
			const int j = i >> 1;                                  // the chroma sample
			const uint32_t u = FMT == PF_NV12 ? v.c[j >> 1] >> (16 * (j & 1)) : v.c[0] >> (8 * j), w = FMT == PF_NV12 ? v.c[j >> 1] >> (16 * (j & 1) + 8) : v.c[1] >> (8 * j);
			return yuv_pixel(m, ((rr ? v.y1 : v.y0)[i >> 2] >> (8 * (i & 3))) & 0xff, yuv_chroma(m, u & 0xff, w & 0xff));
		} else if constexpr (FMT == PF_XRGB32) return v.v[i >> 2][i & 3] & 0xffffffu;
		else return pf_pixel<FMT>(v, i);
	}
};

template <int FMT> __global__ __launch_bounds__(256) void k_time(TimeArgs A)
{
	constexpr bool YUV = FMT >= PF_NV12;
	constexpr int ROWS = YUV ? 2 : 1, PX = YUV ? 8 : 16;           // a lane's pixels: PX of each of ROWS rows
	const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (item >= (size_t)(YUV ? (A.h + 1) >> 1 : A.h) * A.gpr) return;
	const uint32_t ri = (uint32_t)(item / A.gpr), c0 = (uint32_t)(item - (size_t)ri * A.gpr) * PX, r = YUV ? 2 * ri : ri;
	const uint32_t live = A.w - c0 < (uint32_t)PX ? A.w - c0 : (uint32_t)PX, sx = A.x + c0, sy = A.y + r;
	const bool row1 = YUV && r + 1 < A.h;
	const size_t p = (size_t)sy * A.sw + sx;                       // YUV: ld holds the conditions on x, y and sw
	const bool ld = A.ld && sx + PX <= A.sw && (YUV || (p & (FMT == PF_XRGB32 || FMT == PF_RGBA32 ? 3 : 15)) == 0);
	const unsigned long long sn = A.sn, dn = A.dn;
	for (uint32_t jj = blockIdx.y; jj < A.count; jj += gridDim.y) {
		const unsigned long long j = (unsigned long long)A.j0 + jj, lo = j * sn, hi = lo + sn;
		const uint32_t k0 = (uint32_t)(A.nearest ? (lo + hi) / (2 * dn) : lo / dn), k1 = A.nearest ? k0 : (uint32_t)((hi - 1) / dn);
		uint32_t acc[ROWS][PX][3];
#pragma unroll
		for (int rr = 0; rr < ROWS; rr++)
#pragma unroll
			for (int i = 0; i < PX; i++) acc[rr][i][0] = acc[rr][i][1] = acc[rr][i][2] = 0;
		time_raw<FMT> cur;
		if (ld) cur.load(A.src + ((size_t)A.first + (size_t)k0 * A.step) * A.frame_bytes, A.sw, A.sh, sx, sy, row1);
		for (uint32_t k = k0; k <= k1; k++) {
			const unsigned long long a = (unsigned long long)k * dn;
			const uint32_t wt = A.nearest ? A.sn : (uint32_t)(min(a + dn, hi) - max(a, lo));
			if (ld) {
				time_raw<FMT> nxt = cur;
				if (k < k1) nxt.load(A.src + ((size_t)A.first + (size_t)(k + 1) * A.step) * A.frame_bytes, A.sw, A.sh, sx, sy, row1);
#pragma unroll
				for (int rr = 0; rr < ROWS; rr++)
#pragma unroll
					for (int i = 0; i < PX; i++) {
						const uint32_t c = cur.pixel(rr, i, A.m);
						acc[rr][i][0] += wt * (c >> 16); acc[rr][i][1] += wt * ((c >> 8) & 0xffu); acc[rr][i][2] += wt * (c & 0xffu);
					}
				cur = nxt;
			} else {
				const uint8_t* fr = A.src + ((size_t)A.first + (size_t)k * A.step) * A.frame_bytes;
#pragma unroll
				for (int rr = 0; rr < ROWS; rr++)
#pragma unroll
					for (int i = 0; i < PX; i++) if ((uint32_t)i < live && (rr == 0 || row1)) {
						const uint32_t c = sc_read<FMT>(fr, A.sw, A.sh, sx + i, sy + rr, A.m);
						acc[rr][i][0] += wt * (c >> 16); acc[rr][i][1] += wt * ((c >> 8) & 0xffu); acc[rr][i][2] += wt * (c & 0xffu);
					}
			}
		}
		const uint32_t div = A.sn, half = div / 2;
		uint32_t* d = A.dst + ((size_t)jj * A.h + r) * A.w + c0;
#pragma unroll
		for (int rr = 0; rr < ROWS; rr++) {
			if (rr && !row1) break;
#pragma unroll
			for (int q = 0; q < PX / 4; q++) {
				if (4u * q >= live) break;
				pf_u32x4 o;
#pragma unroll
				for (int i = 0; i < 4; i++) o[i] = (acc[rr][4 * q + i][0] + half) / div << 16 | (acc[rr][4 * q + i][1] + half) / div << 8 | (acc[rr][4 * q + i][2] + half) / div;
				view_src_store4(d + (size_t)rr * A.w, q, o, live, A.st);
			}
		}
	}
}

// ---- a decoded XRGB32 clip written at a target size in any of the seven layouts (AGMV_SCALE_NEAREST / _BILINEAR of include/agmv.h) ----
// 1080p XRGB32 is 8.3 MB out per frame from 0.3 MB in, and the source batch stays in L2, so the taps are plain gathers.  A lane
// forms 16 consecutive target pixels of a row (YUV: 16 x 2, the patch of k_yuv_from_xrgb) in registers; where the target's rows of
// 16 lie on 16-byte boundaries they leave through pf_pack16 / yuv_pack_patch with 16-byte stores (k_scale_up_wide), so no XRGB32
// copy of the scaled clip exists.  Every other target -- a width that is no multiple of 16, a clip at an odd offset, a YUV frame
// with an odd last row -- goes pixel by pixel through the layout's byte writer (k_scale_up), to the same bytes.
// The taps of an axis: with p = (2X + 1) * s - d the floor quotient i = p div 2d (-1 where p < 0) and r = p mod 2d give the
// bilinear taps (i0 = max(i, 0), f = (256 r + d) div 2d, 0 where p < 0) and the nearest index i + (r >= d), since
// (2X + 1) * s = p + d.  A lane divides once per axis (in 32 bits where `small` says that every term fits) and then steps:
// p grows by 2s = 2d * (s div d) + 2 * (s mod d) per pixel, 256 r + d by 512 * (s mod d), both kept as quotient and remainder.
struct up_axis { uint32_t s, d, d2, q, m2, fq, fr; };              // d2 = 2d, q = s div d, m2 = 2 (s mod d), (fq, fr) = 512 (s mod d) divmod 2d
struct up_tap { int32_t i; uint32_t r, f, e; };                    // p = 2d i + r, 256 r + d = 2d f + e
struct up_idx { uint32_t i0, i1, f; };

struct UpArgs {
	const uint32_t* src;
	uint8_t* dst;
	size_t frame_bytes;                                            // of a target frame
	uint32_t bpf, gpr, rows;                                       // blocks per frame, groups of 16 per row, rows (YUV: row pairs; wide: bands) per frame
	int small;
	up_axis x, y;
	yuv_wr m;
	const void* table;                                             // PF_T32 / PF_T16: the 3 x 256 elements of agmv_hip_tensor_table, device memory
};

// ---- the target as a normalised float tensor clip (AGMV_TENSORFMT of include/agmv.h, which holds the definition) ----
// A frame is three planes [h][w] of elements R, G, B.  The writer computes nothing: element = T[c][channel c of the pixel], and the
// table holds the element type's bit patterns, so the only template axis is the element's size -- PF_T32 (AGMV_TENSOR_F32) or
// PF_T16 (AGMV_TENSOR_F16 and _BF16).  Every workgroup copies the 768 elements to LDS first.
#define PF_T32 32
#define PF_T16 33
template <int FMT> using ten_elem = std::conditional_t<FMT == PF_T16, uint16_t, uint32_t>;

// (every thread of the workgroup calls it, before any of them returns)
template <int FMT> __device__ __forceinline__ void ten_table_to_lds(ten_elem<FMT>* __restrict__ s_tab, const void* __restrict__ table)
{
	for (uint32_t k = threadIdx.x; k < 768; k += 256) s_tab[k] = static_cast<const ten_elem<FMT>*>(table)[k];
	__syncthreads();
}

template <bool BIL> __device__ __forceinline__ up_tap up_tap_at(const up_axis& a, uint32_t X, int small)
{
	up_tap t;
	if (small) {                                                   // p + 2d = (2X + 1) s + d > 0
		const uint32_t p2 = (2 * X + 1) * a.s + a.d, q = p2 / a.d2;
		t.i = (int32_t)q - 1; t.r = p2 - q * a.d2;
		if (BIL) { const uint32_t v = 256 * t.r + a.d; t.f = v / a.d2; t.e = v - t.f * a.d2; }
	} else {
		const unsigned long long p2 = (2ull * X + 1) * a.s + a.d, q = p2 / a.d2;
		t.i = (int32_t)q - 1; t.r = (uint32_t)(p2 - q * a.d2);
		if (BIL) { const unsigned long long v = 256ull * t.r + a.d; t.f = (uint32_t)(v / a.d2); t.e = (uint32_t)(v - (unsigned long long)t.f * a.d2); }
	}
	if (!BIL) { t.f = 0; t.e = 0; }
	return t;
}

template <bool BIL> __device__ __forceinline__ void up_tap_step(const up_axis& a, up_tap& t)
{
	t.i += (int32_t)a.q; t.r += a.m2;
	const bool wrap = t.r >= a.d2;
	if (wrap) { t.r -= a.d2; t.i++; }
	if (BIL) {
		t.f += a.fq; t.e += a.fr;
		if (t.e >= a.d2) { t.e -= a.d2; t.f++; }
		if (wrap) t.f -= 256;
	}
}

template <bool BIL> __device__ __forceinline__ up_idx up_resolve(const up_axis& a, const up_tap& t)
{
	up_idx x;
	if (BIL) {
		x.i0 = t.i < 0 ? 0u : (uint32_t)t.i; x.f = t.i < 0 ? 0u : t.f;
		x.i1 = min(x.i0 + 1, a.s - 1);
	} else {
		x.i0 = x.i1 = (uint32_t)(t.i + (t.r >= a.d ? 1 : 0)); x.f = 0;
	}
	return x;
}

// target pixel at column taps x of the row whose taps are source rows r0, r1 and fy
template <bool BIL> __device__ __forceinline__ uint32_t up_sample(const uint32_t* __restrict__ r0, const uint32_t* __restrict__ r1, const up_idx& x, uint32_t fy)
{
	if (!BIL) return r0[x.i0] & 0xffffffu;
	const uint32_t a = r0[x.i0], b = r0[x.i1], c = r1[x.i0], d = r1[x.i1], gx = 256 - x.f, gy = 256 - fy;
	uint32_t o = 0;
#pragma unroll
	for (int sh = 16; sh >= 0; sh -= 8) {
		const uint32_t top = gx * ((a >> sh) & 0xff) + x.f * ((b >> sh) & 0xff), bot = gx * ((c >> sh) & 0xff) + x.f * ((d >> sh) & 0xff);
		o |= ((gy * top + fy * bot + 32768u) >> 16) << sh;
	}
	return o;
}

// The wide kernel: a lane owns 16 columns of a band of UP_BAND target rows.  An upscale reads the same two source rows for several
// target rows (4.5 on average from 240 to 1080), so the lane keeps the horizontal pass of its 16 columns -- per column
// (256 - fx) * S(x0, y) + fx * S(x1, y) for both rows, exact in 16 bits per channel, R and B sharing a word -- in registers and forms
// them again only when the row's (y0, y1) change; a target row then costs the vertical pass and the stores.  NEAREST keeps the 16
// source pixels of the row.  A YUV lane keeps the 16 pixels of a pair's even row until the odd row is there (dh is even here).
#define UP_BAND 8

template <int FMT, bool BIL> __global__ __launch_bounds__(256) void k_scale_up_wide(UpArgs A)
{
	constexpr bool YUV = FMT == PF_NV12 || FMT == PF_I420, TEN = FMT >= PF_T32;
	__shared__ ten_elem<FMT> s_tab[TEN ? 768 : 1];
	if constexpr (TEN) ten_table_to_lds<FMT>(s_tab, A.table);
	const uint32_t f = blockIdx.x / A.bpf, g = (blockIdx.x - f * A.bpf) * 256 + threadIdx.x, band = g / A.gpr;
	if (band >= A.rows) return;
	const uint32_t dw = A.x.d, dh = A.y.d, sw = A.x.s, X0 = (g - band * A.gpr) * 16, Y0 = band * UP_BAND, Y1 = min(Y0 + UP_BAND, dh);
	const uint32_t* sf = A.src + (size_t)f * sw * A.y.s;
	uint8_t* fr = A.dst + (size_t)f * A.frame_bytes;
	const up_tap tx0 = up_tap_at<BIL>(A.x, X0, A.small);
	up_tap ty = up_tap_at<BIL>(A.y, Y0, A.small);
	uint32_t cy0 = 0xFFFFFFFFu, cy1 = 0xFFFFFFFFu;                 // the source rows the registers below were made from
	uint32_t h_rb0[16], h_rb1[16], h_g[16];                        // R << 16 | B of row y0, of row y1; G of y0 | G of y1 << 16 (NEAREST: h_rb0 = the pixels)
	// the 16 pixels of the target row ty stands at; ty moves on to the next row
	auto row = [&](pf_u32x4 out[4]) __attribute__((always_inline)) {
		const up_idx y = up_resolve<BIL>(A.y, ty);
		if (y.i0 != cy0 || y.i1 != cy1) {
			const uint32_t *r0 = sf + (size_t)y.i0 * sw, *r1 = sf + (size_t)y.i1 * sw;
			up_tap tx = tx0;
			// (opaque, so that the 16 columns' taps are stepped again at every refill, which is rare: hoisted out of the row loop
			// they take 100 registers more and halve the occupancy)
			asm volatile("" : "+v"(tx.i), "+v"(tx.r), "+v"(tx.f), "+v"(tx.e));
#pragma unroll
			for (int i = 0; i < 16; i++) {
				const up_idx x = up_resolve<BIL>(A.x, tx);
				if (BIL) {
					const uint32_t a = r0[x.i0], b = r0[x.i1], c = r1[x.i0], d = r1[x.i1], gx = 256 - x.f;
					h_rb0[i] = gx * (a & 0xff00ffu) + x.f * (b & 0xff00ffu);
					h_rb1[i] = gx * (c & 0xff00ffu) + x.f * (d & 0xff00ffu);
					h_g[i] = (gx * ((a >> 8) & 0xff) + x.f * ((b >> 8) & 0xff)) | (gx * ((c >> 8) & 0xff) + x.f * ((d >> 8) & 0xff)) << 16;
				} else {
					h_rb0[i] = r0[x.i0] & 0xffffffu;
				}
				up_tap_step<BIL>(A.x, tx);
			}
			cy0 = y.i0; cy1 = y.i1;
		}
		const uint32_t fy = y.f, gy = 256 - fy;
#pragma unroll
		for (int i = 0; i < 16; i++) {
			if (BIL) {
				const uint32_t r = (gy * (h_rb0[i] >> 16) + fy * (h_rb1[i] >> 16) + 32768u) >> 16;
				const uint32_t gg = (gy * (h_g[i] & 0xffffu) + fy * (h_g[i] >> 16) + 32768u) >> 16;
				const uint32_t b = (gy * (h_rb0[i] & 0xffffu) + fy * (h_rb1[i] & 0xffffu) + 32768u) >> 16;
				out[i >> 2][i & 3] = r << 16 | gg << 8 | b;
			} else {
				out[i >> 2][i & 3] = h_rb0[i];
			}
		}
		up_tap_step<BIL>(A.y, ty);
	};
	pf_u32x4 pa[4];                                                // YUV: the even row of the pair, kept until the odd row is there
	for (uint32_t Y = Y0; Y < Y1; Y++) {
		pf_u32x4 px[4];
		row(px);
		if constexpr (YUV) {                                       // (one copy of `row` in the loop, not two: its refill is what costs registers)
			if (!(Y & 1)) {
#pragma unroll
				for (int j = 0; j < 4; j++) pa[j] = px[j];
			} else {
				yuv_store_patch<FMT>(fr, dw, dh, X0, Y >> 1, yuv_pack_patch<FMT>(pa, px, A.m));
			}
		} else if constexpr (FMT == PF_XRGB32) {
#pragma unroll
			for (int j = 0; j < 4; j++) *reinterpret_cast<pf_u32x4*>(fr + 4 * ((size_t)Y * dw + X0) + 16 * j) = px[j];
		} else if constexpr (TEN) {                                // plane by plane: 16 elements are 64 (32) bytes, four (two) stores
			const size_t npx = (size_t)dw * dh;
			ten_elem<FMT>* o = reinterpret_cast<ten_elem<FMT>*>(fr) + (size_t)Y * dw + X0;
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const ten_elem<FMT>* t = s_tab + 256 * c;
				const int sh = 16 - 8 * c;
#pragma unroll
				for (int j = 0; j < (FMT == PF_T32 ? 4 : 2); j++) {
					pf_u32x4 v;
#pragma unroll
					for (int i = 0; i < 4; i++) {
						if constexpr (FMT == PF_T32) v[i] = t[(px[j][i] >> sh) & 0xffu];
						else v[i] = (uint32_t)t[(px[2 * j + (i >> 1)][2 * (i & 1)] >> sh) & 0xffu] | (uint32_t)t[(px[2 * j + (i >> 1)][2 * (i & 1) + 1] >> sh) & 0xffu] << 16;
					}
					*reinterpret_cast<pf_u32x4*>(reinterpret_cast<uint8_t*>(o + (size_t)c * npx) + 16 * j) = v;
				}
			}
		} else {
			const size_t npx = (size_t)dw * dh, p = (size_t)Y * dw + X0;
			const pf_raw<FMT> r = pf_pack16<FMT>(px);
#pragma unroll
			for (int j = 0; j < (FMT == PF_RGBA32 ? 4 : 3); j++)
				*reinterpret_cast<pf_u32x4*>(FMT == PF_RGB8P ? fr + (size_t)j * npx + p : fr + (FMT == PF_RGBA32 ? 4 : 3) * p + 16 * j) = r.v[j];
		}
	}
}

// Every other target, pixel by pixel: a lane owns 16 consecutive target pixels of one row (YUV: of a row pair, column pair by
// column pair, each with the chroma sample of the up to 2 x 2 pixels that exist).
template <int FMT, bool BIL> __global__ __launch_bounds__(256) void k_scale_up(UpArgs A)
{
	constexpr bool YUV = FMT == PF_NV12 || FMT == PF_I420, TEN = FMT >= PF_T32;
	__shared__ ten_elem<FMT> s_tab[TEN ? 768 : 1];
	if constexpr (TEN) ten_table_to_lds<FMT>(s_tab, A.table);
	const uint32_t f = blockIdx.x / A.bpf, g = (blockIdx.x - f * A.bpf) * 256 + threadIdx.x, ry = g / A.gpr;
	if (ry >= A.rows) return;
	const uint32_t dw = A.x.d, dh = A.y.d, sw = A.x.s, X0 = (g - ry * A.gpr) * 16, Y0 = YUV ? 2 * ry : ry;
	const uint32_t* sf = A.src + (size_t)f * sw * A.y.s;
	uint8_t* fr = A.dst + (size_t)f * A.frame_bytes;
	up_tap ty = up_tap_at<BIL>(A.y, Y0, A.small);
	const up_idx ya = up_resolve<BIL>(A.y, ty);
	const bool row1 = YUV && Y0 + 1 < dh;
	if (row1) up_tap_step<BIL>(A.y, ty);
	const up_idx yb = up_resolve<BIL>(A.y, ty);                   // (the row's own taps again where there is no second row)
	const uint32_t *a0 = sf + (size_t)ya.i0 * sw, *a1 = sf + (size_t)ya.i1 * sw, *b0 = sf + (size_t)yb.i0 * sw, *b1 = sf + (size_t)yb.i1 * sw;
	up_tap tx = up_tap_at<BIL>(A.x, X0, A.small);
	const size_t npx = (size_t)dw * dh;
	if constexpr (YUV) {
		const size_t cw = (dw + 1) >> 1, ch = (dh + 1) >> 1;
		for (uint32_t X = X0; X < X0 + 16 && X < dw; X += 2) {
			const bool two = X + 1 < dw;
			up_idx xi = up_resolve<BIL>(A.x, tx);
			const uint32_t p00 = up_sample<BIL>(a0, a1, xi, ya.f), p10 = row1 ? up_sample<BIL>(b0, b1, xi, yb.f) : 0u;
			up_tap_step<BIL>(A.x, tx);
			xi = up_resolve<BIL>(A.x, tx);
			const uint32_t p01 = two ? up_sample<BIL>(a0, a1, xi, ya.f) : 0u, p11 = two && row1 ? up_sample<BIL>(b0, b1, xi, yb.f) : 0u;
			up_tap_step<BIL>(A.x, tx);
			uint8_t* l = fr + (size_t)Y0 * dw + X;
			l[0] = (uint8_t)yuv_luma(A.m, p00);
			if (two) l[1] = (uint8_t)yuv_luma(A.m, p01);
			if (row1) { l[dw] = (uint8_t)yuv_luma(A.m, p10); if (two) l[dw + 1] = (uint8_t)yuv_luma(A.m, p11); }
			const uint32_t uv = yuv_uv(A.m, (int)(((p00 >> 16) & 0xff) + ((p01 >> 16) & 0xff) + ((p10 >> 16) & 0xff) + ((p11 >> 16) & 0xff)),
			                           (int)(((p00 >> 8) & 0xff) + ((p01 >> 8) & 0xff) + ((p10 >> 8) & 0xff) + ((p11 >> 8) & 0xff)),
			                           (int)((p00 & 0xff) + (p01 & 0xff) + (p10 & 0xff) + (p11 & 0xff)), (int)two + (int)row1);
			const size_t ci = (size_t)ry * cw + (X >> 1);
			uint8_t* c = fr + npx;
			if (FMT == PF_NV12) { c[2 * ci] = (uint8_t)uv; c[2 * ci + 1] = (uint8_t)(uv >> 8); }
			else { c[ci] = (uint8_t)uv; c[cw * ch + ci] = (uint8_t)(uv >> 8); }
		}
	} else {
		for (uint32_t X = X0; X < X0 + 16 && X < dw; X++) {
			const uint32_t c = up_sample<BIL>(a0, a1, up_resolve<BIL>(A.x, tx), ya.f);
			up_tap_step<BIL>(A.x, tx);
			if constexpr (FMT == PF_XRGB32) reinterpret_cast<uint32_t*>(fr)[(size_t)Y0 * dw + X] = c;
			else if constexpr (TEN) {
				ten_elem<FMT>* o = reinterpret_cast<ten_elem<FMT>*>(fr) + (size_t)Y0 * dw + X;
				o[0] = s_tab[(c >> 16) & 0xffu]; o[npx] = s_tab[256 + ((c >> 8) & 0xffu)]; o[2 * npx] = s_tab[512 + (c & 0xffu)];
			} else pf_write(FMT, fr, npx, (size_t)Y0 * dw + X, c);
		}
	}
}

// ---- a normalised float tensor clip read as XRGB32 (the reading rule of include/agmv.h: AGMV_TENSORFMT) ----
// An HBM stream: 12 (6) bytes in, 4 out per pixel.  A lane owns 8 consecutive pixels: per plane two (one) 16-byte loads, then two
// 16-byte stores, where every plane and every target frame starts on a 16-byte boundary (`vec`; that makes frame_pixels a
// multiple of 4 resp. 8); the frame's last partial group, and every pixel of any other clip, goes element by element.
#define TEN_F32 1
#define TEN_F16 2
#define TEN_BF16 3
struct ten_ab { float a[3], b[3]; };

// the element's bit pattern as the float32 of the same value, in integers: no conversion mode can touch it
template <int TYPE> __device__ __forceinline__ float ten_f32(uint32_t u)
{
	if (TYPE == TEN_F32) return __uint_as_float(u);
	if (TYPE == TEN_BF16) return __uint_as_float(u << 16);
	const uint32_t s = (u & 0x8000u) << 16, e = (u >> 10) & 31u, m = u & 0x3ffu;
	if (e == 0) return __uint_as_float(s | __float_as_uint((float)m * 0x1p-24f));      // m * 2^-24 is exact and a normal float32
	return __uint_as_float(s | (e == 31 ? 0x7f800000u : (e + 112) << 23) | m << 13);
}

// two separately rounded operations (never an fma), NaN = 0, round half to even
__device__ __forceinline__ uint32_t ten_byte(float x, float a, float b)
{
	const float t = __fadd_rn(__fmul_rn(x, a), b);
	return t != t ? 0u : (uint32_t)(int)rintf(fminf(fmaxf(t, 0.0f), 255.0f));
}

template <int TYPE> __device__ __forceinline__ uint32_t ten_read(const uint8_t* __restrict__ fr, size_t npx, size_t k, const ten_ab& ab)
{
	uint32_t x = 0;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const size_t i = (size_t)c * npx + k;
		const uint32_t u = TYPE == TEN_F32 ? reinterpret_cast<const uint32_t*>(fr)[i] : reinterpret_cast<const uint16_t*>(fr)[i];
		x = x << 8 | ten_byte(ten_f32<TYPE>(u), ab.a[c], ab.b[c]);
	}
	return x;
}

template <int TYPE> __global__ __launch_bounds__(256) void k_tensor_to_xrgb(const uint8_t* __restrict__ src, size_t npx, uint32_t bpf, int vec, ten_ab ab,
                                                                           uint32_t* __restrict__ dst)
{
	constexpr int ES = TYPE == TEN_F32 ? 4 : 2;
	const uint32_t f = blockIdx.x / bpf;
	const size_t g = (size_t)(blockIdx.x - f * bpf) * 256 + threadIdx.x, p = g * 8;
	const uint8_t* fr = src + (size_t)f * 3 * ES * npx;
	uint32_t* out = dst + (size_t)f * npx;
	if (vec && p + 8 <= npx) {
		uint32_t x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const pf_u32x4* a = reinterpret_cast<const pf_u32x4*>(fr + ((size_t)c * npx + p) * ES);
			const pf_u32x4 lo = __builtin_nontemporal_load(a);
			pf_u32x4 hi = 0;
			if (TYPE == TEN_F32) hi = __builtin_nontemporal_load(a + 1);
#pragma unroll
			for (int i = 0; i < 8; i++) {
				const uint32_t u = TYPE == TEN_F32 ? (i < 4 ? lo[i & 3] : hi[i & 3]) : (lo[i >> 1] >> (16 * (i & 1))) & 0xffffu;
				x[i] = x[i] << 8 | ten_byte(ten_f32<TYPE>(u), ab.a[c], ab.b[c]);
			}
		}
#pragma unroll
		for (int j = 0; j < 2; j++) {
			pf_u32x4 o;
#pragma unroll
			for (int i = 0; i < 4; i++) o[i] = x[4 * j + i];
			*reinterpret_cast<pf_u32x4*>(out + p + 4 * j) = o;
		}
	} else if (vec) {                                                  // the last, partial group of the frame
		for (int i = 0; i < 8; i++) if (p + i < npx) out[p + i] = ten_read<TYPE>(fr, npx, p + i, ab);
	} else {                                                           // lanes on consecutive pixels: the wave's 512, 64 at a time
		const size_t w0 = (g & ~(size_t)63) * 8 + (threadIdx.x & 63);
		for (int i = 0; i < 8; i++) if (w0 + 64 * i < npx) out[w0 + 64 * i] = ten_read<TYPE>(fr, npx, w0 + 64 * i, ab);
	}
}

// ---- a decoded clip measured against its reference (AGMV_FRAME_QUALITY of include/agmv.h, which holds the definition) ----
// The test clip is XRGB32, the reference in any of the seven layouts.  A workgroup owns one (frame, tile of MS_TW x MS_TH blocks) at
// a time, plus one block row below and one block column to the right of it, which only its windows use.  First a lane takes four
// neighbouring blocks of one block row (16 x 4 pixels): per pixel row 16 test pixels and 16 reference pixels -- four 16-byte
// loads of the test clip and the loads of sc_group<FMT> where the clip's frames start on 16-byte boundaries and (for the 3-byte
// and planar layouts) the 16 pixels start at a multiple of 16 of the frame's pixel index; the tile's one extra column, the tail
// of a row whose width is no multiple of 16 and every pixel of any other clip go through sc_read<FMT> -- and folds the five
// moments sum a, sum b, sum a^2, sum b^2, sum ab of each block and channel in registers, then stores the block's 15 dwords in LDS
// (each block of the tile has one writer).  After the barrier a lane takes owned blocks: a block's moments give its part of sse
// (sum a^2 + sum b^2 - 2 sum ab) and of block_sse, the moments of the 2 x 2 blocks at (bx, by) give one window, whose value is one
// Q20 division by 20 shift-and-subtract steps per channel.  The lane's sums go through the wave (__shfl_xor), then one 64-bit LDS
// atomic per wave and value, and the workgroup issues one 64-bit global atomic per value into the frame's entry.  All integer:
// any order of the adds gives the same sums.  Items are walked with a grid stride: any number of frames.
#define MS_TW 32
#define MS_TH 18
#define MS_NQ (MS_TW / 4 + 1)                                   // groups of four blocks per block row of a tile, the extra column included
#define MS_C1 26634ull                                          // floor(0.01^2 * 255^2 * 64^2 + 0.5)
#define MS_C2 235963ll                                          // floor(0.03^2 * 255^2 * 64 * 63 + 0.5)

struct MeasureArgs {
	const uint32_t* test;
	const uint8_t* ref;
	unsigned long long* out;                                       // [n_frames][12]: sse, block_sse, max_err, ssim, three channels each
	size_t frame_bytes;                                            // of the reference
	unsigned long long items;                                      // n_frames * tx * ty
	uint32_t w, h, tx, ty;
	int t_vec, wide;                                               // 16-byte loads allowed on the test clip, on the reference
	yuv_rd m;
};

// the SSIM of one window of 64 pixels in Q20, floor towards minus infinity: s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2,
// s12 = sum ab.  den > 0, |num| <= den < 2^58: the remainder stays below 2^59
__device__ __forceinline__ long long ms_ssim_q20(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12)
{
	const unsigned long long p11 = (unsigned long long)s1 * s1, p22 = (unsigned long long)s2 * s2, p12 = (unsigned long long)s1 * s2;
	const long long vars = (long long)(64ull * ss) - (long long)p11 - (long long)p22, cov = (long long)(64ull * s12) - (long long)p12;
	const long long t = 2 * cov + MS_C2;                            // carries the sign of num
	const unsigned long long den = (p11 + p22 + MS_C1) * (unsigned long long)(vars + MS_C2);
	const unsigned long long mag = (2 * p12 + MS_C1) * (unsigned long long)(t < 0 ? -t : t);
	unsigned long long q = mag >= den ? 1 : 0, r = mag - (q ? den : 0);
	for (int k = 0; k < 20; k++) {
		r <<= 1; q <<= 1;
		if (r >= den) { r -= den; q |= 1; }
	}
	return t < 0 ? -(long long)q - (r != 0) : (long long)q;
}

__device__ __forceinline__ unsigned long long ms_wave_sum(unsigned long long v)
{
	for (int d = 32; d; d >>= 1) {
		const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
		v += (unsigned long long)hi << 32 | lo;
	}
	return v;
}

template <int FMT> __global__ __launch_bounds__(256) void k_measure(MeasureArgs A)
{
	__shared__ uint32_t s_mom[MS_TH + 1][MS_TW + 1][15];              // per block and channel c: [5c] sum a, sum b, sum a^2, sum b^2, sum ab
	__shared__ unsigned long long s_red[12];
	const uint32_t w = A.w, h = A.h, bw = w >> 2, bh = h >> 2, per = A.tx * A.ty;
	const size_t npx = (size_t)w * h;
	if (threadIdx.x < 12) s_red[threadIdx.x] = 0;
	for (unsigned long long item = blockIdx.x; item < A.items; item += gridDim.x) {
		const uint32_t f = (uint32_t)(item / per), rem = (uint32_t)(item - (unsigned long long)f * per), ty = rem / A.tx, bx0 = (rem - ty * A.tx) * MS_TW, by0 = ty * MS_TH;
		const uint32_t nbx = min((uint32_t)MS_TW + 1, bw - bx0), nby = min((uint32_t)MS_TH + 1, bh - by0);     // the tile's blocks, the extra ones included
		const uint32_t* tf = A.test + (size_t)f * npx;
		const uint8_t* rf = A.ref + (size_t)f * A.frame_bytes;
		uint32_t mx[3] = { 0, 0, 0 };                              // (the extra blocks are pixels of the frame too: a maximum may count them twice)
		for (uint32_t task = threadIdx.x; task < nby * MS_NQ; task += 256) {
			const uint32_t jr = task / MS_NQ, qd = task - jr * MS_NQ;
			if (4 * qd >= nbx) continue;
			const uint32_t nb = min(4u, nbx - 4 * qd), x0 = (bx0 + 4 * qd) * 4;
			uint32_t acc[4][15];
#pragma unroll
			for (int q = 0; q < 4; q++)
#pragma unroll
				for (int k = 0; k < 15; k++) acc[q][k] = 0;
			for (uint32_t r = 0; r < 4; r++) {
				const uint32_t j = (by0 + jr) * 4 + r, p = j * w + x0;
				uint32_t ta[16], rb[16];                           // blocks the tile does not have read as 0 on both sides
				if (A.t_vec && nb == 4) {
					sc_group<PF_XRGB32> g;
					g.load(reinterpret_cast<const uint8_t*>(tf), w, h, p, j);
#pragma unroll
					for (int i = 0; i < 16; i++) ta[i] = g.pixel(i, A.m);
				} else {
#pragma unroll
					for (int i = 0; i < 16; i++) ta[i] = (uint32_t)(i >> 2) < nb ? tf[p + i] & 0xffffffu : 0u;
				}
				if (A.wide && nb == 4 && (sc_group<FMT>::NV == 4 || (p & 15) == 0)) {
					sc_group<FMT> g;
					g.load(rf, w, h, p, j);
#pragma unroll
					for (int i = 0; i < 16; i++) rb[i] = g.pixel(i, A.m);
				} else {
#pragma unroll
					for (int i = 0; i < 16; i++) rb[i] = (uint32_t)(i >> 2) < nb ? sc_read<FMT>(rf, w, h, x0 + i, j, A.m) : 0u;
				}
#pragma unroll
				for (int i = 0; i < 16; i++)
#pragma unroll
					for (int c = 0; c < 3; c++) {
						const uint32_t a = (ta[i] >> (16 - 8 * c)) & 0xff, b = (rb[i] >> (16 - 8 * c)) & 0xff;
						uint32_t* m = &acc[i >> 2][5 * c];
						m[0] += a; m[1] += b; m[2] += a * a; m[3] += b * b; m[4] += a * b;
						mx[c] = max(mx[c], a > b ? a - b : b - a);
					}
			}
#pragma unroll
			for (int q = 0; q < 4; q++) if ((uint32_t)q < nb) {
#pragma unroll
				for (int k = 0; k < 15; k++) s_mom[jr][4 * qd + q][k] = acc[q][k];
			}
		}
		__syncthreads();
		unsigned long long sse[3] = { 0, 0, 0 }, bsse[3] = { 0, 0, 0 }, ssim[3] = { 0, 0, 0 };
		const uint32_t own_x = min((uint32_t)MS_TW, bw - bx0), own_y = min((uint32_t)MS_TH, bh - by0);
		for (uint32_t k = threadIdx.x; k < own_y * MS_TW; k += 256) {
			const uint32_t ly = k / MS_TW, lx = k - ly * MS_TW;
			if (lx >= own_x) continue;
			const bool win = bx0 + lx + 1 < bw && by0 + ly + 1 < bh;
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const uint32_t* m = &s_mom[ly][lx][5 * c];
				const int d = (int)m[0] - (int)m[1];
				sse[c] += m[2] + m[3] - 2 * m[4];
				bsse[c] += (uint32_t)(d * d);
				if (win) {
					const uint32_t *m1 = &s_mom[ly][lx + 1][5 * c], *m2 = &s_mom[ly + 1][lx][5 * c], *m3 = &s_mom[ly + 1][lx + 1][5 * c];
					ssim[c] += (unsigned long long)ms_ssim_q20(m[0] + m1[0] + m2[0] + m3[0], m[1] + m1[1] + m2[1] + m3[1],
					                                           m[2] + m1[2] + m2[2] + m3[2] + m[3] + m1[3] + m2[3] + m3[3], m[4] + m1[4] + m2[4] + m3[4]);
				}
			}
		}
#pragma unroll
		for (int c = 0; c < 3; c++) {
			sse[c] = ms_wave_sum(sse[c]); bsse[c] = ms_wave_sum(bsse[c]); ssim[c] = ms_wave_sum(ssim[c]);
			for (int d = 32; d; d >>= 1) mx[c] = max(mx[c], (uint32_t)__shfl_xor(mx[c], d, 64));
		}
		if ((threadIdx.x & 63) == 0) {
#pragma unroll
			for (int c = 0; c < 3; c++) {
				atomicAdd(&s_red[c], sse[c]); atomicAdd(&s_red[3 + c], bsse[c]); atomicMax(&s_red[6 + c], (unsigned long long)mx[c]); atomicAdd(&s_red[9 + c], ssim[c]);
			}
		}
		__syncthreads();
		if (threadIdx.x < 12) {                                    // one global atomic per value; the signed sums add as their two's complement
			const unsigned long long v = s_red[threadIdx.x];
			unsigned long long* o = A.out + (size_t)f * 12 + threadIdx.x;
			s_red[threadIdx.x] = 0;
			if (v) { if (threadIdx.x >= 6 && threadIdx.x < 9) atomicMax(o, v); else atomicAdd(o, v); }
		}
	}
}

// ----------------------------------------------------------------------------------------------
// host side.  fmt is an AGMV_PIXFMT: 1 .. 5 the byte layouts, 16 (NV12) or 17 (I420), | 0x100 for BT.709, | 0x200 for full range
// ----------------------------------------------------------------------------------------------
static int yuv_base(int fmt) { return (fmt & ~0x3FF) == 0 && ((fmt & 0xFF) == PF_NV12 || (fmt & 0xFF) == PF_I420) ? fmt & 0xFF : 0; }
static int clip_base(int fmt) { return yuv_base(fmt) ? yuv_base(fmt) : fmt; }      // the layout: what the kernels are templated on

// the usual 8-bit fixed-point matrices, indexed by (fmt >> 8) & 3: BT.601 limited, BT.709 limited, BT.601 full, BT.709 full
static const yuv_rd YUV_RD[4] = { { 298, 16, 409, 100, 208, 516 }, { 298, 16, 459, 55, 136, 541 }, { 256, 0, 359, 88, 183, 454 }, { 256, 0, 403, 48, 120, 475 } };
static const yuv_wr YUV_WR[4] = { { 66, 129, 25, 16, -38, -74, 112, 112, -94, -18 }, { 47, 157, 16, 16, -26, -86, 112, 112, -102, -10 },
                                  { 77, 150, 29, 0, -43, -85, 128, 128, -107, -21 }, { 54, 183, 19, 0, -29, -99, 128, 128, -116, -12 } };

// bytes of a frame of w x h pixels in any layout (a byte layout only needs the product), 0 for an unknown one
static size_t clip_frame_bytes(int fmt, size_t w, size_t h)
{
	switch (clip_base(fmt)) {
	case PF_XRGB32: case PF_RGBA32: return 4 * w * h;
	case PF_RGB24: case PF_BGR24: case PF_RGB8P: return 3 * w * h;
	case PF_NV12: case PF_I420: return w * h + 2 * (size_t)(((uint32_t)w + 1) / 2) * (((uint32_t)h + 1) / 2);
	default: return 0;
	}
}

extern "C" size_t agmv_hip_pixfmt_frame_bytes(int fmt, size_t n_pixels) { return yuv_base(fmt) ? 0 : clip_frame_bytes(fmt, n_pixels, 1); }
extern "C" size_t agmv_hip_yuv_frame_bytes(int fmt, uint32_t w, uint32_t h) { return yuv_base(fmt) ? clip_frame_bytes(fmt, w, h) : 0; }

// The one place where a format becomes a kernel's template argument: launch(F) is called with F::value = the layout of fmt.
// SET has bit F set for every layout F the kernel is instantiated for; fmt has been checked to be one of them.
#define PF_BIT(F) (1u << (F))
constexpr unsigned PF_BYTES = PF_BIT(PF_RGB24) | PF_BIT(PF_BGR24) | PF_BIT(PF_RGBA32) | PF_BIT(PF_RGB8P), PF_YUV = PF_BIT(PF_NV12) | PF_BIT(PF_I420);

template <unsigned SET, class L> static void clip_dispatch(int fmt, L launch)
{
#define CLIP_CASE(F) case F: if constexpr ((SET & PF_BIT(F)) != 0) launch(std::integral_constant<int, F>()); break
	switch (clip_base(fmt)) {
	CLIP_CASE(PF_XRGB32); CLIP_CASE(PF_RGB24); CLIP_CASE(PF_BGR24); CLIP_CASE(PF_RGBA32); CLIP_CASE(PF_RGB8P); CLIP_CASE(PF_NV12); CLIP_CASE(PF_I420);
	}
#undef CLIP_CASE
}
#define CLIP_LAUNCH(SET, kernel, grid, ...) \
	clip_dispatch<SET>(fmt, [&](auto F) { hipLaunchKernelGGL(kernel<decltype(F)::value>, dim3(grid), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); })

// ---- argument checks that several entry points share ----
static int bad_pixfmt(int fmt)
{
	if (fmt >= PF_XRGB32 && fmt <= PF_RGB8P) return 0;
	return agmv_hip_err("agmv_hip: unknown pixel format %d", fmt);
}

static int bad_yuv(int fmt, uint32_t w, uint32_t h)
{
	if (!yuv_base(fmt)) return agmv_hip_err("agmv_hip: unknown pixel format 0x%x (a YUV 4:2:0 format is needed)", (unsigned)fmt);
	if (w == 0 || h == 0 || (unsigned long long)w * h > (1ull << 30)) return agmv_hip_err("agmv_hip: YUV frames of %u x %u", w, h);
	return 0;
}

// more pixels asked for than a frame has
static int pf_bad_count(size_t n, size_t frame_pixels) { return n > frame_pixels ? agmv_hip_err("agmv_hip: n_pixels %zu > frame_pixels %zu", n, frame_pixels) : 0; }
static int yuv_bad_count(size_t n, uint32_t w, uint32_t h) { return n > (size_t)w * h ? agmv_hip_err("agmv_hip: n_pixels %zu > %u x %u", n, w, h) : 0; }

// the grid of a gather kernel: one thread per entry of the table
static int gather_grid(size_t n_out, unsigned* blocks)
{
	if (n_out > ((size_t)1 << 39)) return agmv_hip_err("agmv_hip: gather table too long");
	*blocks = (unsigned)((n_out + 255) / 256);
	return 0;
}

// before a similarity launch: 1 = go on (the counts are cleared: the kernels add to them), 0 = no pair, nothing to do, -1 = error
static int sim_begin(size_t n_pixels, uint32_t n_frames, uint32_t* d_counts, void* stream)
{
	if (n_pixels == 0 || n_pixels > 0xFFFFFFFFu) return agmv_hip_err("agmv_hip: similarity needs 1 .. 2^32 - 1 pixels per frame");
	if (n_frames < 2) return 0;
	CK(hipMemsetAsync(d_counts, 0, 4 * (size_t)(n_frames - 1), (hipStream_t)stream));
	return 1;
}

// the grid of a kernel whose blocks each lie in one frame, `per` blocks per frame, if all of them fit
static int clip_grid(size_t per, uint32_t n_frames, uint32_t* bpf, unsigned* blocks)
{
	if (per * n_frames > 0x7FFFFFFFull) return agmv_hip_err("agmv_hip: clip too large for one launch");
	*bpf = (uint32_t)per; *blocks = (unsigned)(per * n_frames);
	return 0;
}

// clip_grid of the kernels that give a thread 16 pixels of one frame
static int pf_grid(size_t n_pixels, uint32_t n_frames, uint32_t* bpf, unsigned* blocks) { return clip_grid((n_pixels + 4095) / 4096, n_frames, bpf, blocks); }

// every frame of the clip (planes frame_pixels apart) starts on a 16-byte boundary
static int pf_aligned(int fmt, const void* d, size_t frame_pixels, uint32_t n_frames)
{
	if ((uintptr_t)d & 15) return 0;
	if (fmt == PF_RGB8P && (frame_pixels & 15)) return 0;
	return n_frames == 1 || (clip_frame_bytes(fmt, frame_pixels, 1) & 15) == 0;
}

// a clip whose patches of 16 x 2 pixels can be read and written with 16-byte (I420 chroma: 8-byte) accesses
static int yuv_wide(int fmt, const void* d, uint32_t w, uint32_t h, uint32_t n_frames)
{
	return (w & 15) == 0 && ((uintptr_t)d & 15) == 0 && (n_frames == 1 || (clip_frame_bytes(fmt, w, h) & 15) == 0);
}

// clip_grid of the kernels that give a thread 32 pixels of one frame: wide the patches of the rows that hold the first n_pixels,
// else runs of 32 pixels
static int yuv_grid(uint32_t w, size_t n_pixels, int wide, uint32_t n_frames, uint32_t* bpf, unsigned* blocks)
{
	const size_t rows = (n_pixels + w - 1) / w;
	return clip_grid(wide ? ((size_t)(w >> 4) * ((rows + 1) / 2) + 255) / 256 : (n_pixels + 8191) / 8192, n_frames, bpf, blocks);
}

// ---- XRGB32 clips ----
extern "C" int agmv_hip_synth_dev(agmv_hip_ctx* c, uint32_t* d_pix, uint32_t w, uint32_t h, uint32_t t0, uint32_t n_frames,
                                  uint64_t seed, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (w < 2 || h < 2 || n_frames == 0) return agmv_hip_err("agmv_hip: bad synth geometry");
	hipLaunchKernelGGL(k_synth, dim3(8192), dim3(256), 0, (hipStream_t)stream, d_pix, w, h, t0, n_frames, seed);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_interp_dev(agmv_hip_ctx* c, uint32_t* d_out, const uint32_t* d_f1, const uint32_t* d_f2, size_t n, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n == 0) return 0;
	size_t blocks = (n + 255) / 256;
	if (blocks > 8192) blocks = 8192;
	hipLaunchKernelGGL(k_interp, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_out, d_f1, d_f2, n);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_histogram_dev(agmv_hip_ctx* c, const uint32_t* d_pix, size_t n, int quality, uint32_t* d_hist, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n == 0) return 0;
	size_t blocks = (n + 255) / 256;
	if (blocks > 8192) blocks = 8192;
	hipLaunchKernelGGL(k_histogram, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_pix, n, quality, d_hist);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_similarity_dev(agmv_hip_ctx* c, const uint32_t* d_pix, uint32_t n_frames, size_t n_pixels, uint32_t* d_counts, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const int go = sim_begin(n_pixels, n_frames, d_counts, stream);
	if (go <= 0) return go;
	const size_t blocks = (n_pixels + 2047) / 2048;            // 256 lanes x 8 pixels
	const int vec = (n_pixels & 3) == 0 && ((uintptr_t)d_pix & 15) == 0;
	hipLaunchKernelGGL(k_similarity, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_pix, n_frames, n_pixels, vec, d_counts);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_gather_dev(agmv_hip_ctx* c, const uint32_t* d_src, size_t src_frame_pixels, uint32_t n_frames, const uint32_t* d_index,
                                   size_t n_out, uint32_t* d_dst, void* stream)
{
	unsigned blocks;
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0 || n_out == 0) return 0;
	if (gather_grid(n_out, &blocks)) return -1;
	hipLaunchKernelGGL(k_gather, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_src, src_frame_pixels, n_frames, d_index, n_out, d_dst);
	CK(hipGetLastError());
	return 0;
}

// the frames a launch of k_view spreads over blockIdx.y; a longer view takes further trips round the kernel's frame loop
#define VIEW_GRID_FRAMES 65535u

extern "C" int agmv_hip_view_frames_async(agmv_hip_ctx* c, const uint32_t* d_src, uint32_t src_w, uint32_t src_h, uint32_t first, uint32_t step, uint32_t count,
                                          uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t* d_dst, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (!d_src || !d_dst || src_w == 0 || src_h == 0 || w == 0 || h == 0 || step == 0) return agmv_hip_err("agmv_hip: view needs clips, sizes and a step that are not zero");
	if (x > src_w || w > src_w - x || y > src_h || h > src_h - y)
		return agmv_hip_err("agmv_hip: the window %u x %u at (%u, %u) does not lie inside the %u x %u frame", w, h, x, y, src_w, src_h);
	if (count == 0) return 0;
	const uint32_t gpr = w / 4 + ((w & 3) != 0);               // groups of 4 pixels per output row
	const size_t items = (size_t)h * gpr;
	if (items > 0xFFFFFFFFull) return agmv_hip_err("agmv_hip: window too large for one launch");
	const dim3 grid((unsigned)((items + 255) / 256), count < VIEW_GRID_FRAMES ? count : VIEW_GRID_FRAMES);
	const size_t src_px = (size_t)src_w * src_h;
	const bool ld4 = (x & 3) == 0 && (src_w & 3) == 0 && ((uintptr_t)d_src & 15) == 0, st4 = (w & 3) == 0 && ((uintptr_t)d_dst & 15) == 0;
#define VIEW_LAUNCH(L, S) hipLaunchKernelGGL((k_view<L, S>), grid, dim3(256), 0, (hipStream_t)stream, d_src, src_w, src_px, first, step, count, x, y, w, h, gpr, d_dst)
	if (ld4 && st4) VIEW_LAUNCH(true, true);
	else if (ld4) VIEW_LAUNCH(true, false);
	else if (st4) VIEW_LAUNCH(false, true);
	else VIEW_LAUNCH(false, false);
#undef VIEW_LAUNCH
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_view_source_async(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t src_w, uint32_t src_h, uint32_t first, uint32_t step, uint32_t count,
                                          uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t* d_dst, void* stream)
{
	if (fmt == PF_XRGB32) return agmv_hip_view_frames_async(c, (const uint32_t*)d_src, src_w, src_h, first, step, count, x, y, w, h, d_dst, stream);
	if (agmv_hip_enter(c)) return -1;
	if (!d_src || !d_dst || src_w == 0 || src_h == 0 || w == 0 || h == 0 || step == 0) return agmv_hip_err("agmv_hip: view needs clips, sizes and a step that are not zero");
	if (x > src_w || w > src_w - x || y > src_h || h > src_h - y)
		return agmv_hip_err("agmv_hip: the window %u x %u at (%u, %u) does not lie inside the %u x %u frame", w, h, x, y, src_w, src_h);
	const int yuv = yuv_base(fmt);
	if (yuv ? bad_yuv(fmt, src_w, src_h) : bad_pixfmt(fmt)) return -1;
	if (yuv && ((src_w | src_h) & 1)) return agmv_hip_err("agmv_hip: a view of a YUV 4:2:0 source needs an even frame size, got %u x %u", src_w, src_h);
	if (count == 0) return 0;
	ViewSrcArgs A;
	A.src = (const uint8_t*)d_src; A.dst = d_dst; A.frame_bytes = clip_frame_bytes(fmt, src_w, src_h);
	A.sw = src_w; A.sh = src_h; A.first = first; A.step = step; A.count = count; A.x = x; A.y = y; A.w = w; A.h = h;
	A.gpr = w / 16 + ((w & 15) != 0);                          // groups of 16 pixels per output row
	A.m = YUV_RD[(fmt >> 8) & 3];
	// the source groups of the window's rows on 16-byte boundaries: RGBA32 needs multiples of 4 pixels, the byte-per-sample layouts of 16
	const uint32_t px = fmt == PF_RGBA32 ? 3u : 15u;
	A.ld = ((x | src_w) & px) == 0 && ((uintptr_t)d_src & 15) == 0 && !(yuv && (y & 1));
	A.st = (w & 3) == 0 && ((uintptr_t)d_dst & 15) == 0;
	const size_t items = (size_t)(yuv ? (h + 1) / 2 : h) * A.gpr;
	if (items > 0xFFFFFFFFull) return agmv_hip_err("agmv_hip: window too large for one launch");
	const dim3 grid((unsigned)((items + 255) / 256), count < VIEW_GRID_FRAMES ? count : VIEW_GRID_FRAMES);
	clip_dispatch<PF_BYTES | PF_YUV>(fmt, [&](auto F) { hipLaunchKernelGGL(k_view_src<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, A); });
	CK(hipGetLastError());
	return 0;
}

static uint32_t time_gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

extern "C" int agmv_hip_time_frames_async(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t src_w, uint32_t src_h, uint32_t n_frames, uint32_t first, uint32_t step,
                                          uint32_t view_len, uint32_t x, uint32_t y, uint32_t win_w, uint32_t win_h, uint32_t rate_src, uint32_t rate_dst, int time_filter,
                                          uint32_t j0, uint32_t count, uint32_t* d_dst, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (!d_src || !d_dst || src_w == 0 || src_h == 0 || win_w == 0 || win_h == 0 || step == 0) return agmv_hip_err("agmv_hip: time needs clips, sizes and a step that are not zero");
	if (x > src_w || win_w > src_w - x || y > src_h || win_h > src_h - y)
		return agmv_hip_err("agmv_hip: the window %u x %u at (%u, %u) does not lie inside the %u x %u frame", win_w, win_h, x, y, src_w, src_h);
	const int yuv = yuv_base(fmt);
	if (yuv ? bad_yuv(fmt, src_w, src_h) : bad_pixfmt(fmt)) return -1;
	if (yuv && ((src_w | src_h) & 1)) return agmv_hip_err("agmv_hip: a view of a YUV 4:2:0 source needs an even frame size, got %u x %u", src_w, src_h);
	if (time_filter != 1 && time_filter != 2) return agmv_hip_err("agmv_hip: unknown time filter %d", time_filter);
	if (rate_src == 0 || rate_dst == 0 || rate_src > 65535u || rate_dst > 65535u || time_gcd(rate_src, rate_dst) != 1)
		return agmv_hip_err("agmv_hip: the rate %u : %u is not a reduced pair of 1 .. 65535", rate_src, rate_dst);
	if (time_filter == 2 && rate_dst > rate_src) return agmv_hip_err("agmv_hip: the box filter in time does not raise the rate (%u : %u)", rate_src, rate_dst);
	const unsigned long long m = (unsigned long long)view_len * rate_dst / rate_src;
	if ((unsigned long long)j0 + count > m) return agmv_hip_err("agmv_hip: frames %u .. %llu of a result of %llu", j0, (unsigned long long)j0 + count, m);
	if (view_len && (unsigned long long)first + (unsigned long long)(view_len - 1) * step >= n_frames)
		return agmv_hip_err("agmv_hip: a tap of the view (first %u, step %u, %u frames) lies outside the clip of %u frames", first, step, view_len, n_frames);
	if (count == 0) return 0;
	TimeArgs A;
	A.src = (const uint8_t*)d_src; A.dst = d_dst; A.frame_bytes = clip_frame_bytes(fmt, src_w, src_h);
	A.sw = src_w; A.sh = src_h; A.first = first; A.step = step; A.x = x; A.y = y; A.w = win_w; A.h = win_h;
	A.gpr = yuv ? win_w / 8 + ((win_w & 7) != 0) : win_w / 16 + ((win_w & 15) != 0);      // groups of 16 (YUV: 8) pixels per output row
	A.sn = rate_src; A.dn = rate_dst; A.j0 = j0; A.count = count; A.nearest = time_filter == 1;
	A.m = YUV_RD[(fmt >> 8) & 3];
	// every frame (and plane) on a 16-byte boundary; YUV: and the window's patches of 8 x 2 on 8-byte boundaries of rows that share
	// a chroma row (I420: its chroma on 4-byte ones).  The byte layouts leave the group's own offset to the lane.
	A.ld = ((uintptr_t)d_src & 15) == 0 && (A.frame_bytes & 15) == 0 &&
	       (yuv ? ((x | src_w) & 7) == 0 && !(y & 1) : fmt != PF_RGB8P || ((size_t)src_w * src_h & 15) == 0);
	A.st = (win_w & 3) == 0 && ((uintptr_t)d_dst & 15) == 0;
	const size_t items = (size_t)(yuv ? (win_h + 1) / 2 : win_h) * A.gpr;
	if (items > 0xFFFFFFFFull) return agmv_hip_err("agmv_hip: window too large for one launch");
	const dim3 grid((unsigned)((items + 255) / 256), count < VIEW_GRID_FRAMES ? count : VIEW_GRID_FRAMES);
	clip_dispatch<PF_BIT(PF_XRGB32) | PF_BYTES | PF_YUV>(fmt, [&](auto F) { hipLaunchKernelGGL(k_time<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, A); });
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_stabilise_frames_async(agmv_hip_ctx* c, uint32_t strength, uint32_t* d_pix, uint32_t w, uint32_t h, uint32_t n_frames,
                                               uint32_t first_fc, unsigned long long* d_replaced, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (!d_pix || ((uintptr_t)d_pix & 3u)) return agmv_hip_err("agmv_hip: stabilise: d_pix must be a 4-byte aligned device pointer");
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (strength < 1 || strength > 64) return agmv_hip_err("agmv_hip: stabilise: strength must be 1 .. 64 (got %u)", strength);
	const uint32_t lead = (4u - (first_fc & 3u)) & 3u;         // frames whose I-frame lies before the batch
	if (n_frames < lead + 2u) return 0;                        // no P-frame with its I-frame in the batch
	const uint32_t n_gops = (n_frames - lead - 2u) / 4u + 1u, bw = w / 4u, nblk = bw * (h / 4u);
	const dim3 grid((nblk + STAB_T - 1) / STAB_T, n_gops < STAB_GRID_GOPS ? n_gops : STAB_GRID_GOPS);
#define STAB_LAUNCH(V) hipLaunchKernelGGL((k_stabilise<V>), grid, dim3(STAB_T), 0, (hipStream_t)stream, d_pix, w, bw, nblk, (size_t)w * h, n_frames, lead, n_gops, strength, d_replaced)
	if (((uintptr_t)d_pix & 15u) == 0) STAB_LAUNCH(true);
	else STAB_LAUNCH(false);
#undef STAB_LAUNCH
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_deblock_frames_async(agmv_hip_ctx* c, uint32_t strength, const uint32_t* d_src, uint32_t w, uint32_t h, uint32_t n_frames,
                                             uint32_t* d_dst, unsigned long long* d_counts, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (!d_src || ((uintptr_t)d_src & 3u) || !d_dst || ((uintptr_t)d_dst & 3u))
		return agmv_hip_err("agmv_hip: deblock: d_src and d_dst must be 4-byte aligned device pointers");
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (strength < 1 || strength > 64) return agmv_hip_err("agmv_hip: deblock: strength must be 1 .. 64 (got %u)", strength);
	if (n_frames == 0) return 0;
	const uint32_t cw = w / 4u + 1u, bh = h / 4u, ncell = cw * (bh + 1u), gx = (ncell + DBK_T - 1) / DBK_T;
	uint32_t gy = DBK_GRID_BLOCKS / gx;
	if (gy < 1u) gy = 1u;
	if (gy > DBK_GRID_FRAMES) gy = DBK_GRID_FRAMES;
	if (gy > n_frames) gy = n_frames;
	const dim3 grid(gx, gy);
#define DBK_LAUNCH(V) hipLaunchKernelGGL((k_deblock<V>), grid, dim3(DBK_T), 0, (hipStream_t)stream, d_src, d_dst, w, cw, bh, ncell, (size_t)w * h, n_frames, strength, d_counts)
	if ((((uintptr_t)d_src | (uintptr_t)d_dst) & 7u) == 0) DBK_LAUNCH(true);
	else DBK_LAUNCH(false);
#undef DBK_LAUNCH
	CK(hipGetLastError());
	return 0;
}

// ---- the same on clips in the caller's pixel layout ----
extern "C" int agmv_hip_pixels_to_xrgb_dev(agmv_hip_ctx* c, int fmt, const void* d_src, size_t frame_pixels, uint32_t n_frames, size_t n_pixels,
                                           uint32_t* d_dst, void* stream)
{
	if (agmv_hip_enter(c) || bad_pixfmt(fmt) || pf_bad_count(n_pixels, frame_pixels)) return -1;
	if (n_frames == 0 || n_pixels == 0) return 0;
	if (fmt == PF_XRGB32) {
		if (n_frames == 1 || n_pixels == frame_pixels) CK(hipMemcpyAsync(d_dst, d_src, (size_t)n_frames * n_pixels * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
		else CK(hipMemcpy2DAsync(d_dst, n_pixels * 4, d_src, frame_pixels * 4, n_pixels * 4, n_frames, hipMemcpyDeviceToDevice, (hipStream_t)stream));
		return 0;
	}
	uint32_t bpf; unsigned blocks;
	if (pf_grid(n_pixels, n_frames, &bpf, &blocks)) return -1;
	const int wide = pf_aligned(fmt, d_src, frame_pixels, n_frames) && pf_aligned(PF_XRGB32, d_dst, n_pixels, n_frames);
	CLIP_LAUNCH(PF_BYTES, k_pix_to_xrgb, blocks, (const uint8_t*)d_src, frame_pixels, clip_frame_bytes(fmt, frame_pixels, 1), n_pixels, bpf, wide, d_dst);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_pixels_from_xrgb_dev(agmv_hip_ctx* c, int fmt, const uint32_t* d_src, uint32_t n_frames, size_t n_pixels, void* d_dst, void* stream)
{
	if (agmv_hip_enter(c) || bad_pixfmt(fmt)) return -1;
	if (n_frames == 0 || n_pixels == 0) return 0;
	if (fmt == PF_XRGB32) {
		CK(hipMemcpyAsync(d_dst, d_src, (size_t)n_frames * n_pixels * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
		return 0;
	}
	uint32_t bpf; unsigned blocks;
	if (pf_grid(n_pixels, n_frames, &bpf, &blocks)) return -1;
	const int wide = pf_aligned(fmt, d_dst, n_pixels, n_frames) && pf_aligned(PF_XRGB32, d_src, n_pixels, n_frames);
	CLIP_LAUNCH(PF_BYTES, k_pix_from_xrgb, blocks, d_src, n_pixels, clip_frame_bytes(fmt, n_pixels, 1), bpf, wide, (uint8_t*)d_dst);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_gather_fmt_dev(agmv_hip_ctx* c, int fmt, const void* d_src, size_t src_frame_pixels, uint32_t n_frames, const uint32_t* d_index,
                                       size_t n_out, uint32_t* d_dst, void* stream)
{
	unsigned blocks;
	if (agmv_hip_enter(c) || bad_pixfmt(fmt)) return -1;
	if (fmt == PF_XRGB32) return agmv_hip_gather_dev(c, (const uint32_t*)d_src, src_frame_pixels, n_frames, d_index, n_out, d_dst, stream);
	if (n_frames == 0 || n_out == 0) return 0;
	if (gather_grid(n_out, &blocks)) return -1;
	hipLaunchKernelGGL(k_gather_fmt, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_src, fmt, src_frame_pixels,
	                   clip_frame_bytes(fmt, src_frame_pixels, 1), n_frames, d_index, n_out, d_dst);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_histogram_fmt_dev(agmv_hip_ctx* c, int fmt, const void* d_src, size_t frame_pixels, uint32_t n_frames, size_t n_pixels, int quality,
                                          uint32_t* d_hist, void* stream)
{
	if (agmv_hip_enter(c) || bad_pixfmt(fmt) || pf_bad_count(n_pixels, frame_pixels)) return -1;
	if (n_frames == 0 || n_pixels == 0) return 0;
	if (fmt == PF_XRGB32) {
		const uint32_t* d_pix = (const uint32_t*)d_src;
		if (n_pixels == frame_pixels) return agmv_hip_histogram_dev(c, d_pix, (size_t)n_frames * frame_pixels, quality, d_hist, stream);   // one run of pixels
		for (uint32_t f = 0; f < n_frames; f++) if (agmv_hip_histogram_dev(c, d_pix + (size_t)f * frame_pixels, n_pixels, quality, d_hist, stream)) return -1;
		return 0;
	}
	uint32_t bpf; unsigned blocks;
	if (pf_grid(n_pixels, n_frames, &bpf, &blocks)) return -1;
	const int wide = pf_aligned(fmt, d_src, frame_pixels, n_frames);
	CLIP_LAUNCH(PF_BYTES, k_histogram_fmt, blocks, (const uint8_t*)d_src, frame_pixels, clip_frame_bytes(fmt, frame_pixels, 1), n_pixels, bpf, wide, quality, d_hist);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_similarity_fmt_dev(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t n_frames, size_t n_pixels, uint32_t* d_counts, void* stream)
{
	if (agmv_hip_enter(c) || bad_pixfmt(fmt)) return -1;
	if (fmt == PF_XRGB32) return agmv_hip_similarity_dev(c, (const uint32_t*)d_src, n_frames, n_pixels, d_counts, stream);
	const int go = sim_begin(n_pixels, n_frames, d_counts, stream);
	if (go <= 0) return go;
	const unsigned blocks = (unsigned)((n_pixels + 4095) / 4096);    // 256 lanes x 16 pixels
	const int vec = (n_pixels & 15) == 0 && ((uintptr_t)d_src & 15) == 0;
	const size_t frame_bytes = clip_frame_bytes(fmt, n_pixels, 1);
	if (fmt == PF_BGR24) fmt = PF_RGB24;                         // the grey is a sum: the two 3-byte orders are one kernel
	CLIP_LAUNCH(PF_BYTES & ~PF_BIT(PF_BGR24), k_similarity_fmt, blocks, (const uint8_t*)d_src, n_frames, n_pixels, frame_bytes, vec, d_counts);
	CK(hipGetLastError());
	return 0;
}

// ---- the same on clips in 8-bit YUV 4:2:0 ----
extern "C" int agmv_hip_yuv_to_xrgb_dev(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames, size_t n_pixels, uint32_t* d_dst,
                                        void* stream)
{
	if (agmv_hip_enter(c) || bad_yuv(fmt, w, h) || yuv_bad_count(n_pixels, w, h)) return -1;
	if (n_frames == 0 || n_pixels == 0) return 0;
	uint32_t bpf; unsigned blocks;
	const int wide = yuv_wide(fmt, d_src, w, h, n_frames) && pf_aligned(PF_XRGB32, d_dst, n_pixels, n_frames);
	if (yuv_grid(w, n_pixels, wide, n_frames, &bpf, &blocks)) return -1;
	CLIP_LAUNCH(PF_YUV, k_yuv_to_xrgb, blocks, (const uint8_t*)d_src, w, h, clip_frame_bytes(fmt, w, h), (uint32_t)n_pixels, bpf, wide, YUV_RD[(fmt >> 8) & 3], d_dst);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_yuv_from_xrgb_dev(agmv_hip_ctx* c, int fmt, const uint32_t* d_src, uint32_t w, uint32_t h, uint32_t n_frames, void* d_dst, void* stream)
{
	if (agmv_hip_enter(c) || bad_yuv(fmt, w, h)) return -1;
	if (n_frames == 0) return 0;
	uint32_t bpf; unsigned blocks;
	const int wide = yuv_wide(fmt, d_dst, w, h, n_frames) && pf_aligned(PF_XRGB32, d_src, (size_t)w * h, n_frames);
	if (yuv_grid(w, (size_t)w * h, wide, n_frames, &bpf, &blocks)) return -1;
	CLIP_LAUNCH(PF_YUV, k_yuv_from_xrgb, blocks, d_src, w, h, clip_frame_bytes(fmt, w, h), bpf, wide, YUV_WR[(fmt >> 8) & 3], (uint8_t*)d_dst);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_yuv_gather_dev(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames, const uint32_t* d_index, size_t n_out,
                                       uint32_t* d_dst, void* stream)
{
	unsigned blocks;
	if (agmv_hip_enter(c) || bad_yuv(fmt, w, h)) return -1;
	if (n_frames == 0 || n_out == 0) return 0;
	if (gather_grid(n_out, &blocks)) return -1;
	CLIP_LAUNCH(PF_YUV, k_yuv_gather, blocks, (const uint8_t*)d_src, w, h, clip_frame_bytes(fmt, w, h), n_frames, d_index, n_out, YUV_RD[(fmt >> 8) & 3], d_dst);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_yuv_histogram_dev(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames, size_t n_pixels, int quality,
                                          uint32_t* d_hist, void* stream)
{
	if (agmv_hip_enter(c) || bad_yuv(fmt, w, h) || yuv_bad_count(n_pixels, w, h)) return -1;
	if (n_frames == 0 || n_pixels == 0) return 0;
	uint32_t bpf; unsigned blocks;
	const int wide = yuv_wide(fmt, d_src, w, h, n_frames);
	if (yuv_grid(w, n_pixels, wide, n_frames, &bpf, &blocks)) return -1;
	CLIP_LAUNCH(PF_YUV, k_yuv_histogram, blocks, (const uint8_t*)d_src, w, h, clip_frame_bytes(fmt, w, h), (uint32_t)n_pixels, bpf, wide, quality, YUV_RD[(fmt >> 8) & 3],
	            d_hist);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_yuv_similarity_dev(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames, uint32_t* d_counts, void* stream)
{
	if (agmv_hip_enter(c) || bad_yuv(fmt, w, h)) return -1;
	const int go = sim_begin((size_t)w * h, n_frames, d_counts, stream);
	if (go <= 0) return go;
	const unsigned blocks = (unsigned)(((size_t)((w + 15) >> 4) * ((h + 1) >> 1) + 255) / 256);    // 256 lanes x one patch
	const int wide = yuv_wide(fmt, d_src, w, h, n_frames);
	CLIP_LAUNCH(PF_YUV, k_yuv_similarity, blocks, (const uint8_t*)d_src, n_frames, w, h, clip_frame_bytes(fmt, w, h), wide, YUV_RD[(fmt >> 8) & 3], d_counts);
	CK(hipGetLastError());
	return 0;
}

// ---- the exact box-filter downscale (AGMV_SCALE_AREA) of a clip in any layout ----
extern "C" int agmv_hip_scale_area_dev(agmv_hip_ctx* c, int fmt, const void* d_src, uint32_t src_w, uint32_t src_h, uint32_t n_frames, uint32_t dst_w, uint32_t dst_h,
                                       uint32_t* d_dst, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const int yuv = yuv_base(fmt);
	if (!yuv && bad_pixfmt(fmt)) return -1;
	if (src_w == 0 || src_h == 0 || dst_w == 0 || dst_h == 0 || dst_w > src_w || dst_h > src_h || (unsigned long long)src_w * src_h > (1ull << 24))
		return agmv_hip_err("agmv_hip: area scale of %u x %u to %u x %u (a downscale of at most 2^24 source pixels is needed)", src_w, src_h, dst_w, dst_h);
	if (n_frames == 0) return 0;
	ScaleArgs A;
	A.src = (const uint8_t*)d_src; A.dst = d_dst;
	A.frame_bytes = clip_frame_bytes(fmt, src_w, src_h);
	A.sw = src_w; A.sh = src_h; A.dw = dst_w; A.dh = dst_h; A.tiles = (dst_w + SC_TILE - 1) / SC_TILE;
	A.items = (unsigned long long)n_frames * dst_h * A.tiles;
	A.wide = yuv ? yuv_wide(fmt, d_src, src_w, src_h, n_frames) : pf_aligned(fmt, d_src, (size_t)src_w * src_h, n_frames);
	A.small = (unsigned long long)src_w * dst_w < (1ull << 32);
	A.m = YUV_RD[(fmt >> 8) & 3];
	CLIP_LAUNCH(PF_BYTES | PF_YUV | PF_BIT(PF_XRGB32), k_scale_area, (unsigned)(A.items < 65536 ? A.items : 65536), A);
	CK(hipGetLastError());
	return 0;
}

// ---- a decoded XRGB32 clip at a target size in any layout (AGMV_SCALE_NEAREST / AGMV_SCALE_BILINEAR) ----
static up_axis up_axis_of(uint32_t s, uint32_t d)
{
	up_axis a;
	const unsigned long long k = 512ull * (s % d);
	a.s = s; a.d = d; a.d2 = 2 * d; a.q = s / d; a.m2 = 2 * (s % d); a.fq = (uint32_t)(k / a.d2); a.fr = (uint32_t)(k % a.d2);
	return a;
}

// (2X + 1) * s + d for every X < d, and 256 * r + d for every r < 2d, fit 32 bits
static int up_small(uint32_t s, uint32_t d) { return (2ull * d - 1) * s + d < (1ull << 32) && 513ull * d < (1ull << 32); }

// what the four scaling kernels share: the grid (wide: bands of 16 columns; else rows, or YUV row pairs) and the taps of both axes
static int up_geometry(UpArgs& A, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, uint32_t n_frames, int wide, int yuv, unsigned* blocks)
{
	A.gpr = (dst_w + 15) >> 4; A.rows = wide ? (dst_h + UP_BAND - 1) / UP_BAND : yuv ? (dst_h + 1) >> 1 : dst_h;
	A.small = up_small(src_w, dst_w) && up_small(src_h, dst_h);
	A.x = up_axis_of(src_w, dst_w); A.y = up_axis_of(src_h, dst_h);
	return clip_grid(((size_t)A.gpr * A.rows + 255) / 256, n_frames, &A.bpf, blocks);
}

template <int L> static void up_launch(int wide, bool bilinear, unsigned blocks, const UpArgs& A, void* stream)
{
	auto k = wide ? (bilinear ? k_scale_up_wide<L, true> : k_scale_up_wide<L, false>) : (bilinear ? k_scale_up<L, true> : k_scale_up<L, false>);
	hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
}

extern "C" int agmv_hip_scale_frames_async(agmv_hip_ctx* c, int filter, const uint32_t* d_src, uint32_t src_w, uint32_t src_h, uint32_t n_frames, int fmt,
                                           uint32_t dst_w, uint32_t dst_h, void* d_dst, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const int yuv = yuv_base(fmt);
	if (!yuv && bad_pixfmt(fmt)) return -1;
	if (filter == 2) return agmv_hip_err("agmv_hip: the area filter is agmv_hip_scale_area_dev's, not agmv_hip_scale_frames_async's");
	if (filter != 1 && filter != 3) return agmv_hip_err("agmv_hip: unknown scale filter %d", filter);
	if (src_w == 0 || src_h == 0 || dst_w == 0 || dst_h == 0 || (unsigned long long)src_w * src_h > (1ull << 28) || (unsigned long long)dst_w * dst_h > (1ull << 28))
		return agmv_hip_err("agmv_hip: scaling frames of %u x %u to %u x %u (non-zero sizes of at most 2^28 pixels are needed)", src_w, src_h, dst_w, dst_h);
	if (!d_src || !d_dst) return agmv_hip_err("agmv_hip: NULL clip");
	if ((uintptr_t)d_src & 3 || (fmt == PF_XRGB32 && ((uintptr_t)d_dst & 3))) return agmv_hip_err("agmv_hip: an XRGB32 clip needs 4-byte alignment");
	if (n_frames == 0) return 0;
	UpArgs A;
	A.src = d_src; A.dst = (uint8_t*)d_dst; A.table = nullptr;
	A.frame_bytes = clip_frame_bytes(fmt, dst_w, dst_h);
	const int wide = yuv ? (dst_h & 1) == 0 && yuv_wide(fmt, d_dst, dst_w, dst_h, n_frames)
	                     : (dst_w & 15) == 0 && pf_aligned(fmt, d_dst, (size_t)dst_w * dst_h, n_frames);
	A.m = YUV_WR[(fmt >> 8) & 3];
	unsigned blocks;
	if (up_geometry(A, src_w, src_h, dst_w, dst_h, n_frames, wide, yuv, &blocks)) return -1;
	clip_dispatch<PF_BYTES | PF_YUV | PF_BIT(PF_XRGB32)>(fmt, [&](auto F) { up_launch<decltype(F)::value>(wide, filter == 3, blocks, A, stream); });
	CK(hipGetLastError());
	return 0;
}

// ---- normalised float tensor clips (AGMV_TENSORFMT of include/agmv.h): the table, the decoder's sink, the encoder's source ----
static int ten_elem_bytes(int type) { return type == TEN_F32 ? 4 : type == TEN_F16 || type == TEN_BF16 ? 2 : 0; }

extern "C" size_t agmv_hip_tensor_frame_bytes(int type, size_t n_pixels) { return 3 * (size_t)ten_elem_bytes(type) * n_pixels; }

// a float32's bit pattern rounded to nearest-even into binary16, overflow = infinity; integers only
static uint16_t ten_f16_bits(uint32_t u)
{
	const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
	if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);                      // NaN (no table entry is one)
	if (a >= 0x38800000u) {                                                     // 2^-14 and above: a normal binary16, or infinity
		const uint32_t r = a - 0x38000000u, h = (r + 0xFFFu + ((r >> 13) & 1u)) >> 13;
		return (uint16_t)(sign | (h < 0x7C00u ? h : 0x7C00u));
	}
	if (a < 0x33000000u) return (uint16_t)sign;                                 // below 2^-25: 0
	const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - (a >> 23);      // the value is m * 2^-24 >> shift, shift 14 .. 24
	const uint32_t h = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
	return (uint16_t)(sign | (h + (rem > half || (rem == half && (h & 1u)) ? 1u : 0u)));
}

static uint16_t ten_bf16_bits(uint32_t u) { return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }

extern "C" int agmv_hip_tensor_table(int type, const float mean[3], const float std[3], void* table)
{
	if (!ten_elem_bytes(type)) return agmv_hip_err("agmv_hip: unknown tensor type %d", type);
	if (!mean || !std || !table) return agmv_hip_err("agmv_hip: NULL normalisation or table");
	for (int c = 0; c < 3; c++) {                                               // (a NaN fails every comparison)
		const double m = mean[c] < 0 ? -(double)mean[c] : (double)mean[c], s = std[c] < 0 ? -(double)std[c] : (double)std[c];
		if (!(s >= 0x1p-32 && s <= 0x1p32 && m <= 0x1p32))
			return agmv_hip_err("agmv_hip: normalisation of channel %d outside the bounds (2^-32 <= |std| <= 2^32, |mean| <= 2^32)", c);
	}
	for (int c = 0; c < 3; c++)
		for (int v = 0; v < 256; v++) {
			const float f = (float)(((double)v / 255.0 - (double)mean[c]) / (double)std[c]);
			uint32_t u;
			memcpy(&u, &f, 4);
			if (type == TEN_F32) static_cast<uint32_t*>(table)[256 * c + v] = u;
			else static_cast<uint16_t*>(table)[256 * c + v] = type == TEN_F16 ? ten_f16_bits(u) : ten_bf16_bits(u);
		}
	return 0;
}

extern "C" int agmv_hip_tensor_from_xrgb_async(agmv_hip_ctx* c, int type, const uint32_t* d_src, uint32_t src_w, uint32_t src_h, uint32_t n_frames, int filter,
                                               uint32_t dst_w, uint32_t dst_h, const void* d_table, void* d_dst, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const int es = ten_elem_bytes(type);
	if (!es) return agmv_hip_err("agmv_hip: unknown tensor type %d", type);
	if (filter == 2) return agmv_hip_err("agmv_hip: the area filter is agmv_hip_scale_area_dev's, not agmv_hip_tensor_from_xrgb_async's");
	if (filter != 0 && filter != 1 && filter != 3) return agmv_hip_err("agmv_hip: unknown scale filter %d", filter);
	if (src_w == 0 || src_h == 0 || dst_w == 0 || dst_h == 0 || (unsigned long long)src_w * src_h > (1ull << 28) || (unsigned long long)dst_w * dst_h > (1ull << 28))
		return agmv_hip_err("agmv_hip: a tensor clip of %u x %u from frames of %u x %u (non-zero sizes of at most 2^28 pixels are needed)", dst_w, dst_h, src_w, src_h);
	if (filter == 0 && (src_w != dst_w || src_h != dst_h)) return agmv_hip_err("agmv_hip: filter 0 does not scale: %u x %u to %u x %u", src_w, src_h, dst_w, dst_h);
	if (!d_src || !d_table || !d_dst) return agmv_hip_err("agmv_hip: NULL clip or table");
	if ((uintptr_t)d_src & 3 || ((uintptr_t)d_table | (uintptr_t)d_dst) & (uintptr_t)(es - 1))
		return agmv_hip_err("agmv_hip: an XRGB32 clip needs 4-byte alignment, a tensor clip and its table that of their element");
	if (n_frames == 0) return 0;
	UpArgs A;
	A.src = d_src; A.dst = (uint8_t*)d_dst; A.table = d_table;
	A.frame_bytes = 3 * (size_t)es * dst_w * dst_h;
	A.m = YUV_WR[0];
	const int wide = (dst_w & 15) == 0 && ((uintptr_t)d_dst & 15) == 0;            // then every plane is a multiple of 32 bytes
	unsigned blocks;
	if (up_geometry(A, src_w, src_h, dst_w, dst_h, n_frames, wide, 0, &blocks)) return -1;
	if (es == 4) up_launch<PF_T32>(wide, filter == 3, blocks, A, stream);       // (filter 0 is the nearest scale to the same size: the identity)
	else up_launch<PF_T16>(wide, filter == 3, blocks, A, stream);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_tensor_to_xrgb_async(agmv_hip_ctx* c, int type, const void* d_src, size_t frame_pixels, uint32_t n_frames, const float* ab, uint32_t* d_dst,
                                             void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const int es = ten_elem_bytes(type);
	if (!es) return agmv_hip_err("agmv_hip: unknown tensor type %d", type);
	if (frame_pixels == 0 || frame_pixels > ((size_t)1 << 28)) return agmv_hip_err("agmv_hip: tensor frames of %zu pixels (1 .. 2^28 are needed)", frame_pixels);
	if (!d_src || !ab || !d_dst) return agmv_hip_err("agmv_hip: NULL clip or coefficients");
	if ((uintptr_t)d_src & (uintptr_t)(es - 1) || (uintptr_t)d_dst & 3) return agmv_hip_err("agmv_hip: a tensor clip needs the alignment of its element, an XRGB32 clip 4 bytes");
	if (n_frames == 0) return 0;
	uint32_t bpf; unsigned blocks;
	if (clip_grid((frame_pixels + 2047) / 2048, n_frames, &bpf, &blocks)) return -1;
	const int vec = (((uintptr_t)d_src | (uintptr_t)d_dst) & 15) == 0 && (frame_pixels * es & 15) == 0;
	ten_ab k;
	for (int i = 0; i < 3; i++) { k.a[i] = ab[i]; k.b[i] = ab[3 + i]; }
	auto kernel = type == TEN_F32 ? k_tensor_to_xrgb<TEN_F32> : type == TEN_F16 ? k_tensor_to_xrgb<TEN_F16> : k_tensor_to_xrgb<TEN_BF16>;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_src, frame_pixels, bpf, vec, k, d_dst);
	CK(hipGetLastError());
	return 0;
}

// ---- a decoded clip measured against its reference (AGMV_FRAME_QUALITY) ----
extern "C" int agmv_hip_measure_frames_async(agmv_hip_ctx* c, const uint32_t* d_test, int fmt, const void* d_ref, uint32_t w, uint32_t h, uint32_t n_frames,
                                             void* d_quality, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const int yuv = yuv_base(fmt);
	if (yuv ? bad_yuv(fmt, w, h) : bad_pixfmt(fmt)) return -1;
	if (w == 0 || h == 0 || (w & 3) || (h & 3) || (unsigned long long)w * h > (1ull << 28))
		return agmv_hip_err("agmv_hip: measuring frames of %u x %u (multiples of 4, at most 2^28 pixels, are needed)", w, h);
	if (n_frames == 0) return 0;
	if (!d_test || !d_ref || !d_quality) return agmv_hip_err("agmv_hip: NULL clip or result");
	if ((uintptr_t)d_test & 3 || (uintptr_t)d_quality & 7) return agmv_hip_err("agmv_hip: the test clip needs 4-byte, the result 8-byte alignment");
	CK(hipMemsetAsync(d_quality, 0, 96 * (size_t)n_frames, (hipStream_t)stream));
	MeasureArgs A;
	A.test = d_test; A.ref = (const uint8_t*)d_ref; A.out = (unsigned long long*)d_quality;
	A.frame_bytes = clip_frame_bytes(fmt, w, h);
	A.w = w; A.h = h; A.tx = (w / 4 + MS_TW - 1) / MS_TW; A.ty = (h / 4 + MS_TH - 1) / MS_TH;
	A.items = (unsigned long long)n_frames * A.tx * A.ty;
	A.t_vec = pf_aligned(PF_XRGB32, d_test, (size_t)w * h, n_frames);
	A.wide = yuv ? yuv_wide(fmt, d_ref, w, h, n_frames) : pf_aligned(fmt, d_ref, (size_t)w * h, n_frames);
	A.m = YUV_RD[(fmt >> 8) & 3];
	CLIP_LAUNCH(PF_BYTES | PF_YUV | PF_BIT(PF_XRGB32), k_measure, (unsigned)(A.items < 4096 ? A.items : 4096), A);
	CK(hipGetLastError());
	return 0;
}
