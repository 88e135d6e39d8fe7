// libagmv_amd/csrc/agmv_lz77_hip.hip -- the LZ77 stage of AGMV_EncodeFrame on the GPU (reference src/agmv_encode.c:179-238,
// csize :236), bit-exact, for a batch of pre-LZ bitstreams, and the "byte past the end" of the reference's one persistent
// bitstream buffer (:222, emulated on the host by prepare_batch in agmv_pipeline.c).
//
// Contract (the reference's AGMV_LZ77, restated): at token start i of an n-byte stream the match is the longest common
// prefix of d[j..] and d[i..], capped at min(255, n-i), over j in [max(0, i-65535), i); the earliest j wins among equals;
// one equal byte is a match.  A token is {dist lo, dist hi, len, d[i+len]} and advances by len + 1, or {0, 0, 0, d[i]}
// and advances by 1.  A match that ends exactly at n takes its fourth byte from behind the stream: d_peek[f] here.
// csize = 4 * tokens.
//
// Design: the greedy parse from a position p is a function of p and the frame's bytes alone, so
// two parses that reach the same position are identical from there on.
//   k_lz77_spec    one workgroup per segment of LZ77_SEG bytes parses greedily from the segment's first byte.  The
//                  window (<= 65535 bytes), the segment and 255 bytes of look-ahead sit in LDS; every token is one search
//                  of the whole workgroup over the window (4-byte test in registers, then extension; key = (length,
//                  earliest start); a full-cap match ends the search for every later start).  Recorded: one flag per
//                  byte (token start), the token at its start position, the exit of the segment.
//   k_lz77_stitch  one workgroup per frame walks the segments in order.  The entry of a segment is the exit of the one
//                  before; if it is a recorded start the recorded tokens from there on are the true ones, else the
//                  workgroup parses from the entry until it meets a recorded start or leaves the segment.
//   k_lz77_count / k_lz77_scan / k_lz77_emit  count the live tokens per segment, prefix sums per frame, copy the tokens.
// Exactness never rests on the speculation: a token is live only if the true chain from position 0 reaches it.
// No workgroup waits for another inside a kernel, and every loop is bounded by the segment or frame length.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "agmv_hip_impl.h"

constexpr uint32_t LZ77_WIN = 65535;             // matches start in [i - 65535, i)
constexpr uint32_t LZ77_MAXLEN = 255;
constexpr uint32_t LZ77_SEG = 4096;              // bytes per speculative segment
constexpr uint32_t LZ77_T = 512;                 // lanes of a searching workgroup
constexpr uint32_t LZ77_LDS = 65536 + 4 + LZ77_SEG + 256 + 12;   // window + alignment + segment + look-ahead: 2 workgroups per CU
constexpr uint32_t LZ77_MAXN = 1u << 24;         // frame sizes are below this (csize = 4 * tokens stays exact in float)
constexpr uint32_t LZ77_CHUNK = 1u << 26;        // positions per chunk of frames (5 bytes of work area each)
constexpr uint32_t LZ77_CHUNK_FRAMES = 1u << 16;
constexpr uint32_t F_SPEC = 1, F_TRUE = 2;       // flags of a byte: token start of the speculative parse / of a re-parse

// last k in [0, n) with tab[k] <= x (tab ascending, tab[0] <= x); bounded by 32 halvings
__device__ __forceinline__ uint32_t lz77_upper_idx(const uint32_t* __restrict__ tab, uint32_t n, uint32_t x)
{
	uint32_t lo = 0, hi = n - 1;
	for (int it = 0; it < 32 && lo < hi; it++) {
		const uint32_t mid = (lo + hi + 1) >> 1;
		if (tab[mid] <= x) lo = mid; else hi = mid - 1;
	}
	return lo;
}

struct lz77_seg { uint32_t k, n, base, S, E; };

// segment g of the chunk: its frame k, the frame's size and first position in the work areas, its bytes [S, E)
__device__ __forceinline__ lz77_seg lz77_seg_of(uint32_t g, const uint32_t* __restrict__ fstart, const uint32_t* __restrict__ sb, uint32_t nf)
{
	lz77_seg s;
	s.k = lz77_upper_idx(sb, nf + 1, g);         // sb[k] <= g < sb[k+1] (frames without segments are skipped)
	s.base = fstart[s.k];
	s.n = fstart[s.k + 1] - s.base;
	s.S = (g - sb[s.k]) * LZ77_SEG;
	s.E = min(s.S + LZ77_SEG, s.n);
	return s;
}

// bytes [p0, p1) of a row into LDS: byte p sits at l8[p - p0 + a], a = (address of row + p0) & 3, so that the body moves
// as aligned dwords; nothing outside [p0, p1) is read
__device__ __forceinline__ void lz77_stage(uint8_t* l8, const uint8_t* __restrict__ row, uint32_t p0, uint32_t p1, uint32_t a)
{
	const uint8_t* g = row + p0;
	const uint32_t len = p1 - p0, head = min(len, (4u - a) & 3u), nb = (len - head) >> 2, tail = (len - head) & 3u;
	if (threadIdx.x < head) l8[a + threadIdx.x] = g[threadIdx.x];
	const uint32_t* g4 = (const uint32_t*)(g + head);
	uint32_t* l4 = (uint32_t*)(l8 + a + head);
	for (uint32_t t = threadIdx.x; t < nb; t += LZ77_T) l4[t] = g4[t];
	if (threadIdx.x < tail) l8[a + head + 4 * nb + threadIdx.x] = g[head + 4 * nb + threadIdx.x];
}

struct lz77_sh {
	unsigned long long red[LZ77_T / 64];
	uint32_t full;                               // the earliest start so far with a match of the full cap
};

// the 4 bytes at LDS byte address x, which need not be aligned (two dword reads and a byte funnel shift)
__device__ __forceinline__ uint32_t lz77_ld4(const uint32_t* l4, uint32_t x)
{
	return __builtin_amdgcn_alignbyte(l4[(x >> 2) + 1], l4[x >> 2], x & 3u);
}

// the longest, then the earliest, of the lanes' matches (length << 32 | ~start, 0 = none), uniform; `full` is reset
__device__ __forceinline__ unsigned long long lz77_reduce(unsigned long long key, lz77_sh* sh)
{
	for (int o = 32; o >= 1; o >>= 1) {
		const unsigned long long other = __shfl_xor(key, o);
		key = other > key ? other : key;
	}
	if ((threadIdx.x & 63u) == 0) sh->red[threadIdx.x >> 6] = key;
	__syncthreads();
	key = sh->red[0];
	for (uint32_t wv = 1; wv < LZ77_T / 64; wv++) key = sh->red[wv] > key ? sh->red[wv] : key;
	if (threadIdx.x == 0) sh->full = 0xFFFFFFFFu;
	__syncthreads();
	return key;
}

// 0x80 in every byte of x that is zero
__device__ __forceinline__ uint32_t lz77_zero_bytes(uint32_t x)
{
	return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// The match of the token at LDS byte c1 over the candidate starts [c0, c1), cap >= 1 bytes long at most: (length << 32 |
// ~start), 0 length = none.  Called by the whole workgroup, the result is uniform.  Lane t tests the dwords t, t + T, ...
// of the window (consecutive lanes, consecutive banks), oldest first, so inside a lane a strictly longer match is the
// earliest of its length; the reduction takes the longest, then the earliest.  A match of the full cap cannot be beaten
// by a later start: such a lane stops and publishes its start, and lanes whose dwords lie behind it stop too.
//   pass A (cap > 3): matches of 4 bytes and more.  The first 4 bytes of the 4 candidates of a dword are compared in
//     registers (the dword, its successor, a byte funnel shift): about a dozen instructions per dword when nothing matches.
//     A candidate that matches is extended, once the lane holds a match only if it also agrees at offset `best`.
//   pass B (nothing found in pass A): matches of 1..3 bytes, found with zero-byte masks alone.
__device__ __forceinline__ unsigned long long lz77_search(const uint8_t* l8, uint32_t c0, uint32_t c1, uint32_t cap, lz77_sh* sh)
{
	const uint32_t* l4 = (const uint32_t*)l8;
	const uint32_t t4 = lz77_ld4(l4, c1), d0 = c0 >> 2, dend = (c1 + 3) >> 2;
	if (cap > 3) {
		uint32_t best = 0, bs = 0;
		bool done = false;
		for (uint32_t d = d0 + threadIdx.x; d < dend && !done; d += LZ77_T) {
			const uint32_t full = __hip_atomic_load(&sh->full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			const uint32_t w0 = l4[d], w1 = l4[d + 1];                              // (issued together with the read of `full`)
			if ((d << 2) > full) break;
			uint32_t hit = (w0 == t4 ? 1u : 0u) | (__builtin_amdgcn_alignbyte(w1, w0, 1) == t4 ? 2u : 0u) |
			               (__builtin_amdgcn_alignbyte(w1, w0, 2) == t4 ? 4u : 0u) | (__builtin_amdgcn_alignbyte(w1, w0, 3) == t4 ? 8u : 0u);
			while (hit) {
				const uint32_t c = (d << 2) + (uint32_t)(__ffs((int)hit) - 1);
				hit &= hit - 1;
				if (c < c0 || c >= c1) continue;
				if (best && l8[c + best] != l8[c1 + best]) continue;                // cannot be longer than best (best < cap here)
				uint32_t p = 4;
				while (p < cap) {
					const uint32_t y = lz77_ld4(l4, c + p) ^ lz77_ld4(l4, c1 + p);
					if (y) { p += (uint32_t)(__ffs((int)y) - 1) >> 3; break; }
					p += 4;
				}
				p = min(p, cap);
				if (p <= best) continue;
				best = p; bs = c;
				if (p == cap) { atomicMin(&sh->full, c); done = true; break; }
			}
		}
		const unsigned long long key = lz77_reduce(best ? ((unsigned long long)best << 32 | (uint32_t)~bs) : 0ull, sh);
		if (key) return key;
		cap = 3;
	}
	const uint32_t pat0 = (t4 & 255u) * 0x01010101u, pat1 = (t4 >> 8 & 255u) * 0x01010101u, pat2 = (t4 >> 16 & 255u) * 0x01010101u;
	uint32_t best = 0, bs = 0;
	for (uint32_t d = d0 + threadIdx.x; d < dend; d += LZ77_T) {
		const uint32_t full = __hip_atomic_load(&sh->full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		const uint32_t w0 = l4[d], w1 = l4[d + 1];
		if ((d << 2) > full) break;
		uint32_t m1 = lz77_zero_bytes(w0 ^ pat0);                                   // byte k: candidate 4d + k agrees in its first byte
		if (d == d0) m1 &= 0x80808080u << 8 * (c0 & 3u);                            // candidates before c0
		if (d == dend - 1 && (c1 & 3u)) m1 &= 0x80808080u >> 8 * (4u - (c1 & 3u));  // candidates at and behind c1
		if (!m1) continue;
		const uint32_t m2 = cap > 1 ? m1 & lz77_zero_bytes(__builtin_amdgcn_alignbyte(w1, w0, 1) ^ pat1) : 0u;
		const uint32_t m3 = cap > 2 ? m2 & lz77_zero_bytes(__builtin_amdgcn_alignbyte(w1, w0, 2) ^ pat2) : 0u;
		const uint32_t len = m3 ? 3u : m2 ? 2u : 1u, m = m3 ? m3 : m2 ? m2 : m1;
		if (len <= best) continue;
		best = len; bs = (d << 2) + ((uint32_t)(__ffs((int)m) - 1) >> 3);
		if (len == cap) { atomicMin(&sh->full, bs); break; }
	}
	return lz77_reduce(best ? ((unsigned long long)best << 32 | (uint32_t)~bs) : 0ull, sh);
}

// one token at position i of a frame whose bytes [W0, ..) are staged with offset a: search, record, the next position
__device__ __forceinline__ uint32_t lz77_token(const uint8_t* l8, uint32_t W0, uint32_t a, uint32_t i, uint32_t n, lz77_sh* sh,
                                               uint32_t* __restrict__ tokv, uint8_t* __restrict__ flag, uint32_t base, uint32_t mark)
{
	const uint32_t cap = min(LZ77_MAXLEN, n - i), lo = i > LZ77_WIN ? i - LZ77_WIN : 0u, c1 = i - W0 + a;
	const unsigned long long key = lz77_search(l8, lo - W0 + a, c1, cap, sh);
	const uint32_t len = (uint32_t)(key >> 32);
	if (threadIdx.x == 0) {
		const uint32_t dist = len ? c1 - ~(uint32_t)key : 0u;
		const uint32_t next = i + len < n ? l8[c1 + len] : 0u;                      // at n: the peek byte, put in by k_lz77_emit
		tokv[base + i] = dist | len << 16 | next << 24;
		flag[base + i] = (uint8_t)mark;
	}
	return i + (len ? len + 1 : 1);
}

__global__ void __launch_bounds__(LZ77_T) k_lz77_spec(const uint8_t* __restrict__ bits, unsigned long long stride,
                                                      const uint32_t* __restrict__ fstart, const uint32_t* __restrict__ sb,
                                                      uint32_t f0, uint32_t nf, uint32_t* __restrict__ tokv, uint8_t* __restrict__ flag,
                                                      uint32_t* __restrict__ sexit, uint32_t* __restrict__ smerge)
{
	__shared__ uint32_t lds[LZ77_LDS / 4];
	__shared__ lz77_sh sh;
	uint8_t* l8 = (uint8_t*)lds;
	const lz77_seg s = lz77_seg_of(blockIdx.x, fstart, sb, nf);
	const uint8_t* row = bits + (unsigned long long)(f0 + s.k) * stride;
	const uint32_t W0 = s.S > LZ77_WIN ? s.S - LZ77_WIN : 0u, p1 = min(s.n, s.E + LZ77_MAXLEN);
	const uint32_t a = (uint32_t)((uintptr_t)(row + W0) & 3u);
	for (uint32_t t = s.S + threadIdx.x; t < s.E; t += LZ77_T) flag[s.base + t] = 0;
	lz77_stage(l8, row, W0, p1, a);
	if (threadIdx.x == 0) { sh.full = 0xFFFFFFFFu; smerge[blockIdx.x] = 0xFFFFFFFFu; }
	__syncthreads();
	uint32_t i = s.S;
	for (uint32_t it = 0; it < LZ77_SEG && i < s.E; it++) i = lz77_token(l8, W0, a, i, s.n, &sh, tokv, flag, s.base, F_SPEC);
	if (threadIdx.x == 0) sexit[blockIdx.x] = i;
}

// smerge[g]: the recorded starts of segment g at or behind it are live (0xFFFFFFFF: none); re-parsed tokens carry F_TRUE
__global__ void __launch_bounds__(LZ77_T) k_lz77_stitch(const uint8_t* __restrict__ bits, unsigned long long stride,
                                                        const uint32_t* __restrict__ fstart, const uint32_t* __restrict__ sb,
                                                        uint32_t f0, uint32_t* __restrict__ tokv, uint8_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ sexit, uint32_t* __restrict__ smerge,
                                                        uint32_t* __restrict__ reparsed)
{
	__shared__ uint32_t lds[LZ77_LDS / 4];
	__shared__ lz77_sh sh;
	uint8_t* l8 = (uint8_t*)lds;
	const uint32_t k = blockIdx.x, base = fstart[k], n = fstart[k + 1] - base, nseg = sb[k + 1] - sb[k];
	const uint8_t* row = bits + (unsigned long long)(f0 + k) * stride;
	if (threadIdx.x == 0) sh.full = 0xFFFFFFFFu;
	uint32_t e = 0;
	for (uint32_t it = 0; it < nseg && e < n; it++) {
		const uint32_t sl = e / LZ77_SEG, g = sb[k] + sl, S = sl * LZ77_SEG, E = min(S + LZ77_SEG, n);
		if (flag[base + e] & F_SPEC) {
			if (threadIdx.x == 0) smerge[g] = e;
			e = sexit[g];
			continue;
		}
		const uint32_t W0 = S > LZ77_WIN ? S - LZ77_WIN : 0u, p1 = min(n, E + LZ77_MAXLEN);
		const uint32_t a = (uint32_t)((uintptr_t)(row + W0) & 3u);
		if (threadIdx.x == 0) atomicAdd(reparsed, 1u);
		__syncthreads();
		lz77_stage(l8, row, W0, p1, a);
		__syncthreads();
		uint32_t i = e;
		bool merged = false;
		for (uint32_t jt = 0; jt < LZ77_SEG && i < E; jt++) {
			if (flag[base + i] & F_SPEC) { merged = true; break; }
			i = lz77_token(l8, W0, a, i, n, &sh, tokv, flag, base, F_TRUE);
		}
		if (merged) {
			if (threadIdx.x == 0) smerge[g] = i;
			e = sexit[g];
		} else e = i;
	}
}

__device__ __forceinline__ bool lz77_live(uint32_t fl, uint32_t pos, uint32_t merge)
{
	return (fl & F_TRUE) || ((fl & F_SPEC) && pos >= merge);
}

__device__ __forceinline__ uint32_t lz77_block_excl_scan_256(uint32_t v, uint32_t* sh, uint32_t* total)
{
	const uint32_t t = threadIdx.x;
	sh[t] = v;
	__syncthreads();
	for (uint32_t o = 1; o < 256; o <<= 1) {
		const uint32_t x = t >= o ? sh[t - o] : 0u;
		__syncthreads();
		sh[t] += x;
		__syncthreads();
	}
	const uint32_t incl = sh[t];
	*total = sh[255];
	__syncthreads();
	return incl - v;
}

constexpr uint32_t LZ77_PER = LZ77_SEG / 256;    // positions per lane in count and emit

__global__ void __launch_bounds__(256) k_lz77_count(const uint32_t* __restrict__ fstart, const uint32_t* __restrict__ sb, uint32_t nf,
                                                    const uint8_t* __restrict__ flag, const uint32_t* __restrict__ smerge,
                                                    uint32_t* __restrict__ scnt)
{
	__shared__ uint32_t shs[256];
	const lz77_seg s = lz77_seg_of(blockIdx.x, fstart, sb, nf);
	const uint32_t merge = smerge[blockIdx.x];
	uint32_t c = 0;
	for (uint32_t j = 0; j < LZ77_PER; j++) {
		const uint32_t p = s.S + threadIdx.x * LZ77_PER + j;
		if (p < s.E && lz77_live(flag[s.base + p], p, merge)) c++;
	}
	uint32_t tot;
	lz77_block_excl_scan_256(c, shs, &tot);
	if (threadIdx.x == 0) scnt[blockIdx.x] = tot;
}

// one workgroup per frame: exclusive sums of its segments' counts, csize
__global__ void __launch_bounds__(256) k_lz77_scan(const uint32_t* __restrict__ sb, uint32_t f0, uint32_t* __restrict__ scnt,
                                                   uint32_t* __restrict__ csize)
{
	__shared__ uint32_t shs[256];
	const uint32_t k = blockIdx.x, g0 = sb[k], g1 = sb[k + 1];
	uint32_t carry = 0;
	for (uint32_t b = g0; b < g1; b += 256) {                       // <= 2^24 / LZ77_SEG / 256 = 16 rounds
		const uint32_t g = b + threadIdx.x;
		const uint32_t v = g < g1 ? scnt[g] : 0u;
		uint32_t tot;
		const uint32_t ex = lz77_block_excl_scan_256(v, shs, &tot);
		if (g < g1) scnt[g] = carry + ex;
		carry += tot;
	}
	if (threadIdx.x == 0) csize[f0 + k] = 4u * carry;
}

__global__ void __launch_bounds__(256) k_lz77_emit(const uint32_t* __restrict__ fstart, const uint32_t* __restrict__ sb, uint32_t f0,
                                                   uint32_t nf, const uint32_t* __restrict__ tokv, const uint8_t* __restrict__ flag,
                                                   const uint32_t* __restrict__ smerge, const uint32_t* __restrict__ soff,
                                                   const uint8_t* __restrict__ peek, uint8_t* __restrict__ out, unsigned long long out_stride)
{
	__shared__ uint32_t shs[256];
	const lz77_seg s = lz77_seg_of(blockIdx.x, fstart, sb, nf);
	const uint32_t merge = smerge[blockIdx.x];
	uint32_t c = 0, live = 0;
	for (uint32_t j = 0; j < LZ77_PER; j++) {
		const uint32_t p = s.S + threadIdx.x * LZ77_PER + j;
		if (p < s.E && lz77_live(flag[s.base + p], p, merge)) { c++; live |= 1u << j; }
	}
	uint32_t tot;
	uint32_t at = soff[blockIdx.x] + lz77_block_excl_scan_256(c, shs, &tot);
	uint8_t* dst = out + (unsigned long long)(f0 + s.k) * out_stride;
	for (uint32_t j = 0; j < LZ77_PER; j++) {
		if (!(live >> j & 1u)) continue;
		const uint32_t p = s.S + threadIdx.x * LZ77_PER + j;
		uint32_t t = tokv[s.base + p];
		const uint32_t len = t >> 16 & 255u;
		if (len && p + len == s.n) t = (t & 0x00FFFFFFu) | (peek ? (uint32_t)peek[f0 + s.k] << 24 : 0u);
		uint8_t* o = dst + 4ull * at++;
		o[0] = (uint8_t)t; o[1] = (uint8_t)(t >> 8); o[2] = (uint8_t)(t >> 16); o[3] = (uint8_t)(t >> 24);
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// the byte past the end (prepare_batch of agmv_pipeline.c, position-parallel).  In frame order the host does
//   peek[f] = n_f < persist_len ? persist[n_f] : 0;  persist[0, min(n_f, persist_len)) = row f
// so peek[f] is byte n_f of the last earlier frame that is longer than n_f, else the buffer's own byte; and the buffer
// ends with byte q of the last frame that is longer than q.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lz77_peek(const uint8_t* __restrict__ bits, unsigned long long stride,
                                                   const uint32_t* __restrict__ sizes, uint32_t nf, const uint8_t* __restrict__ persist,
                                                   unsigned long long persist_len, uint8_t* __restrict__ peek)
{
	const uint32_t f = blockIdx.x * 256u + threadIdx.x;
	if (f >= nf) return;
	const uint32_t q = sizes[f];
	uint8_t v = 0;
	if (q < persist_len) {
		v = persist[q];
		for (uint32_t g = f; g-- > 0;)                               // bounded by the frames of the call
			if (sizes[g] > q) { v = bits[(unsigned long long)g * stride + q]; break; }
	}
	peek[f] = v;
}

// sm[g] = max(sizes[g..nf)): one workgroup, strips of frames
__global__ void __launch_bounds__(1024) k_lz77_sufmax(const uint32_t* __restrict__ sizes, uint32_t nf, uint32_t* __restrict__ sm)
{
	__shared__ uint32_t part[1024];
	const uint32_t per = (nf + 1023u) / 1024u, a = min(nf, threadIdx.x * per), b = min(nf, a + per);
	uint32_t m = 0;
	for (uint32_t g = a; g < b; g++) m = max(m, sizes[g]);
	part[threadIdx.x] = m;
	__syncthreads();
	uint32_t run = 0;
	for (uint32_t t = threadIdx.x + 1; t < 1024; t++) run = max(run, part[t]);       // the strips behind this one
	for (uint32_t g = b; g-- > a;) { run = max(run, sizes[g]); sm[g] = run; }
}

__global__ void __launch_bounds__(256) k_lz77_persist(const uint8_t* __restrict__ bits, unsigned long long stride, uint32_t nf,
                                                      const uint32_t* __restrict__ sm, uint8_t* __restrict__ persist,
                                                      unsigned long long persist_len)
{
	const unsigned long long lim = persist_len < sm[0] ? persist_len : sm[0];
	for (unsigned long long q = blockIdx.x * 256ull + threadIdx.x; q < lim; q += gridDim.x * 256ull) {
		uint32_t lo = 0, hi = nf - 1;                                // the last g with sm[g] > q (sm descends, sm[0] > q)
		for (int it = 0; it < 32 && lo < hi; it++) {
			const uint32_t mid = (lo + hi + 1) >> 1;
			if (sm[mid] > q) lo = mid; else hi = mid - 1;
		}
		persist[q] = bits[(unsigned long long)lo * stride + q];
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// work areas (per context, grown on demand)
// ---------------------------------------------------------------------------------------------------------------------
struct lz77_ws {
	size_t cap_n;               // positions of a chunk
	uint32_t* tokv;
	uint8_t* flag;
	size_t cap_seg;
	uint32_t *sexit, *smerge, *scnt;
	size_t cap_tab;             // u32 entries of the chunk tables
	uint32_t* tab;
	size_t cap_sm;
	uint32_t* sm;
	uint32_t* reparsed;
};

static void lz77_free(void* p)
{
	lz77_ws* w = (lz77_ws*)p;
	void* all[] = {w->tokv, w->flag, w->sexit, w->smerge, w->scnt, w->tab, w->sm, w->reparsed};
	for (void* a : all) if (a) (void)hipFree(a);
	free(w);
}

static int lz77_get_ws(agmv_hip_ctx* c, lz77_ws** out)
{
	lz77_ws* w = (lz77_ws*)agmv_hip_area(c, AREA_LZ77, sizeof(lz77_ws), lz77_free);
	if (!w) return -1;
	if (!w->reparsed) {
		CK(hipMalloc((void**)&w->reparsed, 4));
		CK(hipMemset(w->reparsed, 0, 4));
	}
	*out = w;
	return 0;
}

static int lz77_grow(lz77_ws* w, size_t n, size_t nseg, size_t ntab)
{
	if (n > w->cap_n) {                                            // a shared capacity is committed when all its buffers exist
		w->cap_n = 0;
		CK(agmv_hip_dev_grow(&w->tokv, nullptr, n));
		CK(agmv_hip_dev_grow(&w->flag, nullptr, n));
		w->cap_n = n;
	}
	if (nseg > w->cap_seg) {
		w->cap_seg = 0;
		for (uint32_t** b : {&w->sexit, &w->smerge, &w->scnt}) CK(agmv_hip_dev_grow(b, nullptr, nseg));
		w->cap_seg = nseg;
	}
	CK(agmv_hip_dev_grow(&w->tab, &w->cap_tab, ntab));
	return 0;
}

extern "C" size_t agmv_hip_lz77_max_csize(size_t n)
{
	return 4 * n;                   // every byte a token
}

extern "C" int agmv_hip_lz77_peek_dev(agmv_hip_ctx* c, const uint8_t* d_bits, size_t bits_stride, const uint32_t* d_sizes,
                                      uint32_t n_frames, uint8_t* d_persist, size_t persist_len, uint8_t* d_peek, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0) return 0;
	hipStream_t s = (hipStream_t)stream;
	lz77_ws* w;
	if (lz77_get_ws(c, &w)) return -1;
	CK(agmv_hip_dev_grow(&w->sm, &w->cap_sm, n_frames));
	hipLaunchKernelGGL(k_lz77_peek, dim3((n_frames + 255) / 256), dim3(256), 0, s, d_bits, (unsigned long long)bits_stride, d_sizes,
	                   n_frames, d_persist, (unsigned long long)persist_len, d_peek);
	CK(hipGetLastError());
	if (persist_len) {
		const size_t top = persist_len < bits_stride ? persist_len : bits_stride;
		const uint32_t gx = (uint32_t)((top + 255) / 256 < 4096 ? (top + 255) / 256 : 4096);
		hipLaunchKernelGGL(k_lz77_sufmax, dim3(1), dim3(1024), 0, s, d_sizes, n_frames, w->sm);
		hipLaunchKernelGGL(k_lz77_persist, dim3(gx < 1 ? 1 : gx), dim3(256), 0, s, d_bits, (unsigned long long)bits_stride, n_frames,
		                   w->sm, d_persist, (unsigned long long)persist_len);
		CK(hipGetLastError());
	}
	return 0;
}

extern "C" int agmv_hip_lz77_frames_dev(agmv_hip_ctx* c, const uint8_t* d_bits, size_t bits_stride, const uint32_t* d_sizes,
                                        uint32_t n_frames, const uint8_t* d_peek, uint8_t* d_out, size_t out_stride,
                                        uint32_t* d_csize, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0) return 0;
	hipStream_t s = (hipStream_t)stream;
	lz77_ws* w;
	if (lz77_get_ws(c, &w)) return -1;

	// the sizes decide the chunks: read them once
	std::vector<uint32_t> sz(n_frames);
	CK(hipMemcpyAsync(sz.data(), d_sizes, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s));
	CK(hipStreamSynchronize(s));
	for (uint32_t f = 0; f < n_frames; f++) {
		if (sz[f] > bits_stride || sz[f] >= LZ77_MAXN || agmv_hip_lz77_max_csize(sz[f]) > out_stride)
			return agmv_hip_err("agmv_hip_lz77_frames_dev: frame %u: %u bytes (bits_stride %zu, out_stride %zu, at most %u bytes per frame)",
			                    f, sz[f], bits_stride, out_stride, LZ77_MAXN - 1);
	}
	// chunks: [f0, f0 + nf) with <= LZ77_CHUNK positions; per chunk the tables fstart[nf + 1] (positions), sb[nf + 1] (first segment)
	struct chunk { uint32_t f0, nf, n, nseg; size_t tab; };
	std::vector<chunk> ch;
	std::vector<uint32_t> tab;
	size_t maxn = 1, maxs = 1;
	for (uint32_t f = 0; f < n_frames;) {
		chunk k = {f, 0, 0, 0, tab.size()};
		while (f < n_frames && k.nf < LZ77_CHUNK_FRAMES && (uint64_t)k.n + sz[f] <= LZ77_CHUNK) { k.n += sz[f]; k.nf++; f++; }
		const size_t t0 = tab.size();
		tab.resize(t0 + 2 * (size_t)(k.nf + 1));
		uint32_t* fs = &tab[t0]; uint32_t* sb = fs + k.nf + 1;
		uint32_t at = 0, sc = 0;
		for (uint32_t j = 0; j < k.nf; j++) {
			fs[j] = at; sb[j] = sc;
			at += sz[k.f0 + j]; sc += (sz[k.f0 + j] + LZ77_SEG - 1) / LZ77_SEG;
		}
		fs[k.nf] = at; sb[k.nf] = sc;
		k.nseg = sc;
		if (k.n > maxn) maxn = k.n;
		if (sc > maxs) maxs = sc;
		ch.push_back(k);
	}
	if (lz77_grow(w, maxn, maxs, tab.size())) return -1;
	CK(hipMemcpyAsync(w->tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
	CK(hipMemsetAsync(w->reparsed, 0, 4, s));
	CK(hipStreamSynchronize(s));                                   // (tab is host memory of this call)

	for (const chunk& k : ch) {
		const uint32_t* fs = w->tab + k.tab;
		const uint32_t* sb = fs + k.nf + 1;
		if (k.nseg) {
			hipLaunchKernelGGL(k_lz77_spec, dim3(k.nseg), dim3(LZ77_T), 0, s, d_bits, (unsigned long long)bits_stride, fs, sb, k.f0, k.nf,
			                   w->tokv, w->flag, w->sexit, w->smerge);
			hipLaunchKernelGGL(k_lz77_stitch, dim3(k.nf), dim3(LZ77_T), 0, s, d_bits, (unsigned long long)bits_stride, fs, sb, k.f0,
			                   w->tokv, w->flag, w->sexit, w->smerge, w->reparsed);
			hipLaunchKernelGGL(k_lz77_count, dim3(k.nseg), dim3(256), 0, s, fs, sb, k.nf, w->flag, w->smerge, w->scnt);
			CK(hipGetLastError());
		}
		hipLaunchKernelGGL(k_lz77_scan, dim3(k.nf), dim3(256), 0, s, sb, k.f0, w->scnt, d_csize);
		if (k.nseg)
			hipLaunchKernelGGL(k_lz77_emit, dim3(k.nseg), dim3(256), 0, s, fs, sb, k.f0, k.nf, w->tokv, w->flag, w->smerge, w->scnt,
			                   d_peek, d_out, (unsigned long long)out_stride);
		CK(hipGetLastError());
	}
	return 0;
}

extern "C" int agmv_hip_lz77_reparsed_segments(agmv_hip_ctx* c, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const lz77_ws* w = (const lz77_ws*)c->ws[AREA_LZ77];
	if (!w || !w->reparsed) return 0;
	uint32_t v = 0;
	CK(hipStreamSynchronize((hipStream_t)stream));
	CK(hipMemcpy(&v, w->reparsed, 4, hipMemcpyDeviceToHost));
	return (int)v;
}

extern "C" int agmv_hip_lz77_frames(agmv_hip_ctx* c, const uint8_t* h_bits, size_t bits_stride, const uint32_t* h_sizes,
                                    uint32_t n_frames, uint8_t* h_persist, size_t persist_len, uint8_t* h_out, size_t out_stride,
                                    uint32_t* h_csize)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0) return 0;
	uint8_t *db = nullptr, *dout = nullptr, *dp = nullptr, *dpeek = nullptr;
	uint32_t *ds = nullptr, *dc = nullptr;
	int rc = -1;
	hipError_t e;
	if ((e = hipMalloc((void**)&db, (size_t)n_frames * bits_stride + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&dout, (size_t)n_frames * out_stride + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&dp, persist_len + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&dpeek, n_frames)) != hipSuccess ||
	    (e = hipMalloc((void**)&ds, (size_t)n_frames * 4)) != hipSuccess ||
	    (e = hipMalloc((void**)&dc, (size_t)n_frames * 4)) != hipSuccess ||
	    (e = hipMemcpy(db, h_bits, (size_t)n_frames * bits_stride, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = hipMemcpy(ds, h_sizes, (size_t)n_frames * 4, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = h_persist ? hipMemcpy(dp, h_persist, persist_len, hipMemcpyHostToDevice) : hipMemset(dp, 0, persist_len + 1)) != hipSuccess) {
		agmv_hip_hip_failed("agmv_hip_lz77_frames", e, __FILE_NAME__, __LINE__);
		goto done;
	}
	if (agmv_hip_lz77_peek_dev(c, db, bits_stride, ds, n_frames, dp, persist_len, dpeek, nullptr)) goto done;
	if (agmv_hip_lz77_frames_dev(c, db, bits_stride, ds, n_frames, dpeek, dout, out_stride, dc, nullptr)) goto done;
	if ((e = hipDeviceSynchronize()) != hipSuccess ||
	    (e = hipMemcpy(h_csize, dc, (size_t)n_frames * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
	    (e = h_persist && persist_len ? hipMemcpy(h_persist, dp, persist_len, hipMemcpyDeviceToHost) : hipSuccess) != hipSuccess) {
		agmv_hip_hip_failed("agmv_hip_lz77_frames", e, __FILE_NAME__, __LINE__);
		goto done;
	}
	for (uint32_t f = 0; f < n_frames; f++)                        // rows: only the payload bytes are defined
		if (h_csize[f] && (e = hipMemcpy(h_out + (size_t)f * out_stride, dout + (size_t)f * out_stride, h_csize[f], hipMemcpyDeviceToHost)) != hipSuccess) {
			agmv_hip_hip_failed("agmv_hip_lz77_frames", e, __FILE_NAME__, __LINE__);
			goto done;
		}
	rc = 0;
done:
	(void)hipFree(db); (void)hipFree(dout); (void)hipFree(dp); (void)hipFree(dpeek); (void)hipFree(ds); (void)hipFree(dc);
	return rc;
}
