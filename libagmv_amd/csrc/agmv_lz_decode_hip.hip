// libagmv_amd/csrc/agmv_lz_decode_hip.hip -- the LZ stage of AGMV_DecodeFrameChunk on the GPU (reference src/agmv_decode.c:160-222,
// bit reader src/agmv_utils.c:32-57), bit-exact with agmv_lz_decode_mem (agmv_lz.c), for a batch of frame payloads; and the
// reference's single persistent decompression buffer applied to a batch in frame order.
//
// Contract (agmv_lz_decode_mem, restated; data = the frame's output row, lim = cap - 16):
//   payload: avail[f] bytes exist; a read at an index >= avail returns 0 and is not counted.  The reader never fetches
//     more than csize + 3 bytes, so a row needs only R = min(avail, csize + 3) readable bytes: nothing here reads past R.
//   LZSS (version 1, 2): LSB-first tokens while bits < 8 csize, bpos < usize and bpos < lim.  Flag 1: literal, 8 bits.
//     Flag 0: 16-bit offset, 4-bit len; byte k < len copies src = pos - offset + k (pos = bpos at the token, unsigned
//     wrap-around) when src < bpos and bpos < lim.
//   LZ77 (any other version): 4-byte tokens {u16 offset, u8 len, u8 byte} for t < csize in steps of 4 (64-bit t), the
//     copies as for LZSS, then data[bpos++] = byte while bpos < lim.
//   used = bytes the reader fetched, capped at avail.
//
// Design ("The LZ stage of the decoder"):
//   every token has a nominal output length: a literal 1; a match len when 1 <= offset <= pos, 0 when offset = 0; an
//   LZ77 token one more for its byte.  A match with offset > pos copies, in closed form, max(0, len - (offset - pos))
//   bytes (none at pos = 0) from position 0 onward: it is a match of offset pos.  Up to and including the first such
//   match the nominal positions are the true ones; a frame in which a further token follows it is left to a serial
//   kernel (only damaged or crafted streams do that -- encoder output can end with one, when its last token reads guard
//   bits).
//   token starts: LZSS tokens are 9 or 21 bits, so a piece of LZD_PB bits is entered at one of 21 offsets.  k_lzd_spiece
//     walks every piece from all 21 (the piece's bytes staged in LDS), k_lzd_chain (one lane per frame) chains them and
//     finds the pieces the stream reaches, k_lzd_semit re-walks each live piece from its true entry.  LZ77 tokens sit at
//     4t: pieces of LZD_PT tokens, one entry (k_lzd_tpiece, k_lzd_temit).
//   bytes: the emit kernels write one word per output position into a word area: a literal byte, resolved (bit 31), or the
//     position it copies (always lower, same frame).  Pointer jumping (k_lzd_jump: word[p] = word[word[p]]) resolves the
//     chains in at most ceil(log2(frame length)) + 1 rounds; a round that finds nothing unresolved ends the rest early.
//   tails in closed form: past avail an LZSS stream is 21-bit zero-length matches (no output, used = avail), an LZ77
//     stream is (0, 0, 0) tokens that each write a zero byte while bpos < lim.  Work is bounded by the readable bytes and
//     the output, never by csize alone.
// agmv_hip_lz_decode_frames_dev reads avail / usize / csize once (one stream synchronisation) to cut the batch into chunks;
// agmv_hip_lz_decode_frames_sized_dev takes them from host memory and does not synchronise.
// The commit (k_lzc_*): tail byte p of frame f is row j's for the last j < f with bpos_j > p, found by a descent over a
// sparse table of range maxima of bpos; frame order needs no serial pass.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "agmv_hip_impl.h"

constexpr uint32_t LZD_PB = 2048;              // LZSS: bits per piece
constexpr uint32_t LZD_PW = LZD_PB / 32 + 2;   // LDS words of a piece: its bits and the <= 20 a token may run past it
constexpr uint32_t LZD_NE = 21;                // LZSS: entry offsets of a piece (tokens are 9 or 21 bits)
constexpr uint32_t LZD_PPB = 12;               // LZSS: pieces per workgroup of k_lzd_piece (12 x 21 = 252 lanes)
constexpr uint32_t LZD_PT = 256;               // LZ77: tokens per piece
constexpr uint32_t LZD_RES = 0x80000000u;      // word: resolved byte (else the position it copies)
constexpr uint8_t LZD_DEAD = 0xFF;             // piece the stream does not reach
constexpr uint32_t LZD_WORDS = 1u << 26;       // word positions per chunk (a single larger frame gets a chunk of its own)
constexpr uint32_t LZD_PIECES = 1u << 18;      // pieces per chunk (idem)
constexpr uint32_t LZD_FRAMES = 16384;         // frames per chunk (grid y of k_lzd_out)
constexpr uint32_t LZD_ROUNDS = 34;            // pointer-jumping rounds at most (ceil(log2(2^31)) + 1, with room)

// per frame of a chunk, from the host
struct lzd_fd {
	unsigned long long nb;      // LZSS: bits the walk covers (8 min(csize, avail)); LZ77: tokens with readable bytes
	unsigned long long T;       // LZ77: tokens of the stream, ceil(csize / 4); LZSS: 8 csize
	uint32_t R;                 // readable payload bytes, min(avail, csize + 3)
	uint32_t leff;              // LZSS: a token at pos >= leff = min(usize, lim) is not read; LZ77: lim
	uint32_t W;                 // word positions of the frame (its output below lim that tokens can write, bounded)
	uint32_t wbase;             // first word of the frame in the chunk's word area
	uint32_t avail;
	uint32_t pad;
};

// per frame of a chunk, on the device
struct lzd_fs {
	unsigned long long ebits;   // LZSS: bit position at which the stream stops
	unsigned long long epos;    // true output position there (LZ77: behind the readable tokens), not clipped to lim
	uint32_t fb;                // 1: left to the serial kernel
	uint32_t wlen;              // output positions the word area holds
};

// last k in [0, n) with tab[k] <= x (tab ascending, tab[0] <= x)
__device__ __forceinline__ uint32_t lzd_upper(const uint32_t* __restrict__ tab, uint32_t n, uint32_t x)
{
	uint32_t lo = 0, hi = n - 1;
	for (int it = 0; it < 32 && lo < hi; it++) {
		const uint32_t mid = (lo + hi + 1) >> 1;
		if (tab[mid] <= x) lo = mid; else hi = mid - 1;
	}
	return lo;
}

__device__ __forceinline__ uint32_t rd8(const uint8_t* __restrict__ p, uint32_t R, unsigned long long i)
{
	return i < R ? (uint32_t)p[i] : 0u;
}

// >= 25 bits of the stream from bit b on (bytes at or past R read as 0)
__device__ __forceinline__ uint32_t rdbits(const uint8_t* __restrict__ p, uint32_t R, unsigned long long b)
{
	const unsigned long long i = b >> 3;
	const uint32_t v = rd8(p, R, i) | rd8(p, R, i + 1) << 8 | rd8(p, R, i + 2) << 16 | rd8(p, R, i + 3) << 24;
	return v >> (b & 7u);
}

__device__ __forceinline__ uint32_t lz77_count(uint32_t off, uint32_t len, unsigned long long pos)
{
	if (off == 0) return 0;
	if (off <= pos) return len;
	const unsigned long long d = off - pos;
	return (pos > 0 && len > d) ? len - (uint32_t)d : 0u;
}

// ---------------------------------------------------------------------------------------------------------------------
// token starts and nominal lengths per piece
// ---------------------------------------------------------------------------------------------------------------------
// LZSS: piece q entered at offset e (0..20): where its walk leaves (bits from the piece start) and its nominal output
__global__ void __launch_bounds__(256) k_lzd_spiece(uint32_t npieces, const uint32_t* __restrict__ pbase, uint32_t nf,
                                                    const lzd_fd* __restrict__ fd, const uint8_t* __restrict__ src,
                                                    const unsigned long long* __restrict__ off, uint32_t f0,
                                                    uint16_t* __restrict__ pexit, uint32_t* __restrict__ psum)
{
	__shared__ uint32_t wds[LZD_PPB * LZD_PW];
	const uint32_t q0 = blockIdx.x * LZD_PPB;
	for (uint32_t i = threadIdx.x; i < LZD_PPB * LZD_PW; i += 256) {
		const uint32_t q = q0 + i / LZD_PW, w = i % LZD_PW;
		uint32_t v = 0;
		if (q < npieces) {
			const uint32_t k = lzd_upper(pbase, nf + 1, q);
			const uint8_t* p = src + off[f0 + k];
			const unsigned long long b0 = (unsigned long long)(q - pbase[k]) * (LZD_PB / 8) + 4ull * w;
			const uint32_t R = fd[k].R;
			v = rd8(p, R, b0) | rd8(p, R, b0 + 1) << 8 | rd8(p, R, b0 + 2) << 16 | rd8(p, R, b0 + 3) << 24;
		}
		wds[i] = v;
	}
	__syncthreads();
	const uint32_t lq = threadIdx.x / LZD_NE, e = threadIdx.x % LZD_NE, q = q0 + lq;
	if (lq >= LZD_PPB || q >= npieces) return;
	const uint32_t k = lzd_upper(pbase, nf + 1, q);
	const unsigned long long start = (unsigned long long)(q - pbase[k]) * LZD_PB;
	const unsigned long long nb = fd[k].nb;
	const uint32_t end = (uint32_t)(nb - start < LZD_PB ? nb - start : LZD_PB);     // bits of this piece
	const uint32_t* w = wds + lq * LZD_PW;
	uint32_t b = e, sum = 0;
	while (b < end) {
		const uint32_t i = b >> 5, sh = b & 31u;
		const uint32_t v = (uint32_t)((((unsigned long long)w[i + 1] << 32) | w[i]) >> sh);
		if (v & 1u) { sum += 1; b += 9; }
		else { const uint32_t o = (v >> 1) & 0xFFFFu, len = (v >> 17) & 15u; sum += o ? len : 0u; b += 21; }
	}
	pexit[q * LZD_NE + e] = (uint16_t)b;
	psum[q * LZD_NE + e] = sum;
}

// LZ77: nominal output of piece q (tokens [j LZD_PT, min((j+1) LZD_PT, nb)) of its frame)
__global__ void __launch_bounds__(256) k_lzd_tpiece(uint32_t npieces, const uint32_t* __restrict__ pbase, uint32_t nf,
                                                    const lzd_fd* __restrict__ fd, const uint8_t* __restrict__ src,
                                                    const unsigned long long* __restrict__ off, uint32_t f0,
                                                    uint32_t* __restrict__ psum)
{
	const uint32_t q = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
	if (q >= npieces) return;
	const uint32_t k = lzd_upper(pbase, nf + 1, q);
	const uint8_t* p = src + off[f0 + k];
	const uint32_t R = fd[k].R;
	const unsigned long long t0 = (unsigned long long)(q - pbase[k]) * LZD_PT, nb = fd[k].nb;
	uint32_t sum = 0;
	for (uint32_t s = lane; s < LZD_PT && t0 + s < nb; s += 64) {     // nominal lengths: offset <= pos taken for granted
		const unsigned long long a = 4ull * (t0 + s);
		const uint32_t o = rd8(p, R, a) | rd8(p, R, a + 1) << 8, len = rd8(p, R, a + 2);
		sum += (o ? len : 0u) + 1u;
	}
	for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
	if (lane == 0) psum[q] = sum;
}

// one lane per frame: chain the pieces from offset 0, mark the pieces the stream does not reach, and a first guess of
// where it stops (k_lzd_emit writes the truth where a piece knows better)
template <bool LZSS>
__global__ void __launch_bounds__(64) k_lzd_chain(uint32_t nf, const uint32_t* __restrict__ pbase, const lzd_fd* __restrict__ fd,
                                                  const uint16_t* __restrict__ pexit, const uint32_t* __restrict__ psum,
                                                  uint8_t* __restrict__ pentry, unsigned long long* __restrict__ ppos,
                                                  lzd_fs* __restrict__ fs)
{
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= nf) return;
	const unsigned long long nb = fd[k].nb, leff = fd[k].leff;
	unsigned long long pos = 0, bits = 0;
	uint32_t e = 0;
	bool live = true;
	for (uint32_t q = pbase[k]; q < pbase[k + 1]; q++) {
		const unsigned long long start = (unsigned long long)(q - pbase[k]) * (LZSS ? LZD_PB : LZD_PT);
		if (live && (pos >= leff || (LZSS && start + e >= nb))) { live = false; bits = start + e; }
		if (!live) { pentry[q] = LZD_DEAD; continue; }
		pentry[q] = (uint8_t)e;
		ppos[q] = pos;
		if (LZSS) {
			pos += psum[q * LZD_NE + e];
			const uint32_t x = pexit[q * LZD_NE + e];
			bits = start + x;
			e = x >= LZD_PB ? min(x - LZD_PB, LZD_NE - 1) : 0u;          // (<= 20 by construction; the clamp keeps reads in range)
		} else {
			pos += psum[q];
		}
	}
	fs[k].ebits = bits;
	fs[k].epos = pos;
	fs[k].fb = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// emission: one lane per live piece, from its true entry.  Words of positions >= W are not written.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_match(uint32_t* __restrict__ words, uint32_t wbase, uint32_t W, unsigned long long pos,
                                          uint32_t cnt, unsigned long long back)
{
	for (uint32_t i = 0; i < cnt && pos + i < W; i++) words[wbase + pos + i] = wbase + (uint32_t)(pos + i - back);
}

__global__ void __launch_bounds__(256) k_lzd_semit(uint32_t npieces, const uint32_t* __restrict__ pbase, uint32_t nf,
                                                   const lzd_fd* __restrict__ fd, const uint8_t* __restrict__ src,
                                                   const unsigned long long* __restrict__ off, uint32_t f0,
                                                   const uint8_t* __restrict__ pentry, const unsigned long long* __restrict__ ppos,
                                                   uint32_t* __restrict__ words, lzd_fs* __restrict__ fs)
{
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	if (q >= npieces || pentry[q] == LZD_DEAD) return;
	const uint32_t k = lzd_upper(pbase, nf + 1, q);
	const lzd_fd d = fd[k];
	const uint8_t* p = src + off[f0 + k];
	const unsigned long long start = (unsigned long long)(q - pbase[k]) * LZD_PB;
	const unsigned long long end = d.nb - start < LZD_PB ? d.nb : start + LZD_PB;
	unsigned long long b = start + pentry[q], pos = ppos[q];
	bool wrapped = false;
	while (b < end) {
		if (pos >= d.leff) { fs[k].ebits = b; fs[k].epos = pos; return; }        // the token the reference does not read
		if (wrapped) { fs[k].fb = 1; return; }                                    // a token behind a match with offset > pos
		const uint32_t v = rdbits(p, d.R, b);
		if (v & 1u) {
			if (pos < d.W) words[d.wbase + pos] = LZD_RES | ((v >> 1) & 255u);
			pos += 1; b += 9;
		} else {
			const uint32_t o = (v >> 1) & 0xFFFFu, len = (v >> 17) & 15u;
			const uint32_t cnt = lz77_count(o, len, pos);
			if (o > pos) wrapped = true;
			put_match(words, d.wbase, d.W, pos, cnt, o > pos ? pos : (unsigned long long)o);
			pos += cnt; b += 21;
		}
	}
	if (b >= d.nb || pos >= d.leff) { fs[k].ebits = b; fs[k].epos = pos; }     // the stream stops here
	else if (wrapped) fs[k].fb = 1;                                              // ... else the next piece reads on
}

__global__ void __launch_bounds__(256) k_lzd_temit(uint32_t npieces, const uint32_t* __restrict__ pbase, uint32_t nf,
                                                   const lzd_fd* __restrict__ fd, const uint8_t* __restrict__ src,
                                                   const unsigned long long* __restrict__ off, uint32_t f0,
                                                   const uint8_t* __restrict__ pentry, const unsigned long long* __restrict__ ppos,
                                                   uint32_t* __restrict__ words, lzd_fs* __restrict__ fs)
{
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	if (q >= npieces || pentry[q] == LZD_DEAD) return;
	const uint32_t k = lzd_upper(pbase, nf + 1, q);
	const lzd_fd d = fd[k];
	const uint8_t* p = src + off[f0 + k];
	const unsigned long long t0 = (unsigned long long)(q - pbase[k]) * LZD_PT;
	const unsigned long long t1 = d.nb - t0 < LZD_PT ? d.nb : t0 + LZD_PT;
	unsigned long long pos = ppos[q];
	bool wrapped = false;
	for (unsigned long long t = t0; t < t1; t++) {
		if (pos >= d.leff) break;                                                 // nothing behind lim is written
		if (wrapped) { fs[k].fb = 1; return; }
		const unsigned long long a = 4ull * t;
		const uint32_t o = rd8(p, d.R, a) | rd8(p, d.R, a + 1) << 8, len = rd8(p, d.R, a + 2), byte = rd8(p, d.R, a + 3);
		const uint32_t cnt = lz77_count(o, len, pos);
		if (o > pos) wrapped = true;
		put_match(words, d.wbase, d.W, pos, cnt, o > pos ? pos : (unsigned long long)o);
		pos += cnt;
		if (pos < d.W) words[d.wbase + pos] = LZD_RES | byte;
		pos += 1;
	}
	if (t1 >= d.nb || pos >= d.leff) fs[k].epos = pos;                          // the readable tokens end here
	else if (wrapped) fs[k].fb = 1;
}

// per frame: bpos, used; frames whose output does not fit their words go to the serial kernel
template <bool LZSS>
__global__ void __launch_bounds__(64) k_lzd_final(uint32_t nf, uint32_t f0, const lzd_fd* __restrict__ fd, uint32_t lim,
                                                  lzd_fs* __restrict__ fs, uint32_t* __restrict__ bpos, uint32_t* __restrict__ used,
                                                  uint32_t* __restrict__ nfallback)
{
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= nf) return;
	const lzd_fd d = fd[k];
	lzd_fs s = fs[k];
	const unsigned long long end = s.epos < lim ? s.epos : lim;
	if (!s.fb && end > d.W) s.fb = 1;
	if (s.fb) { fs[k].fb = 1; atomicAdd(nfallback, 1u); return; }
	fs[k].wlen = (uint32_t)end;
	if (LZSS) {
		bpos[f0 + k] = (uint32_t)end;
		const unsigned long long u = (s.ebits + 7) >> 3;
		used[f0 + k] = u < d.avail ? (uint32_t)u : d.avail;
	} else {
		const unsigned long long tz = d.T - d.nb;                              // (0, 0, 0) tokens: one zero byte each
		bpos[f0 + k] = (uint32_t)(end < lim ? (tz < lim - end ? end + tz : lim) : end);
		used[f0 + k] = 4 * d.T < d.avail ? (uint32_t)(4 * d.T) : d.avail;
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// pointer jumping over the chunk's words: word[p] = word[word[p]] until every word is resolved
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lzd_jump(uint32_t n, uint32_t round, uint32_t* __restrict__ flags, uint32_t* words)
{
	if (round > 0 && flags[round - 1] == 0) return;   // the last round found nothing to do
	bool any = false;
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
		const uint32_t w = words[p];
		if (w & LZD_RES) continue;
		words[p] = w < p ? words[w] : LZD_RES;          // (a word always copies a lower one; the guard keeps reads in range)
		any = true;
	}
	if (__any(any) && (threadIdx.x & 63u) == 0) flags[round] = 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// exact fallback: one lane walks a frame as agmv_lz_decode_mem does (tails in closed form)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_lzd_serial(uint32_t nf, uint32_t f0, int lzss, const lzd_fd* __restrict__ fd,
                                                   const uint8_t* __restrict__ src, const unsigned long long* __restrict__ off,
                                                   uint32_t lim, uint8_t* __restrict__ bits, unsigned long long stride,
                                                   lzd_fs* __restrict__ fs, uint32_t* __restrict__ bpos, uint32_t* __restrict__ used)
{
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= nf || !fs[k].fb) return;
	const lzd_fd d = fd[k];
	const uint8_t* p = src + off[f0 + k];
	uint8_t* data = bits + (unsigned long long)(f0 + k) * stride;
	unsigned long long bp = 0;
	if (lzss) {
		unsigned long long b = 0;
		while (b < d.nb && bp < d.leff) {                                         // leff = min(usize, lim)
			const uint32_t v = rdbits(p, d.R, b);
			if (v & 1u) { data[bp++] = (uint8_t)(v >> 1); b += 9; }
			else {
				const uint32_t o = (v >> 1) & 0xFFFFu, len = (v >> 17) & 15u;
				const unsigned long long pos = bp;
				for (uint32_t i = 0; i < len; i++) {
					const unsigned long long s = pos - o + i;
					if (s < bp && bp < lim) { data[bp] = data[s]; bp++; }
				}
				b += 21;
			}
		}
		fs[k].wlen = (uint32_t)bp;
		bpos[f0 + k] = (uint32_t)bp;
		const unsigned long long u = (b + 7) >> 3;
		used[f0 + k] = u < d.avail ? (uint32_t)u : d.avail;
	} else {
		for (unsigned long long t = 0; t < d.nb; t++) {
			const unsigned long long a = 4ull * t;
			const uint32_t o = rd8(p, d.R, a) | rd8(p, d.R, a + 1) << 8, len = rd8(p, d.R, a + 2), byte = rd8(p, d.R, a + 3);
			const unsigned long long pos = bp;
			for (uint32_t i = 0; i < len; i++) {
				const unsigned long long s = pos - o + i;
				if (s < bp && bp < lim) { data[bp] = data[s]; bp++; }
			}
			if (bp < lim) data[bp++] = (uint8_t)byte;
		}
		fs[k].wlen = (uint32_t)bp;                                                // k_lzd_out writes the zero tail
		const unsigned long long tz = d.T - d.nb;
		bpos[f0 + k] = (uint32_t)(bp < lim ? (tz < lim - bp ? bp + tz : lim) : bp);
		used[f0 + k] = 4 * d.T < d.avail ? (uint32_t)(4 * d.T) : d.avail;
	}
}

// row bytes [0, bpos): from the words below wlen, zero above (LZ77's tail); the serial kernel wrote [0, wlen) of its frames
__global__ void __launch_bounds__(256) k_lzd_out(uint32_t f0, const lzd_fd* __restrict__ fd, const lzd_fs* __restrict__ fs,
                                                 const uint32_t* __restrict__ words, const uint32_t* __restrict__ bpos,
                                                 uint8_t* __restrict__ bits, unsigned long long stride)
{
	const uint32_t k = blockIdx.y;
	const uint32_t n = bpos[f0 + k], wlen = fs[k].wlen, wbase = fd[k].wbase;
	const bool fb = fs[k].fb != 0;
	uint8_t* data = bits + (unsigned long long)(f0 + k) * stride;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		if (i < wlen) { if (!fb) data[i] = (uint8_t)words[wbase + i]; }
		else data[i] = 0;
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// the persistent buffer: frame f's tail byte p in [bp_f, bp_f + 16) is row j's byte p for the last j < f with bp_j > p
// (or the buffer's, if there is none); the buffer's byte p becomes row j's for the last j of all with bp_j > p.  "The last
// j < f with bp_j > p" is a descent over a sparse table of range maxima of bp (level L: max over 2^L frames).
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lzc_level(uint32_t n, uint32_t half, const uint32_t* __restrict__ lo, uint32_t* __restrict__ hi)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	hi[i] = i + half < n ? max(lo[i], lo[i + half]) : lo[i];
}

// smallest j <= f such that every bp in [j, f) is <= x
__device__ __forceinline__ uint32_t lzc_descend(const uint32_t* __restrict__ tab, uint32_t n, uint32_t levels, uint32_t f, uint32_t x)
{
	uint32_t j = f;
	for (int L = (int)levels - 1; L >= 0; L--) {
		const uint32_t s = 1u << L;
		if (j >= s && tab[(size_t)L * n + (j - s)] <= x) j -= s;
	}
	return j;
}

__global__ void __launch_bounds__(256) k_lzc_tail(uint32_t n, uint32_t levels, const uint32_t* __restrict__ tab,
                                                  uint8_t* __restrict__ bits, unsigned long long stride, unsigned long long cap,
                                                  const uint8_t* __restrict__ persist)
{
	const uint32_t g = blockIdx.x * 256u + threadIdx.x, f = g >> 4;
	if (f >= n) return;
	const unsigned long long p = (unsigned long long)tab[f] + (g & 15u);
	if (p >= stride || p >= cap) return;
	const uint32_t j = lzc_descend(tab, n, levels, f, (uint32_t)p);
	bits[(unsigned long long)f * stride + p] = j ? bits[(unsigned long long)(j - 1) * stride + p] : persist[p];
}

__global__ void __launch_bounds__(256) k_lzc_persist(uint32_t n, uint32_t levels, const uint32_t* __restrict__ tab,
                                                     const uint8_t* __restrict__ bits, unsigned long long stride,
                                                     unsigned long long cap, uint8_t* __restrict__ persist)
{
	const uint32_t m = tab[(size_t)(levels - 1) * n];                        // max over all frames (2^(levels-1) >= n)
	for (unsigned long long p = blockIdx.x * 256ull + threadIdx.x; p < cap && p < m; p += gridDim.x * 256ull) {
		const uint32_t j = lzc_descend(tab, n, levels, n, (uint32_t)p);
		if (j) persist[p] = bits[(unsigned long long)(j - 1) * stride + p];
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// work areas (per context, grown on demand)
// ---------------------------------------------------------------------------------------------------------------------
struct lzd_ws {
	size_t cap_words; uint32_t* words;
	size_t cap_pieces; uint16_t* pexit; uint32_t* psum; uint8_t* pentry; unsigned long long* ppos;
	size_t cap_fd; lzd_fd* fd; lzd_fs* fs;          // n_frames entries each
	size_t cap_pb; uint32_t* pbase;                  // n_frames + chunks entries
	size_t cap_stage; uint8_t* h_stage;              // pinned: fd and pbase of a call on their way to the device ...
	hipEvent_t ev_up;                                // ... and the end of their upload (the staging is rewritten after it)
	hipEvent_t ev_done;                              // end of the last call's work: a work area is freed (to grow) after it
	size_t cap_tab; uint32_t* tab;                  // commit: sparse table
	uint32_t* ctl;                                  // [0] fallback frames of the last call, [1 ..] round flags
};

static void lzd_free(void* p)
{
	lzd_ws* w = (lzd_ws*)p;
	void* all[] = {w->words, w->pexit, w->psum, w->pentry, w->ppos, w->fd, w->fs, w->pbase, w->tab, w->ctl};
	for (void* a : all) if (a) (void)hipFree(a);
	if (w->ev_done) { (void)hipEventSynchronize(w->ev_done); (void)hipEventDestroy(w->ev_done); }
	if (w->ev_up) { (void)hipEventSynchronize(w->ev_up); (void)hipEventDestroy(w->ev_up); }
	if (w->h_stage) (void)hipHostFree(w->h_stage);
	free(w);
}

static lzd_ws* lzd_get(agmv_hip_ctx* c)
{
	lzd_ws* w = (lzd_ws*)agmv_hip_area(c, AREA_LZ_DECODE, sizeof(lzd_ws), lzd_free);
	if (w && !w->ctl && (hipMalloc((void**)&w->ctl, (1 + LZD_ROUNDS) * 4) != hipSuccess || hipMemset(w->ctl, 0, (1 + LZD_ROUNDS) * 4) != hipSuccess)) {
		(void)hipFree(w->ctl);
		w->ctl = nullptr;
		agmv_hip_err("agmv_hip: LZ decode work area: hipMalloc failed");
		return nullptr;
	}
	return w;
}

static int lzd_mark_done(lzd_ws* w, hipStream_t s)
{
	if (!w->ev_done) CK(hipEventCreateWithFlags(&w->ev_done, hipEventDisableTiming));
	CK(hipEventRecord(w->ev_done, s));
	return 0;
}

static uint32_t ceil_log2(unsigned long long x) { uint32_t b = 0; while ((1ull << b) < x) b++; return b; }

static int lzd_frames(agmv_hip_ctx* c, int version, const uint8_t* d_src, const unsigned long long* d_off, const uint32_t* h_avail,
                      const uint32_t* h_usize, const uint32_t* h_csize, uint32_t n_frames, uint8_t* d_bits, size_t bits_stride,
                      size_t cap, uint32_t* d_bpos, uint32_t* d_used, hipStream_t s)
{
	lzd_ws* w = lzd_get(c);
	if (!w) return -1;
	const bool lzss = version == 1 || version == 2;
	const unsigned long long lim = cap > 16 ? cap - 16 : 0;
	CK(hipMemsetAsync(w->ctl, 0, 4, s));
	// per frame: readable bytes, the walk's extent, word positions; chunks of frames
	struct chunk { uint32_t f0, nf, npieces, nwords, maxw; };
	std::vector<lzd_fd> fd(n_frames);
	std::vector<uint32_t> pb;
	std::vector<chunk> ch;
	pb.reserve(n_frames + 64);
	size_t maxp = 1, maxwords = 1, maxnf = 1;
	for (uint32_t f = 0; f < n_frames;) {
		chunk k = {f, 0, 0, 0, 1};
		while (f < n_frames && k.nf < LZD_FRAMES) {
			lzd_fd& d = fd[f];
			const unsigned long long avail = h_avail[f], csize = h_csize[f], usize = h_usize[f];
			d.R = (uint32_t)(avail < csize + 3 ? avail : csize + 3);
			d.avail = (uint32_t)avail;
			d.pad = 0;
			unsigned long long W, np;
			if (lzss) {
				d.nb = 8 * (avail < csize ? avail : csize);
				d.T = 8 * csize;
				d.leff = (uint32_t)(usize < lim ? usize : lim);
				W = usize + 15;
				if (15 * (d.nb / 9 + 1) < W) W = 15 * (d.nb / 9 + 1);
				np = (d.nb + LZD_PB - 1) / LZD_PB;
			} else {
				d.T = (csize + 3) / 4;
				d.nb = (avail + 3) / 4 < d.T ? (avail + 3) / 4 : d.T;
				d.leff = (uint32_t)lim;
				W = usize + 256;
				if (256 * d.nb < W) W = 256 * d.nb;
				np = (d.nb + LZD_PT - 1) / LZD_PT;
			}
			if (W > lim) W = lim;
			d.W = (uint32_t)W;
			if (k.nf && ((unsigned long long)k.nwords + W > LZD_WORDS || (unsigned long long)k.npieces + np > LZD_PIECES)) break;
			if ((unsigned long long)k.nwords + W >= (1ull << 31) || (unsigned long long)k.npieces + np >= (1ull << 31))
				return agmv_hip_err("agmv_hip_lz_decode_frames_dev: frame %u is too large (%llu output words, %llu pieces)", f, W, np);
			d.wbase = k.nwords;
			pb.push_back(k.npieces);
			k.nwords += (uint32_t)W;
			k.npieces += (uint32_t)np;
			if (W > k.maxw) k.maxw = (uint32_t)W;
			k.nf++;
			f++;
		}
		pb.push_back(k.npieces);
		if (k.npieces > maxp) maxp = k.npieces;
		if (k.nwords > maxwords) maxwords = k.nwords;
		if (k.nf > maxnf) maxnf = k.nf;
		ch.push_back(k);
	}
	const size_t nfd = n_frames, npb = pb.size();     // fd and fs: one entry per frame of the call; pbase: per frame and chunk
	if ((maxwords > w->cap_words || maxp > w->cap_pieces || nfd > w->cap_fd || npb > w->cap_pb) && w->ev_done)
		CK(hipEventSynchronize(w->ev_done));           // the areas about to be replaced may still be in use by the last call
	CK(agmv_hip_dev_grow(&w->words, &w->cap_words, maxwords));
	if (maxp > w->cap_pieces) {                                    // a shared capacity is committed when all its buffers exist
		w->cap_pieces = 0;
		CK(agmv_hip_dev_grow(&w->pexit, nullptr, maxp * LZD_NE));
		CK(agmv_hip_dev_grow(&w->psum, nullptr, maxp * LZD_NE));
		CK(agmv_hip_dev_grow(&w->pentry, nullptr, maxp));
		CK(agmv_hip_dev_grow(&w->ppos, nullptr, maxp));
		w->cap_pieces = maxp;
	}
	if (nfd > w->cap_fd) {
		w->cap_fd = 0;
		CK(agmv_hip_dev_grow(&w->fd, nullptr, nfd));
		CK(agmv_hip_dev_grow(&w->fs, nullptr, nfd));
		w->cap_fd = nfd;
	}
	CK(agmv_hip_dev_grow(&w->pbase, &w->cap_pb, npb));
	// the tables go up from pinned staging, without a stream synchronisation: the staging is rewritten only once the
	// upload of the previous call has ended
	const size_t fdb = nfd * sizeof(lzd_fd), stage = fdb + npb * 4;
	if (!w->ev_up) CK(hipEventCreateWithFlags(&w->ev_up, hipEventDisableTiming));
	else CK(hipEventSynchronize(w->ev_up));
	if (stage > w->cap_stage) {
		if (w->h_stage) CK(hipHostFree(w->h_stage));
		w->h_stage = nullptr; w->cap_stage = 0;
		CK(hipHostMalloc((void**)&w->h_stage, stage, hipHostMallocDefault));
		w->cap_stage = stage;
	}
	memcpy(w->h_stage, fd.data(), fdb);
	memcpy(w->h_stage + fdb, pb.data(), npb * 4);
	CK(hipMemcpyAsync(w->fd, w->h_stage, fdb, hipMemcpyHostToDevice, s));
	CK(hipMemcpyAsync(w->pbase, w->h_stage + fdb, npb * 4, hipMemcpyHostToDevice, s));
	CK(hipEventRecord(w->ev_up, s));

	size_t pbo = 0;
	for (const chunk& k : ch) {
		const lzd_fd* fdk = w->fd + k.f0;
		const uint32_t* pbk = w->pbase + pbo;
		lzd_fs* fsk = w->fs + k.f0;
		pbo += k.nf + 1;
		const uint32_t rounds = ceil_log2(k.maxw) + 1;
		CK(hipMemsetD32Async((hipDeviceptr_t)w->words, (int)LZD_RES, k.nwords ? k.nwords : 1, s));
		CK(hipMemsetAsync(w->ctl + 1, 0, LZD_ROUNDS * 4, s));
		if (lzss) {
			if (k.npieces)
				hipLaunchKernelGGL(k_lzd_spiece, dim3((k.npieces + LZD_PPB - 1) / LZD_PPB), dim3(256), 0, s, k.npieces, pbk, k.nf, fdk,
				                   d_src, d_off, k.f0, w->pexit, w->psum);
			hipLaunchKernelGGL(k_lzd_chain<true>, dim3((k.nf + 63) / 64), dim3(64), 0, s, k.nf, pbk, fdk, w->pexit, w->psum, w->pentry,
			                   w->ppos, fsk);
			if (k.npieces)
				hipLaunchKernelGGL(k_lzd_semit, dim3((k.npieces + 255) / 256), dim3(256), 0, s, k.npieces, pbk, k.nf, fdk, d_src, d_off,
				                   k.f0, w->pentry, w->ppos, w->words, fsk);
			hipLaunchKernelGGL(k_lzd_final<true>, dim3((k.nf + 63) / 64), dim3(64), 0, s, k.nf, k.f0, fdk, (uint32_t)lim, fsk, d_bpos,
			                   d_used, w->ctl);
		} else {
			if (k.npieces)
				hipLaunchKernelGGL(k_lzd_tpiece, dim3((k.npieces + 3) / 4), dim3(256), 0, s, k.npieces, pbk, k.nf, fdk, d_src, d_off,
				                   k.f0, w->psum);
			hipLaunchKernelGGL(k_lzd_chain<false>, dim3((k.nf + 63) / 64), dim3(64), 0, s, k.nf, pbk, fdk, w->pexit, w->psum, w->pentry,
			                   w->ppos, fsk);
			if (k.npieces)
				hipLaunchKernelGGL(k_lzd_temit, dim3((k.npieces + 255) / 256), dim3(256), 0, s, k.npieces, pbk, k.nf, fdk, d_src, d_off,
				                   k.f0, w->pentry, w->ppos, w->words, fsk);
			hipLaunchKernelGGL(k_lzd_final<false>, dim3((k.nf + 63) / 64), dim3(64), 0, s, k.nf, k.f0, fdk, (uint32_t)lim, fsk, d_bpos,
			                   d_used, w->ctl);
		}
		CK(hipGetLastError());
		if (k.nwords) {
			const uint32_t g = (k.nwords + 1023) / 1024;
			for (uint32_t r = 0; r < rounds; r++)
				hipLaunchKernelGGL(k_lzd_jump, dim3(g < 8192 ? g : 8192), dim3(256), 0, s, k.nwords, r, w->ctl + 1, w->words);
			CK(hipGetLastError());
		}
		hipLaunchKernelGGL(k_lzd_serial, dim3((k.nf + 63) / 64), dim3(64), 0, s, k.nf, k.f0, lzss ? 1 : 0, fdk, d_src, d_off,
		                   (uint32_t)lim, d_bits, (unsigned long long)bits_stride, fsk, d_bpos, d_used);
		const unsigned long long gx = (lim + 4095) / 4096;
		hipLaunchKernelGGL(k_lzd_out, dim3(gx < 1 ? 1 : (gx > 1024 ? 1024 : (uint32_t)gx), k.nf), dim3(256), 0, s, k.f0, fdk, fsk,
		                   w->words, d_bpos, d_bits, (unsigned long long)bits_stride);
		CK(hipGetLastError());
	}
	return lzd_mark_done(w, s);
}

static int check_args(agmv_hip_ctx* c, size_t bits_stride, size_t cap, const char* who)
{
	if (!c) return agmv_hip_err("agmv_hip: NULL context");
	if (cap > bits_stride || cap >= (1ull << 31)) return agmv_hip_err("%s: cap %zu must be <= bits_stride %zu and < 2^31", who, cap, bits_stride);
	return 0;
}

extern "C" int agmv_hip_lz_decode_frames_dev(agmv_hip_ctx* c, int version, const uint8_t* d_src, const unsigned long long* d_off,
                                             const uint32_t* d_avail, const uint32_t* d_usize, const uint32_t* d_csize, uint32_t n_frames,
                                             uint8_t* d_bits, size_t bits_stride, size_t cap, uint32_t* d_bpos, uint32_t* d_used,
                                             void* stream)
{
	if (check_args(c, bits_stride, cap, "agmv_hip_lz_decode_frames_dev")) return -1;
	CK(hipSetDevice(c->device));
	hipStream_t s = (hipStream_t)stream;
	if (n_frames == 0) {
		lzd_ws* w = lzd_get(c);
		if (!w) return -1;
		CK(hipMemsetAsync(w->ctl, 0, 4, s));
		return 0;
	}
	std::vector<uint32_t> h((size_t)3 * n_frames);     // the sizes decide the chunks: read them once
	CK(hipMemcpyAsync(h.data(), d_avail, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s));
	CK(hipMemcpyAsync(h.data() + n_frames, d_usize, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s));
	CK(hipMemcpyAsync(h.data() + 2 * (size_t)n_frames, d_csize, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s));
	CK(hipStreamSynchronize(s));
	return lzd_frames(c, version, d_src, d_off, h.data(), h.data() + n_frames, h.data() + 2 * (size_t)n_frames, n_frames, d_bits,
	                  bits_stride, cap, d_bpos, d_used, s);
}

extern "C" int agmv_hip_lz_decode_frames_sized_dev(agmv_hip_ctx* c, int version, const uint8_t* d_src, const unsigned long long* d_off,
                                                   const uint32_t* h_avail, const uint32_t* h_usize, const uint32_t* h_csize,
                                                   uint32_t n_frames, uint8_t* d_bits, size_t bits_stride, size_t cap, uint32_t* d_bpos,
                                                   uint32_t* d_used, void* stream)
{
	if (check_args(c, bits_stride, cap, "agmv_hip_lz_decode_frames_sized_dev")) return -1;
	CK(hipSetDevice(c->device));
	hipStream_t s = (hipStream_t)stream;
	if (n_frames == 0) {
		lzd_ws* w = lzd_get(c);
		if (!w) return -1;
		CK(hipMemsetAsync(w->ctl, 0, 4, s));
		return 0;
	}
	return lzd_frames(c, version, d_src, d_off, h_avail, h_usize, h_csize, n_frames, d_bits, bits_stride, cap, d_bpos, d_used, s);
}

extern "C" int agmv_hip_lz_decode_commit_dev(agmv_hip_ctx* c, uint8_t* d_bits, size_t bits_stride, const uint32_t* d_bpos,
                                             uint32_t n_frames, uint8_t* d_persist, size_t cap, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0 || cap == 0) return 0;
	hipStream_t s = (hipStream_t)stream;
	lzd_ws* w = lzd_get(c);
	if (!w) return -1;
	const uint32_t levels = ceil_log2(n_frames) + 1, n = n_frames;
	if ((size_t)levels * n > w->cap_tab && w->ev_done) CK(hipEventSynchronize(w->ev_done));
	CK(agmv_hip_dev_grow(&w->tab, &w->cap_tab, (size_t)levels * n));
	CK(hipMemcpyAsync(w->tab, d_bpos, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
	for (uint32_t L = 1; L < levels; L++)
		hipLaunchKernelGGL(k_lzc_level, dim3((n + 255) / 256), dim3(256), 0, s, n, 1u << (L - 1), w->tab + (size_t)(L - 1) * n,
		                   w->tab + (size_t)L * n);
	hipLaunchKernelGGL(k_lzc_tail, dim3((16 * (size_t)n + 255) / 256), dim3(256), 0, s, n, levels, w->tab, d_bits,
	                   (unsigned long long)bits_stride, (unsigned long long)cap, d_persist);
	const unsigned long long g = (cap + 1023) / 1024;
	hipLaunchKernelGGL(k_lzc_persist, dim3(g > 4096 ? 4096 : (uint32_t)g), dim3(256), 0, s, n, levels, w->tab, d_bits,
	                   (unsigned long long)bits_stride, (unsigned long long)cap, d_persist);
	CK(hipGetLastError());
	return lzd_mark_done(w, s);
}

extern "C" int agmv_hip_lz_decode_fallback_frames(agmv_hip_ctx* c, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	const lzd_ws* w = (const lzd_ws*)c->ws[AREA_LZ_DECODE];
	if (!w || !w->ctl) return 0;
	uint32_t v = 0;
	CK(hipStreamSynchronize((hipStream_t)stream));
	CK(hipMemcpy(&v, w->ctl, 4, hipMemcpyDeviceToHost));
	return (int)v;
}

extern "C" int agmv_hip_lz_decode_frames(agmv_hip_ctx* c, int version, const uint8_t* h_src, size_t src_len,
                                         const unsigned long long* h_off, const uint32_t* h_avail, const uint32_t* h_usize,
                                         const uint32_t* h_csize, uint32_t n_frames, uint8_t* h_bits, size_t bits_stride, size_t cap,
                                         uint32_t* h_bpos, uint32_t* h_used, uint8_t* h_persist)
{
	if (check_args(c, bits_stride, cap, "agmv_hip_lz_decode_frames")) return -1;
	CK(hipSetDevice(c->device));
	if (n_frames == 0) return 0;
	for (uint32_t f = 0; f < n_frames; f++) {
		const unsigned long long r = h_avail[f] < (unsigned long long)h_csize[f] + 3 ? h_avail[f] : (unsigned long long)h_csize[f] + 3;
		if (h_off[f] > src_len || r > src_len - h_off[f])
			return agmv_hip_err("agmv_hip_lz_decode_frames: frame %u reads %llu bytes at %llu of a %zu-byte source", f, r, h_off[f], src_len);
	}
	uint8_t *dsrc = nullptr, *dbits = nullptr, *dper = nullptr;
	unsigned long long* doff = nullptr;
	uint32_t *dbp = nullptr, *dused = nullptr;
	int rc = -1;
	hipError_t e;
	if ((e = hipMalloc((void**)&dsrc, src_len + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&dbits, (size_t)n_frames * bits_stride + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&dper, cap + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&doff, (size_t)n_frames * 8)) != hipSuccess ||
	    (e = hipMalloc((void**)&dbp, (size_t)n_frames * 4)) != hipSuccess ||
	    (e = hipMalloc((void**)&dused, (size_t)n_frames * 4)) != hipSuccess ||
	    (src_len && (e = hipMemcpy(dsrc, h_src, src_len, hipMemcpyHostToDevice)) != hipSuccess) ||
	    (e = hipMemcpy(doff, h_off, (size_t)n_frames * 8, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = hipMemcpy(dbits, h_bits, (size_t)n_frames * bits_stride, hipMemcpyHostToDevice)) != hipSuccess ||
	    (h_persist ? (e = hipMemcpy(dper, h_persist, cap, hipMemcpyHostToDevice)) : (e = hipMemset(dper, 0, cap))) != hipSuccess) {
		agmv_hip_hip_failed("agmv_hip_lz_decode_frames", e, __FILE_NAME__, __LINE__);
		goto done;
	}
	if (lzd_frames(c, version, dsrc, doff, h_avail, h_usize, h_csize, n_frames, dbits, bits_stride, cap, dbp, dused, nullptr) ||
	    agmv_hip_lz_decode_commit_dev(c, dbits, bits_stride, dbp, n_frames, dper, cap, nullptr))
		goto done;
	if ((e = hipDeviceSynchronize()) != hipSuccess ||
	    (e = hipMemcpy(h_bpos, dbp, (size_t)n_frames * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
	    (e = hipMemcpy(h_used, dused, (size_t)n_frames * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
	    (e = hipMemcpy(h_bits, dbits, (size_t)n_frames * bits_stride, hipMemcpyDeviceToHost)) != hipSuccess ||
	    (h_persist && (e = hipMemcpy(h_persist, dper, cap, hipMemcpyDeviceToHost)) != hipSuccess)) {
		agmv_hip_hip_failed("agmv_hip_lz_decode_frames", e, __FILE_NAME__, __LINE__);
		goto done;
	}
	rc = 0;
done:
	(void)hipFree(dsrc); (void)hipFree(dbits); (void)hipFree(dper); (void)hipFree(doff); (void)hipFree(dbp); (void)hipFree(dused);
	return rc;
}
