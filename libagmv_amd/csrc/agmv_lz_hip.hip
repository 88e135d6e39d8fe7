// libagmv_amd/csrc/agmv_lz_hip.hip -- the LZSS stage of AGMV_EncodeFrame on the GPU (reference src/agmv_encode.c:106-177,
// AGMV_FlushWriteBits src/agmv_utils.c:106-112, csize :567-585 / :622-624), bit-exact, for a batch of pre-LZ bitstreams.
//
// Contract (the reference's AGMV_LZSS, restated): at token position i the match is the longest common prefix of d[j..]
// and d[i..], capped at min(15, n-i), over j in [max(0, i-65535), i); the earliest j wins among equals.  Below 3 the
// token is a literal (1, 8 bits of d[i]), else a match (0, 16 bits of i-j, 4 bits of length); LSB-first.
// csize = (u32)((float)outbits / 8.0f); the payload is csize bytes, the last one the partial byte when the float
// rounded up.
//
// Design:
//   match finding, position-parallel: "an L-gram of i occurs in the window" is monotone in L, so the match at i is
//     L* = the largest L <= cap for which it occurs, with start E_L*(i) = the earliest in-window occurrence.  The
//     positions of a chunk of frames are kept sorted by (frame, L-gram, position) for L = 3, 4, ..., 15: level 3 by one
//     radix sort of (frame, 3 bytes), every further level by a stable radix sort of (group rank, next byte) -- the
//     groups of level L are split by byte L, position order inside a group is kept.  In that order the members of i's
//     group that lie in the window are the <= 65535 entries just before i: the one before i decides whether the gram
//     occurs, a 17-step binary search finds the earliest.  Work per position and level is bounded by constants.
//   parse: the greedy parse has a carry of 0..14 positions.  Pieces of LZ_P positions are walked from every entry offset
//     (k_lz_piece); one lane per frame chains the pieces (k_lz_fscan); every piece then emits its tokens from its true
//     entry at its bit offset (k_lz_emit) into a zeroed word buffer: words a piece fills alone are stored, the two it
//     may share with its neighbours are OR-ed in.  k_lz_copy writes the csize bytes of each frame.
// The host reads the sizes once (one stream synchronisation) to cut the batch into chunks of <= LZ_CHUNK positions.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "agmv_hip_impl.h"

constexpr uint32_t LZ_WIN = 65535;            // matches start in [i - 65535, i)
constexpr uint32_t LZ_MAXLEN = 15;
constexpr uint32_t LZ_CHUNK = 1u << 24;       // positions per chunk: (group rank << 8 | byte) stays a 32-bit key
constexpr uint32_t LZ_CHUNK_FRAMES = 256;     // frames per chunk: (frame << 24 | 3 bytes) is the level-3 key
constexpr uint32_t LZ_PAD = 64;               // readable zero bytes behind a chunk (keys read up to 14 bytes ahead)
constexpr uint32_t LZ_P = 512;                // positions per parse piece
constexpr uint32_t RS_TILE = 1024;            // radix sort: elements per tile (one wave, 16 rounds of 64)
constexpr uint32_t SC_BLOCK = 1024;           // scan: elements per block (256 lanes x 4)

// ---------------------------------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------------------------------
// last k in [0, n) with tab[k] <= x (tab ascending, tab[0] <= x); bounded by 32 halvings
__device__ __forceinline__ uint32_t upper_idx(const uint32_t* __restrict__ tab, uint32_t n, uint32_t x)
{
	uint32_t lo = 0, hi = n - 1;
	for (int it = 0; it < 32 && lo < hi; it++) {
		const uint32_t mid = (lo + hi + 1) >> 1;
		if (tab[mid] <= x) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// match finding
// ---------------------------------------------------------------------------------------------------------------------
// chunk bytes back to back (+ LZ_PAD zero bytes), the level-3 keys (frame << 24 | d[i] d[i+1] d[i+2]) in position order,
// the end of each position's frame, and no match yet
__global__ void __launch_bounds__(256) k_lz_gather(const uint8_t* __restrict__ bits, unsigned long long stride,
                                                   const uint32_t* __restrict__ fstart, uint32_t f0, uint32_t nf, uint32_t N,
                                                   uint8_t* __restrict__ cat, uint32_t* __restrict__ fend)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= N + LZ_PAD) return;
	if (i >= N) { cat[i] = 0; return; }
	const uint32_t k = upper_idx(fstart, nf, i);
	cat[i] = bits[(unsigned long long)(f0 + k) * stride + (i - fstart[k])];
	fend[i] = fstart[k + 1];
}

__global__ void __launch_bounds__(256) k_lz_key3(const uint32_t* __restrict__ fstart, uint32_t nf, uint32_t N,
                                                 const uint8_t* __restrict__ cat, uint32_t* __restrict__ key,
                                                 uint32_t* __restrict__ val, uint32_t* __restrict__ res)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	const uint32_t k = upper_idx(fstart, nf, i);
	key[i] = k << 24 | (uint32_t)cat[i] << 16 | (uint32_t)cat[i + 1] << 8 | cat[i + 2];
	val[i] = i;
	res[i] = 0;
}

// level L > 3: (rank of the (L-1)-group << 8 | byte L-1 of the position); grp holds rank + 1
__global__ void __launch_bounds__(256) k_lz_key(uint32_t N, uint32_t L, const uint8_t* __restrict__ cat,
                                                const uint32_t* __restrict__ grp, const uint32_t* __restrict__ val,
                                                uint32_t* __restrict__ key)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	key[i] = (grp[i] - 1u) << 8 | cat[val[i] + L - 1];
}

// group heads of the sorted keys (inclusive-scanned afterwards into rank + 1)
__global__ void __launch_bounds__(256) k_lz_heads(uint32_t N, const uint32_t* __restrict__ key, uint32_t* __restrict__ grp)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	grp[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// entry i of the level-L order: does its L-gram occur earlier in the window?  Then the earliest such occurrence.
// Members of a group are in position order and distinct, so the in-window ones are the <= 65535 entries before i.
__global__ void __launch_bounds__(256) k_lz_query(uint32_t N, uint32_t L, const uint32_t* __restrict__ key,
                                                  const uint32_t* __restrict__ val, const uint32_t* __restrict__ fend,
                                                  uint32_t* __restrict__ res)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= N || i == 0) return;
	const uint32_t k = key[i], pos = val[i];
	const uint32_t lo = pos >= LZ_WIN ? pos - LZ_WIN : 0u;
	if (key[i - 1] != k || val[i - 1] < lo) return;              // (groups never span frames: the frame is in the key)
	if (fend[pos] - pos < L) return;                             // longer than the cap min(15, n - i)
	uint32_t a = i > LZ_WIN ? i - LZ_WIN : 0u, b = i - 1;        // first entry of [a, b] in i's group at >= lo; b qualifies
	for (int it = 0; it < 17 && a < b; it++) {
		const uint32_t m = (a + b) >> 1;
		if (key[m] == k && val[m] >= lo) b = m; else a = m + 1;
	}
	res[pos] = L << 16 | (pos - val[a]);                         // levels run upwards: the last write is L*
}

// ---------------------------------------------------------------------------------------------------------------------
// stable LSD radix sort of (key, value) pairs, 8 bits per pass.  One wave per tile of RS_TILE elements; the rank of an
// element among the equal digits of its round comes from ballots, so the order inside a digit is the input order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_rs_hist(uint32_t N, const uint32_t* __restrict__ key, uint32_t shift,
                                                uint32_t* __restrict__ hist, uint32_t ntiles)
{
	__shared__ uint32_t cnt[256];
	const uint32_t lane = threadIdx.x, t = blockIdx.x;
	for (uint32_t d = lane; d < 256; d += 64) cnt[d] = 0;
	__syncthreads();
	for (uint32_t r = 0; r < RS_TILE / 64; r++) {
		const uint32_t i = t * RS_TILE + r * 64 + lane;
		if (i < N) atomicAdd(&cnt[(key[i] >> shift) & 255u], 1u);
	}
	__syncthreads();
	for (uint32_t d = lane; d < 256; d += 64) hist[d * ntiles + t] = cnt[d];
}

__global__ void __launch_bounds__(64) k_rs_scatter(uint32_t N, const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                   uint32_t* __restrict__ kout, uint32_t* __restrict__ vout, uint32_t shift,
                                                   const uint32_t* __restrict__ offs, uint32_t ntiles)
{
	__shared__ uint32_t cnt[256];
	const uint32_t lane = threadIdx.x, t = blockIdx.x;
	for (uint32_t d = lane; d < 256; d += 64) cnt[d] = offs[d * ntiles + t];
	__syncthreads();
	const unsigned long long below = (1ull << lane) - 1ull;
	for (uint32_t r = 0; r < RS_TILE / 64; r++) {
		const uint32_t i = t * RS_TILE + r * 64 + lane;
		const bool ok = i < N;
		const uint32_t kk = ok ? kin[i] : 0u, vv = ok ? vin[i] : 0u;
		const uint32_t d = (kk >> shift) & 255u;
		unsigned long long peers = __ballot(ok);
#pragma unroll
		for (int b = 0; b < 8; b++) {
			const unsigned long long m = __ballot(ok && ((d >> b) & 1u));
			peers &= ((d >> b) & 1u) ? m : ~m;
		}
		uint32_t base = 0;
		if (ok) base = cnt[d];
		__syncthreads();
		if (ok) {
			const uint32_t dst = base + (uint32_t)__popcll(peers & below);
			kout[dst] = kk;
			vout[dst] = vv;
			if ((peers >> lane) == 1ull) cnt[d] = base + (uint32_t)__popcll(peers);   // the highest lane of the digit
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// in-place scan of n u32 (exclusive or inclusive): block sums, one block scans those, blocks add their offset
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t* sh, uint32_t* total)
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

__global__ void __launch_bounds__(256) k_scan_up(const uint32_t* __restrict__ a, uint32_t n, uint32_t* __restrict__ part)
{
	__shared__ uint32_t sh[256];
	const uint32_t base = blockIdx.x * SC_BLOCK + threadIdx.x * 4;
	uint32_t s = 0;
	for (int k = 0; k < 4; k++) if (base + k < n) s += a[base + k];
	uint32_t tot;
	block_excl_scan_256(s, sh, &tot);
	if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) k_scan_part(uint32_t* __restrict__ part, uint32_t nb)
{
	__shared__ uint32_t sh[256];
	uint32_t carry = 0;
	for (uint32_t b0 = 0; b0 < nb; b0 += 256) {                    // nb <= LZ_CHUNK / SC_BLOCK: <= 64 rounds
		const uint32_t i = b0 + threadIdx.x;
		const uint32_t v = i < nb ? part[i] : 0u;
		uint32_t tot;
		const uint32_t ex = block_excl_scan_256(v, sh, &tot);
		if (i < nb) part[i] = carry + ex;
		carry += tot;
	}
}

template <bool INCL>
__global__ void __launch_bounds__(256) k_scan_down(uint32_t* __restrict__ a, uint32_t n, const uint32_t* __restrict__ part)
{
	__shared__ uint32_t sh[256];
	const uint32_t base = blockIdx.x * SC_BLOCK + threadIdx.x * 4;
	uint32_t v[4], s = 0;
	for (int k = 0; k < 4; k++) { v[k] = base + k < n ? a[base + k] : 0u; s += v[k]; }
	uint32_t tot;
	uint32_t run = part[blockIdx.x] + block_excl_scan_256(s, sh, &tot);
	for (int k = 0; k < 4; k++) {
		if (INCL) run += v[k];
		if (base + k < n) a[base + k] = run;
		if (!INCL) run += v[k];
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// greedy parse and emission
// ---------------------------------------------------------------------------------------------------------------------
struct piece_at { uint32_t start, end; };

__device__ __forceinline__ piece_at piece_of(uint32_t q, const uint32_t* __restrict__ pb, const uint32_t* __restrict__ fstart, uint32_t nf)
{
	const uint32_t k = upper_idx(pb, nf + 1, q);                 // pb[k] <= q < pb[k+1] (frames without pieces are skipped)
	piece_at p;
	p.start = fstart[k] + (q - pb[k]) * LZ_P;
	p.end = min(p.start + LZ_P, fstart[k + 1]);
	return p;
}

// piece q entered at offset e (0..14): exit offset into the next piece and the bits of its tokens
__global__ void __launch_bounds__(256) k_lz_piece(uint32_t npieces, const uint32_t* __restrict__ pb, const uint32_t* __restrict__ fstart,
                                                  uint32_t nf, const uint32_t* __restrict__ res, uint8_t* __restrict__ pexit,
                                                  uint32_t* __restrict__ pbits)
{
	const uint32_t g = blockIdx.x * 256u + threadIdx.x, q = g >> 4, e = g & 15u;
	if (q >= npieces || e >= LZ_MAXLEN) return;
	const piece_at p = piece_of(q, pb, fstart, nf);
	uint32_t x = p.start + e, nb = 0;
	for (uint32_t s = 0; s < LZ_P && x < p.end; s++) {
		const uint32_t len = res[x] >> 16;
		if (len >= 3) { nb += 21; x += len; } else { nb += 9; x += 1; }
	}
	pexit[q * LZ_MAXLEN + e] = (uint8_t)(x > p.end ? x - p.end : 0u);
	pbits[q * LZ_MAXLEN + e] = nb;
}

// one lane per frame: chain the pieces from offset 0, bit offsets of the pieces, csize
__global__ void __launch_bounds__(64) k_lz_fscan(uint32_t nf, const uint32_t* __restrict__ pb, const uint8_t* __restrict__ pexit,
                                                 const uint32_t* __restrict__ pbits, uint8_t* __restrict__ pentry,
                                                 uint32_t* __restrict__ poff, uint32_t* __restrict__ csize)
{
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= nf) return;
	uint32_t e = 0, acc = 0;
	for (uint32_t q = pb[k]; q < pb[k + 1]; q++) {               // <= LZ_CHUNK / LZ_P pieces
		pentry[q] = (uint8_t)e;
		poff[q] = acc;
		acc += pbits[q * LZ_MAXLEN + e];
		e = pexit[q * LZ_MAXLEN + e];
	}
	csize[k] = (uint32_t)((float)acc / 8.0f);                    // in float, as the reference (src/agmv_encode.c:176)
}

__global__ void __launch_bounds__(256) k_lz_emit(uint32_t npieces, const uint32_t* __restrict__ pb, const uint32_t* __restrict__ fstart,
                                                 uint32_t nf, const uint32_t* __restrict__ wb, const uint8_t* __restrict__ cat,
                                                 const uint32_t* __restrict__ res, const uint8_t* __restrict__ pentry,
                                                 const uint32_t* __restrict__ poff, uint32_t* __restrict__ words)
{
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	if (q >= npieces) return;
	const uint32_t k = upper_idx(pb, nf + 1, q);
	const uint32_t start = fstart[k] + (q - pb[k]) * LZ_P, end = min(start + LZ_P, fstart[k + 1]);
	const uint32_t b0 = poff[q];
	uint32_t* w = words + wb[k] + (b0 >> 5);
	const bool shared_first = (b0 & 31u) != 0;
	bool first = true;
	unsigned long long acc = 0;
	uint32_t nacc = b0 & 31u, x = start + pentry[q];
	for (uint32_t s = 0; s < LZ_P && x < end; s++) {
		const uint32_t r = res[x], len = r >> 16;
		if (len >= 3) { acc |= (unsigned long long)(0u | (r & 0xFFFFu) << 1 | len << 17) << nacc; nacc += 21; x += len; }
		else          { acc |= (unsigned long long)(1u | (uint32_t)cat[x] << 1) << nacc; nacc += 9; x += 1; }
		if (nacc >= 32) {
			if (first && shared_first) atomicOr(w, (uint32_t)acc);
			else *w = (uint32_t)acc;
			first = false;
			w++;
			acc >>= 32;
			nacc -= 32;
		}
	}
	if (nacc > (first ? (b0 & 31u) : 0u)) atomicOr(w, (uint32_t)acc);  // the last word may be the next piece's first
}

// csize bytes of frame k into its row of the caller's output
__global__ void __launch_bounds__(256) k_lz_copy(uint32_t f0, const uint32_t* __restrict__ wb, const uint32_t* __restrict__ words,
                                                 const uint32_t* __restrict__ csize, uint8_t* __restrict__ out, unsigned long long out_stride)
{
	const uint32_t k = blockIdx.y, n = csize[f0 + k];
	const uint8_t* src = (const uint8_t*)(words + wb[k]);
	uint8_t* dst = out + (unsigned long long)(f0 + k) * out_stride;
	for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < n; t += gridDim.x * 256u) dst[t] = src[t];
}

// ---------------------------------------------------------------------------------------------------------------------
// work areas (per context, grown on demand)
// ---------------------------------------------------------------------------------------------------------------------
struct lz_ws {
	size_t cap_n;               // positions of a chunk
	uint8_t* cat;               // cap_n + LZ_PAD
	uint32_t *kA, *kB, *vA, *vB, *grp, *res, *fend;
	uint32_t* hist;             // 256 per radix tile, then the scan's block sums
	uint32_t* part;
	size_t cap_pieces;
	uint8_t* pexit;             // 15 per piece
	uint32_t* pbits;            // 15 per piece
	uint8_t* pentry;
	uint32_t* poff;
	size_t cap_words;
	uint32_t* words;
	size_t cap_tab;             // u32 entries of the chunk tables
	uint32_t* tab;
};

static void lz_free(void* p)
{
	lz_ws* w = (lz_ws*)p;
	void* all[] = {w->cat, w->kA, w->kB, w->vA, w->vB, w->grp, w->res, w->fend, w->hist, w->part, w->pexit, w->pbits, w->pentry, w->poff, w->words, w->tab};
	for (void* a : all) if (a) (void)hipFree(a);
	free(w);
}

static int lz_grow(lz_ws* w, uint32_t n, size_t pieces, size_t nwords, size_t ntab)
{
	if (n > w->cap_n) {                                            // one capacity for all of these: committed when all exist
		w->cap_n = 0;
		for (uint32_t** b : {&w->kA, &w->kB, &w->vA, &w->vB, &w->grp, &w->res, &w->fend}) CK(agmv_hip_dev_grow(b, nullptr, n));
		CK(agmv_hip_dev_grow(&w->cat, nullptr, (size_t)n + LZ_PAD));
		CK(agmv_hip_dev_grow(&w->hist, nullptr, ((size_t)n + RS_TILE - 1) / RS_TILE * 256));
		CK(agmv_hip_dev_grow(&w->part, nullptr, (size_t)n / SC_BLOCK + 2));
		w->cap_n = n;
	}
	if (pieces > w->cap_pieces) {
		w->cap_pieces = 0;
		CK(agmv_hip_dev_grow(&w->pexit, nullptr, pieces * LZ_MAXLEN));
		CK(agmv_hip_dev_grow(&w->pbits, nullptr, pieces * LZ_MAXLEN));
		CK(agmv_hip_dev_grow(&w->pentry, nullptr, pieces));
		CK(agmv_hip_dev_grow(&w->poff, nullptr, pieces));
		w->cap_pieces = pieces;
	}
	CK(agmv_hip_dev_grow(&w->words, &w->cap_words, nwords));
	CK(agmv_hip_dev_grow(&w->tab, &w->cap_tab, ntab));
	return 0;
}

static int scan_u32(lz_ws* w, uint32_t* a, uint32_t n, bool inclusive, hipStream_t s)
{
	const uint32_t nb = (n + SC_BLOCK - 1) / SC_BLOCK;
	hipLaunchKernelGGL(k_scan_up, dim3(nb), dim3(256), 0, s, a, n, w->part);
	hipLaunchKernelGGL(k_scan_part, dim3(1), dim3(256), 0, s, w->part, nb);
	if (inclusive) hipLaunchKernelGGL(k_scan_down<true>, dim3(nb), dim3(256), 0, s, a, n, w->part);
	else           hipLaunchKernelGGL(k_scan_down<false>, dim3(nb), dim3(256), 0, s, a, n, w->part);
	CK(hipGetLastError());
	return 0;
}

// stable sort of (key, val) by bits [0, nbits) of the key; returns 1 when the result is in the B buffers
static int radix_sort(lz_ws* w, uint32_t n, uint32_t nbits, bool* in_b, hipStream_t s)
{
	const uint32_t ntiles = (n + RS_TILE - 1) / RS_TILE;
	bool b = false;
	for (uint32_t shift = 0; shift < nbits; shift += 8) {
		uint32_t* ki = b ? w->kB : w->kA; uint32_t* vi = b ? w->vB : w->vA;
		uint32_t* ko = b ? w->kA : w->kB; uint32_t* vo = b ? w->vA : w->vB;
		hipLaunchKernelGGL(k_rs_hist, dim3(ntiles), dim3(64), 0, s, n, ki, shift, w->hist, ntiles);
		CK(hipGetLastError());
		if (scan_u32(w, w->hist, ntiles * 256, false, s)) return -1;
		hipLaunchKernelGGL(k_rs_scatter, dim3(ntiles), dim3(64), 0, s, n, ki, vi, ko, vo, shift, w->hist, ntiles);
		CK(hipGetLastError());
		b = !b;
	}
	*in_b = b;
	return 0;
}

static uint32_t bit_len(uint32_t x) { uint32_t b = 0; while (x) { b++; x >>= 1; } return b; }

extern "C" size_t agmv_hip_lzss_max_csize(size_t n)
{
	return (9 * n + 7) / 8 + 1;     // ceil(9n/8) literal bits, + 1 byte the float csize can add above 2^27 bits
}

extern "C" int agmv_hip_lzss_frames_dev(agmv_hip_ctx* c, const uint8_t* d_bits, size_t bits_stride, const uint32_t* d_sizes,
                                        uint32_t n_frames, uint8_t* d_out, size_t out_stride, uint32_t* d_csize, void* stream)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0) return 0;
	hipStream_t s = (hipStream_t)stream;
	lz_ws* w = (lz_ws*)agmv_hip_area(c, AREA_LZSS, sizeof(lz_ws), lz_free);
	if (!w) return -1;

	// the sizes decide the chunks: read them once
	std::vector<uint32_t> sz(n_frames);
	CK(hipMemcpyAsync(sz.data(), d_sizes, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s));
	CK(hipStreamSynchronize(s));
	for (uint32_t f = 0; f < n_frames; f++) {
		if (sz[f] > bits_stride || sz[f] >= LZ_CHUNK || agmv_hip_lzss_max_csize(sz[f]) > out_stride)
			return agmv_hip_err("agmv_hip_lzss_frames_dev: frame %u: %u bytes (bits_stride %zu, out_stride %zu, at most %u bytes per frame)",
			                    f, sz[f], bits_stride, out_stride, LZ_CHUNK - 1);
	}
	// chunks: [f0, f1) with <= LZ_CHUNK positions and <= LZ_CHUNK_FRAMES frames; per chunk the tables
	//   fstart[nf + 1] (chunk positions), pb[nf + 1] (first piece), wb[nf + 1] (first output word)
	struct chunk { uint32_t f0, nf, n, npieces, nwords; size_t tab; };
	std::vector<chunk> ch;
	std::vector<uint32_t> tab;
	uint32_t maxn = 0; size_t maxp = 0, maxw = 0;
	for (uint32_t f = 0; f < n_frames;) {
		chunk k = {f, 0, 0, 0, 0, tab.size()};
		while (f < n_frames && k.nf < LZ_CHUNK_FRAMES && (uint64_t)k.n + sz[f] <= LZ_CHUNK) { k.n += sz[f]; k.nf++; f++; }
		const size_t t0 = tab.size();
		tab.resize(t0 + 3 * (size_t)(k.nf + 1));
		uint32_t* fs = &tab[t0]; uint32_t* pb = fs + k.nf + 1; uint32_t* wb = pb + k.nf + 1;
		uint32_t at = 0, pc = 0, wc = 0;
		for (uint32_t j = 0; j < k.nf; j++) {
			const uint32_t n = sz[k.f0 + j];
			fs[j] = at; pb[j] = pc; wb[j] = wc;
			at += n; pc += (n + LZ_P - 1) / LZ_P; wc += (uint32_t)((agmv_hip_lzss_max_csize(n) + 3) / 4 + 1);
		}
		fs[k.nf] = at; pb[k.nf] = pc; wb[k.nf] = wc;
		k.npieces = pc; k.nwords = wc;
		if (k.n > maxn) maxn = k.n;
		if (pc > maxp) maxp = pc;
		if (wc > maxw) maxw = wc;
		ch.push_back(k);
	}
	if (lz_grow(w, maxn < RS_TILE ? RS_TILE : maxn, maxp < 1 ? 1 : maxp, maxw < 1 ? 1 : maxw, tab.size())) return -1;
	CK(hipMemcpyAsync(w->tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
	CK(hipStreamSynchronize(s));                                   // (tab is host memory of this call)

	for (const chunk& k : ch) {
		const uint32_t* fs = w->tab + k.tab;
		const uint32_t* pb = fs + k.nf + 1;
		const uint32_t* wb = pb + k.nf + 1;
		const uint32_t N = k.n, gN = (N + 255) / 256;
		if (N) {
			hipLaunchKernelGGL(k_lz_gather, dim3((N + LZ_PAD + 255) / 256), dim3(256), 0, s, d_bits, (unsigned long long)bits_stride,
			                   fs, k.f0, k.nf, N, w->cat, w->fend);
			hipLaunchKernelGGL(k_lz_key3, dim3(gN), dim3(256), 0, s, fs, k.nf, N, w->cat, w->kA, w->vA, w->res);
			CK(hipGetLastError());
			const uint32_t rank_bits = bit_len(N - 1) > 1 ? bit_len(N - 1) : 1;
			for (uint32_t L = 3; L <= LZ_MAXLEN; L++) {
				bool in_b = false;
				if (radix_sort(w, N, L == 3 ? 24 + bit_len(k.nf - 1) : 8 + rank_bits, &in_b, s)) return -1;
				uint32_t* ks = in_b ? w->kB : w->kA; uint32_t* vs = in_b ? w->vB : w->vA;
				hipLaunchKernelGGL(k_lz_query, dim3(gN), dim3(256), 0, s, N, L, ks, vs, w->fend, w->res);
				CK(hipGetLastError());
				if (L == LZ_MAXLEN) break;
				hipLaunchKernelGGL(k_lz_heads, dim3(gN), dim3(256), 0, s, N, ks, w->grp);
				CK(hipGetLastError());
				if (scan_u32(w, w->grp, N, true, s)) return -1;
				// the next level's keys go to the A buffers: its sort starts there
				if (in_b) CK(hipMemcpyAsync(w->vA, w->vB, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
				hipLaunchKernelGGL(k_lz_key, dim3(gN), dim3(256), 0, s, N, L + 1, w->cat, w->grp, w->vA, w->kA);
				CK(hipGetLastError());
			}
		}
		if (k.npieces) {
			hipLaunchKernelGGL(k_lz_piece, dim3((k.npieces * 16 + 255) / 256), dim3(256), 0, s, k.npieces, pb, fs, k.nf, w->res,
			                   w->pexit, w->pbits);
			CK(hipGetLastError());
		}
		hipLaunchKernelGGL(k_lz_fscan, dim3((k.nf + 63) / 64), dim3(64), 0, s, k.nf, pb, w->pexit, w->pbits, w->pentry, w->poff,
		                   d_csize + k.f0);
		CK(hipGetLastError());
		if (k.npieces) {
			CK(hipMemsetAsync(w->words, 0, (size_t)k.nwords * 4, s));
			hipLaunchKernelGGL(k_lz_emit, dim3((k.npieces + 255) / 256), dim3(256), 0, s, k.npieces, pb, fs, k.nf, wb, w->cat, w->res,
			                   w->pentry, w->poff, w->words);
			CK(hipGetLastError());
			uint32_t maxf = 0;
			for (uint32_t j = 0; j < k.nf; j++) if (sz[k.f0 + j] > maxf) maxf = sz[k.f0 + j];
			const uint32_t gx = (uint32_t)((agmv_hip_lzss_max_csize(maxf) + 4095) / 4096);
			hipLaunchKernelGGL(k_lz_copy, dim3(gx < 1 ? 1 : gx, k.nf), dim3(256), 0, s, k.f0, wb, w->words, d_csize, d_out,
			                   (unsigned long long)out_stride);
			CK(hipGetLastError());
		}
	}
	return 0;
}

extern "C" int agmv_hip_lzss_frames(agmv_hip_ctx* c, const uint8_t* h_bits, size_t bits_stride, const uint32_t* h_sizes,
                                    uint32_t n_frames, uint8_t* h_out, size_t out_stride, uint32_t* h_csize)
{
	if (agmv_hip_enter(c)) return -1;
	if (n_frames == 0) return 0;
	uint8_t *db = nullptr, *dout = nullptr;
	uint32_t *ds = nullptr, *dc = nullptr;
	int rc = -1;
	hipError_t e;
	if ((e = hipMalloc((void**)&db, (size_t)n_frames * bits_stride + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&dout, (size_t)n_frames * out_stride + 1)) != hipSuccess ||
	    (e = hipMalloc((void**)&ds, (size_t)n_frames * 4)) != hipSuccess ||
	    (e = hipMalloc((void**)&dc, (size_t)n_frames * 4)) != hipSuccess ||
	    (e = hipMemcpy(db, h_bits, (size_t)n_frames * bits_stride, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = hipMemcpy(ds, h_sizes, (size_t)n_frames * 4, hipMemcpyHostToDevice)) != hipSuccess) {
		agmv_hip_hip_failed("agmv_hip_lzss_frames", e, __FILE_NAME__, __LINE__);
		goto done;
	}
	if (agmv_hip_lzss_frames_dev(c, db, bits_stride, ds, n_frames, dout, out_stride, dc, nullptr)) goto done;
	if ((e = hipDeviceSynchronize()) != hipSuccess ||
	    (e = hipMemcpy(h_csize, dc, (size_t)n_frames * 4, hipMemcpyDeviceToHost)) != hipSuccess) {
		agmv_hip_hip_failed("agmv_hip_lzss_frames", e, __FILE_NAME__, __LINE__);
		goto done;
	}
	for (uint32_t f = 0; f < n_frames; f++)                        // rows: only the payload bytes are defined
		if (h_csize[f] && (e = hipMemcpy(h_out + (size_t)f * out_stride, dout + (size_t)f * out_stride, h_csize[f], hipMemcpyDeviceToHost)) != hipSuccess) {
			agmv_hip_hip_failed("agmv_hip_lzss_frames", e, __FILE_NAME__, __LINE__);
			goto done;
		}
	rc = 0;
done:
	(void)hipFree(db); (void)hipFree(dout); (void)hipFree(ds); (void)hipFree(dc);
	return rc;
}
