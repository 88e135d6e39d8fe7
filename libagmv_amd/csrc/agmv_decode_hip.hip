// libagmv_amd/csrc/agmv_decode_hip.hip -- the decoder of the per-frame hot path: bitstream parsers and block reconstruction
// (include/agmv_hip.h: agmv_hip_parse_frames_dev to agmv_hip_decode_frames).  The encoder, the palette tables and the
// context are in agmv_hip.hip.
//
// What runs where (the reference is cited as file:line):
//   k_parse_serial  block entry positions of a decompressed bitstream (src/agmv_decode.c:224-322), one lane per frame
//   k_parse_*       the same in parallel for any stream: chunk maps, stitched per frame (the robust parser)
//   k_fp_*          the fast parser: speculative walks proven per frame; offsets[] or entry bitmaps + tile entries
//   k_decode        block -> RGB reconstruction (src/agmv_decode.c:249-319, 350-396, 401-405)
//   k_fixup         sequential repair of blocks whose value depends on an earlier GOP
//                   (stale tail after `escape`, src/agmv_decode.c:229-232; last-block FILL
//                   quirk :264-266)
// On the host DEC_LAUNCH is the one place where a run-time flag (the palette's mode; for k_decode / k_fixup the bitmap form;
// for k_decode the looping form) becomes a kernel's template argument.  Integer/byte work only: no MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "agmv_hip_impl.h"

#ifndef DEC_T_OVERRIDE
#define DEC_T_OVERRIDE 256
#endif
constexpr int DEC_T = DEC_T_OVERRIDE;          // threads per decode workgroup
#ifndef DEC_BPB
#define DEC_BPB 24
#endif
constexpr int DEC_STAGE = DEC_T * DEC_BPB;   // LDS window for a tile's bitstream bytes in ONE frame (24 B per block; beyond it bytes come from global memory); x4 frames = 24 KB, 5 workgroups per CU
constexpr int DEC_SR = DEC_STAGE / 4 / DEC_T;   // dwords of the window each lane carries from global memory to LDS
constexpr int DEC_MAX_SLICES = 32;           // agmv_hip_parse_decode_frames_dev: GOP ranges whose parse overlaps the reconstruction of the range before

// the decoder's work area of a context (AREA_DEC): created by the first parse or decode call, freed by agmv_hip_destroy
struct dec_ws {
	uint32_t* d_dirty;              // decode: bitmap of block positions needing the fix-up
	size_t dirty_cap;               // in bytes
	bool dep_split;                 // the last decode call was cut into ranges: its prior dependence is range 0's, whose words are the second set
	uint32_t* d_parse_ws;           // parser workspace: cum | centry | summ
	size_t parse_ws_cap;            // in bytes
	uint32_t* d_fp_ws;              // fast parser workspace: rec | vm | kb | fstate
	size_t fp_ws_cap;               // in bytes
	uint32_t* d_fp_fstate;          // frame states of the last parse (inside d_fp_ws, or d_fstate_call) and how many
	uint32_t fp_frames;
	uint32_t* d_fstate_call;        // agmv_hip_decode_bitstreams_dev cut into ranges: the frame states of the whole call
	size_t fstate_call_cap;         // in bytes
	uint32_t* d_nent_own;           // agmv_hip_decode_bitstreams_dev without a caller's nentered[]
	size_t nent_cap;                // in bytes
	hipStream_t aux_stream;         // decode pipeline: the parser's stream (the reconstruction runs on the caller's)
	hipEvent_t ev_fork;             // ... caller's stream -> parser's stream
	hipEvent_t ev_slice[DEC_MAX_SLICES];   // ... slice parsed
};

static dec_ws* dec_area(agmv_hip_ctx* c) { return (dec_ws*)c->ws[AREA_DEC]; }

static void dec_free(void* p)                                 // (device of the context is current)
{
	dec_ws* d = (dec_ws*)p;
	(void)hipFree(d->d_dirty); (void)hipFree(d->d_parse_ws); (void)hipFree(d->d_fp_ws); (void)hipFree(d->d_nent_own);
	(void)hipFree(d->d_fstate_call);
	if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
	for (int i = 0; i < DEC_MAX_SLICES; i++) if (d->ev_slice[i]) (void)hipEventDestroy(d->ev_slice[i]);
	if (d->aux_stream) (void)hipStreamDestroy(d->aux_stream);
	free(d);
}

// palette: the call parses or decodes -- a palette must be set, and the context has its work area afterwards
static int need_dec_ctx(agmv_hip_ctx* c, bool palette)
{
	if (agmv_hip_enter(c, palette)) return -1;
	return palette && !agmv_hip_area(c, AREA_DEC, sizeof(dec_ws), dec_free) ? -1 : 0;
}

// f(std::bool_constant<flag>()...): every run-time flag becomes a compile-time one
template <class F>
static void dec_flags(F&& f) { f(); }
template <class F, class... Rest>
static void dec_flags(F&& f, bool flag, Rest... rest) { dec_flags([&](auto... r_) { if (flag) f(std::true_type(), r_...); else f(std::false_type(), r_...); }, rest...); }
// launch k<flags...> on stream s, then check the launch
#define DEC_LAUNCH(k, grid, block, s, A, ...) do { \
	dec_flags([&](auto... b_) { hipLaunchKernelGGL((k<decltype(b_)::value...>), grid, block, 0, s, A); }, __VA_ARGS__); \
	CK(hipGetLastError()); } while (0)

// ----------------------------------------------------------------------------------------------
// decode side
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_flag(uint32_t b) { return b == FILL_FLAG || b == NORMAL_FLAG || b == COPY_FLAG; }

struct ByteSrc {
	const uint8_t* p;
	uint32_t cap;
	__device__ __forceinline__ uint32_t operator()(uint32_t pos) const { return pos < cap ? p[pos] : 0u; }
};

// bytes of one frame read through an LDS window [lo, lo+len) staged by the workgroup; anything outside falls back to
// global memory (streams full of resync garbage can make a tile's byte range larger than the window)
struct StagedSrc {
	const __attribute__((address_space(3))) uint8_t* lds;      // explicit LDS pointer: ds_read_u8, never flat_load
	uint32_t lo, len;
	const uint8_t* p;
	uint32_t cap;
	__device__ __forceinline__ uint32_t operator()(uint32_t pos) const
	{
		const uint32_t d = pos - lo;
		if (d < len) return lds[d];
		return pos < cap ? p[pos] : 0u;
	}
};

// K2 (serial form): one lane walks one frame's bitstream exactly like the reference's block loop
// (src/agmv_decode.c:226-320 / 327-397) but only records where each block is entered.
__global__ __launch_bounds__(64) void k_parse_serial(const uint8_t* __restrict__ bits, unsigned long long stride,
                                                     const uint32_t* __restrict__ bpos_a, uint32_t n_frames,
                                                     uint32_t nblk, int mode512, uint32_t* __restrict__ offsets,
                                                     uint32_t* __restrict__ nentered)
{
	uint32_t f = blockIdx.x * 64u + threadIdx.x;
	if (f >= n_frames) return;
	ByteSrc src{bits + (size_t)f * stride, (uint32_t)stride};
	const uint32_t bpos = bpos_a[f];
	uint32_t* off = offsets + (size_t)f * nblk;
	uint32_t bitpos = 0, k = 0;
	bool escape = false;
	while (k < nblk && !escape) {
		if (bitpos > bpos) break;
		off[k++] = bitpos;
		uint32_t byte = src(bitpos++);
		bool invalid = false;
		while (!is_flag(byte)) {
			byte = src(bitpos++);
			if (bitpos > bpos) { escape = true; break; }
		}
		if (!is_flag(byte)) invalid = true;
		if (byte == FILL_FLAG) {
			uint32_t idx = src(bitpos++);
			if (mode512 && (idx & 0x7fu) == 127u) bitpos++;
			if (bitpos > bpos) escape = true;
		} else if (byte == COPY_FLAG) {
		} else {
			for (int j = 0; j < 4; j++)
				for (int i = 0; i < 4; i++) {
					uint32_t idx = src(bitpos++);
					if (mode512 && (idx & 0x7fu) == 127u) bitpos++;
					if (bitpos > bpos || invalid) { escape = true; invalid = false; break; }
				}
		}
	}
	nentered[f] = k;
}

// ----------------------------------------------------------------------------------------------
// K2 (parallel form).  The block loop of the reference (src/agmv_decode.c:226-320) is a chain:
// block k+1 is entered where block k ended, and an entry position that does not hold a flag byte
// slides forward to the next flag-valued byte (the resync of :236-243).  So the only positions
// that can start a block are the flag-valued bytes: the NODES.  A node at p ends at
//   COPY   -> p+1        FILL -> p+2 (+1 after an escape code, 512 colours)
//   NORMAL -> 16 codes of 1 or 2 bytes after p+1
// and its successor is the first node at or after that end.  next(p)-p <= 33, so a chunk of PC
// bytes is summarised by a map {entry offset 0..32} -> (exit offset, blocks counted).
// k_parse_chunks (one WAVE per chunk, no workgroup barriers): flags are found with ballots, ranked
// with popcounts into a dense node list, each node's end is computed by one lane, and the chain
// is resolved by pointer doubling over the node list -- the work is proportional to the number
// of blocks in the chunk, not to its bytes.  One wave per frame then threads the chunk maps
// together (k_parse_stitch), and k_parse_emit rebuilds the node list, marks the nodes of the
// true chain (three doubling levels + a walk in steps of 8 nodes) and writes the entry offsets,
// a node's block number being the popcount of marked nodes before it.
// ----------------------------------------------------------------------------------------------
constexpr int PC = 512;         // bytes per chunk (one wave)
constexpr int PNSEG = PC / 64;  // ballot segments per chunk
#ifndef PEL_OVERRIDE
#define PEL_OVERRIDE 3
#endif
constexpr int PCL = 3;          // k_parse_chunks: doubling rounds before the 33 entry lanes walk 2^PCL nodes at a time
constexpr int PEL = PEL_OVERRIDE;   // k_parse_emit: levels kept for marking; the chain is walked 2^PEL nodes at a time
constexpr int PHALO = 64;       // bytes staged beyond the chunk (a block spans <= 33)
constexpr uint32_t J_EXIT = 0x8000u;    // jump leaves the chunk: J_EXIT | offset into the next chunk
constexpr uint32_t J_END = 0xFFFFu;     // chain left the readable stream (position > bpos)
constexpr uint32_t X_END = 63u;         // chunk map: exit code of an ended chain

// geometry of the fast parser (k_fp_*, below); the robust kernels can deliver their result in its bitmap form
constexpr int FC = 64;                  // bytes per piece (one lane)
constexpr int FH = 4;                   // run-in pieces
constexpr int FOWN = 64 - FH - 1;       // pieces a region owns (lane 63 holds the piece behind it)
constexpr int FRB = FOWN * FC;          // bytes a region owns

struct ParseArgs {
	const uint8_t* bits;
	unsigned long long stride;
	const uint32_t* bpos;
	uint32_t cpf;           // chunk rows per frame in summ / centry (the worst case: frame f's chunk c is row f * cpf + c -- no prefix over the frames, no launch for one)
	uint16_t* summ;         // [chunk][33] exit<<10 | count   (exit X_END: chain ended in the chunk)
	uint32_t* centry;       // [chunk] kbase<<8 | entry offset (0xff: chain never reaches the chunk)
	uint32_t* offsets;
	uint32_t* nentered;
	uint32_t n_frames, nblk;
	const uint32_t* fstate; // != NULL: only the frames the fast path gave up on (fstate[f] == FS_BAD) are parsed here
	const uint32_t* nbad;   // != NULL: how many frames are FS_BAD (0: every kernel of this path returns at once, without a look at the frames)
	unsigned long long* vm; // != NULL: the result goes out as entry BITS (the fast parser's bitmaps, [frame][maxR * FOWN] words of 64 bytes of stream) instead of offsets[]
	uint32_t maxR;
};
constexpr uint32_t FS_OK = 0, FS_TODO = 1, FS_BAD = 2;

// chunks of frame f that the robust kernels parse: ceil((bpos + 1) / PC), or none when the frame is not theirs
__device__ __forceinline__ uint32_t parse_nch(const ParseArgs& A, uint32_t f, uint32_t bpos)
{
	return (!A.fstate || A.fstate[f] == FS_BAD) ? (bpos + PC) / PC : 0u;
}

__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// LDS of one wave's chunk.  NLV jump tables: 2 (ping-pong, k_parse_chunks) or PEL+1 (kept levels, k_parse_emit).
// The two tables that only the node build needs (rank_at: position -> nodes before it = index of the first node at
// or after it; npos: node -> position) are not members: the caller lends them the space of tables that are first
// written after the build (4.75 KB / 5.75 KB per wave instead of 6.8 / 8.3: 33 / 27 waves per CU instead of 23 / 19).
template <int NLV>
struct ParseLds {
	uint8_t b[PC + PHALO];                  // staged bytes
	unsigned long long esc[PNSEG + 2];      // per 64 bytes (chunk + halo): which bytes are escape codes ((b & 0x7f) == 127)
	uint16_t jl[NLV][PC];                   // node -> jump target (node index | J_EXIT+offset | J_END)
};

constexpr int PCD = ((PC + PHALO) / 4 + 63) / 64;      // dwords of a chunk (+halo) per lane

// the chunk's bytes, dword-wide (cs and the slab stride are multiples of 4); bytes past the slab read as 0
__device__ __forceinline__ void load_chunk(uint32_t (&raw)[PCD], const uint8_t* fbits, uint32_t cap, uint32_t cs, int lane)
{
#pragma unroll
	for (int q = 0; q < PCD; q++) {
		const uint32_t pos = cs + 4u * (uint32_t)(q * 64 + lane);
		raw[q] = (q * 64 + lane < (PC + PHALO) / 4 && pos < cap) ? *(const uint32_t*)(fbits + pos) : 0u;
	}
}

// Build the node list of chunk [cs, cs+PC): rank_at, npos, and per node the end of its block (eo, bit 15 = the
// block counts, i.e. the next one starts inside the stream) and its successor (jl[0]).  Returns the node count.
template <bool M512, int NLV>
__device__ __forceinline__ uint32_t parse_chunk_nodes(ParseLds<NLV>& S, uint16_t* rank_at, uint16_t* npos, uint16_t* eo, uint16_t* n0,
                                                      const uint32_t (&raw)[PCD], uint32_t bpos, uint32_t cs, int lane)
{
	// ---- stage the chunk (+halo) the caller fetched (load_chunk) while the previous chunk was being parsed
#pragma unroll
	for (int q = 0; q < PCD; q++) {
		const int i = q * 64 + lane;
		if (i < (PC + PHALO) / 4) ((uint32_t*)S.b)[i] = raw[q];
	}
	wave_lds_sync();
	// ---- nodes = flag-valued bytes at positions <= bpos, ranked by ballot + popcount
	uint32_t mtot = 0, by[PNSEG];
#pragma unroll
	for (int sg = 0; sg < PNSEG; sg++) by[sg] = S.b[sg * 64 + lane];
#pragma unroll
	for (int sg = 0; sg < PNSEG; sg++) {
		const uint32_t p = sg * 64 + lane;
		const bool node = is_flag(by[sg]) && cs + p <= bpos;
		const unsigned long long m = __ballot(node);
		const uint32_t r = mtot + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
		rank_at[p] = (uint16_t)r;
		if (node) npos[r] = (uint16_t)p;
		mtot += (uint32_t)__popcll(m);
		if (M512) {
			const unsigned long long em = __ballot((by[sg] & 0x7fu) == 127u);
			if (lane == 0) S.esc[sg] = em;
		}
	}
	if (M512) {
		const unsigned long long em = __ballot((S.b[PC + lane] & 0x7fu) == 127u);    // the halo
		if (lane == 0) { S.esc[PNSEG] = em; S.esc[PNSEG + 1] = 0; }
	}
	wave_lds_sync();
	// ---- one lane per node: where its block ends, and the node that follows
	const bool more = cs + PC <= bpos;                         // the stream continues into the next chunk
	for (uint32_t k = lane; k < mtot; k += 64) {
		const uint32_t p = npos[k], byte = S.b[p];
		uint32_t e = p + 1u;
		if (byte == FILL_FLAG) e += M512 ? 1u + ((S.b[p + 1] & 0x7fu) == 127u ? 1u : 0u) : 1u;
		else if (byte == NORMAL_FLAG) {
			if (M512) {
				// 16 codes of 1 or 2 bytes: the escape bits of the 32 bytes behind the flag, walked in registers
				const uint32_t sg = e >> 6, sh = e & 63u;
				const unsigned long long lo = S.esc[sg], hi = S.esc[sg + 1];
				const uint32_t m = (uint32_t)(sh ? (lo >> sh) | (hi << (64u - sh)) : lo);
				uint32_t pos = 0;
#pragma unroll
				for (int i = 0; i < 16; i++) pos += 1u + ((m >> pos) & 1u);
				e += pos;
			} else e += 16u;
		}
		uint32_t j = J_END, n = 0;
		if (cs + e <= bpos) {                                  // block k+1 starts inside the stream: this one counts
			n = 1;
			if (e >= (uint32_t)PC) j = J_EXIT | (e - PC);
			else {
				const uint32_t nx = rank_at[e];                    // a non-flag entry slides to the next node (:236-243)
				j = nx < mtot ? nx : (more ? J_EXIT : J_END);
			}
		}
		S.jl[0][k] = (uint16_t)j;
		if (eo) eo[k] = (uint16_t)(e | n << 15);
		if (n0) n0[k] = (uint16_t)n;
	}
	wave_lds_sync();
	return mtot;
}

template <bool M512>
__global__ __launch_bounds__(64) void k_parse_chunks(ParseArgs A)
{
	__shared__ ParseLds<2> S;
	__shared__ uint16_t nn[2][PC];                             // node -> blocks counted along its jump (ping-pong)
	const int lane = threadIdx.x;
	if (A.nbad && *A.nbad == 0) return;
	// 2-D grid: y strides over frames, x over the chunks of a frame (no search for the frame of a chunk)
	for (uint32_t f = blockIdx.y; f < A.n_frames; f += gridDim.y) {
	const uint32_t bpos = A.bpos[f], g0 = f * A.cpf, nch = parse_nch(A, f, bpos);
	const uint8_t* fbits = A.bits + (size_t)f * A.stride;
	uint32_t nxt[PCD];
	if (blockIdx.x < nch) load_chunk(nxt, fbits, (uint32_t)A.stride, blockIdx.x * PC, lane);
	for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
		const uint32_t g = g0 + c, cs = c * PC;
		uint32_t raw[PCD];
#pragma unroll
		for (int q = 0; q < PCD; q++) raw[q] = nxt[q];
		if (c + gridDim.x < nch) load_chunk(nxt, fbits, (uint32_t)A.stride, (c + gridDim.x) * PC, lane);   // in flight over this chunk
		if (A.vm && lane < PC / 64) A.vm[(size_t)f * A.maxR * FOWN + c * (PC / 64) + lane] = 0ull;   // k_parse_emit ORs the entry bits in (a later launch); FOWN words per region, linear in the byte position
		const uint32_t mtot = parse_chunk_nodes<M512>(S, /*rank_at*/ nn[1], /*npos*/ S.jl[1], nullptr, nn[0], raw, bpos, cs, lane);
		const uint32_t k0 = lane < 33 ? nn[1][lane] : 0u;         // first node at or after entry offset `lane` (rank_at dies below)
		wave_lds_sync();
		// ---- PCL rounds of pointer doubling over the node list (jump + blocks counted along it), then the 33 entry
		// lanes walk their chains 2^PCL nodes at a time
#pragma unroll
		for (int lv = 0; lv < PCL; lv++) {
			const uint16_t *js = S.jl[lv & 1], *ns = nn[lv & 1];
			uint16_t *jd = S.jl[(lv + 1) & 1], *nd = nn[(lv + 1) & 1];
			for (uint32_t k = lane; k < mtot; k += 64) {
				uint32_t j = js[k], n = ns[k];
				if (j < J_EXIT) { n += ns[j]; j = js[j]; }
				jd[k] = (uint16_t)j;
				nd[k] = (uint16_t)n;
			}
			wave_lds_sync();
		}
		if (lane < 33) {
			uint32_t ex = X_END, cnt = 0;
			if (cs + lane <= bpos) {
				uint32_t k = k0;
				if (k >= mtot) { if (cs + PC <= bpos) ex = 0; }
				else {
					const uint16_t *jf = S.jl[PCL & 1], *nf = nn[PCL & 1];
					do { cnt += nf[k]; k = jf[k]; } while (k < J_EXIT);
					if (k != J_END) ex = k & 0x3Fu;
				}
			}
			A.summ[(size_t)g * 33 + lane] = (uint16_t)(ex << 10 | cnt);
		}
		wave_lds_sync();
	}
	}
}

// one wave per frame: thread the chunk maps together.  Rows are fetched a batch of 32 chunks ahead (lane j holds
// map[j]; unconditional clamped loads so that a whole batch is in flight while the previous one is consumed); the
// chain state (entry offset, blocks so far) is wave-uniform, so the dependent step is a v_readlane and scalar
// arithmetic, not a memory access.
constexpr int PSB = 32;
__global__ __launch_bounds__(64) void k_parse_stitch(ParseArgs A)
{
	const int lane = threadIdx.x;
	if (A.nbad && *A.nbad == 0) return;
	for (uint32_t f = blockIdx.x; f < A.n_frames; f += gridDim.x) {
	const uint32_t c0 = f * A.cpf, nch = parse_nch(A, f, A.bpos[f]);     // nch >= 1 for a frame that is parsed here
	if (nch == 0) continue;
	const uint16_t* rows = A.summ + (size_t)c0 * 33 + (lane < 33 ? lane : 0);
	uint32_t o = 0, kb = 0;
	uint32_t nxt[PSB];
#pragma unroll
	for (int u = 0; u < PSB; u++) nxt[u] = rows[(size_t)min((uint32_t)u, nch - 1u) * 33];
	for (uint32_t c = 0; c < nch; c += PSB) {
		uint32_t row[PSB];
#pragma unroll
		for (int u = 0; u < PSB; u++) row[u] = nxt[u];
#pragma unroll
		for (int u = 0; u < PSB; u++) nxt[u] = rows[(size_t)min(c + PSB + u, nch - 1u) * 33];
		uint32_t mine = 0;                                     // lane u: centry of chunk c+u
#pragma unroll
		for (int u = 0; u < PSB; u++) {
			if (lane == u) mine = kb << 8 | o;
			if (c + u < nch && o != 0xFFu) {
				const uint32_t v = __builtin_amdgcn_readlane(row[u], __builtin_amdgcn_readfirstlane(o));
				kb += v & 0x3FFu;
				o = (v >> 10) == X_END ? 0xFFu : v >> 10;
			}
		}
		if (lane < PSB && c + lane < nch) A.centry[c0 + c + lane] = mine;
	}
	if (lane == 0) A.nentered[f] = min(A.nblk, kb + 1u);
	}
}

template <bool M512>
__global__ __launch_bounds__(64) void k_parse_emit(ParseArgs A)
{
	__shared__ ParseLds<PEL + 1> S;
	__shared__ uint16_t eo[PC];                                // node -> end of its block (chunk-relative, <= PC+32) | counts << 15
	uint8_t* mark = S.b;                                       // chain marks: in the staged bytes' space once the nodes are built
	static_assert(PEL >= 2 && PC + PHALO >= PC, "rank_at / npos borrow jl[PEL-1] / jl[PEL], the marks borrow the bytes");
	const int lane = threadIdx.x;
	if (A.nbad && *A.nbad == 0) return;
	for (uint32_t f = blockIdx.y; f < A.n_frames; f += gridDim.y) {
	const uint32_t bpos = A.bpos[f], g0 = f * A.cpf, nch = parse_nch(A, f, bpos);
	const uint8_t* fbits = A.bits + (size_t)f * A.stride;
	uint32_t* off = A.offsets + (size_t)f * A.nblk;
	uint32_t nxt[PCD], ce_n = 0;
	if (blockIdx.x < nch) { ce_n = A.centry[g0 + blockIdx.x]; load_chunk(nxt, fbits, (uint32_t)A.stride, blockIdx.x * PC, lane); }
	for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
		const uint32_t ce = ce_n, o = ce & 0xFFu, kb = ce >> 8;
		uint32_t raw[PCD];
#pragma unroll
		for (int q = 0; q < PCD; q++) raw[q] = nxt[q];
		if (c + gridDim.x < nch) {                             // next chunk: in flight over this one
			ce_n = A.centry[g0 + c + gridDim.x];
			load_chunk(nxt, fbits, (uint32_t)A.stride, (c + gridDim.x) * PC, lane);
		}
		unsigned long long* fvm = A.vm ? A.vm + (size_t)f * A.maxR * FOWN : nullptr;
		if (c == 0 && lane == 0) {                             // block 0 is entered at byte 0
			if (fvm) atomicOr(fvm, 1ull); else off[0] = 0;
		}
		if (o == 0xFFu) continue;                              // the chain ended before this chunk (uniform)
		if (kb + 1u >= A.nblk) continue;                       // every block this chunk could enter is beyond the frame
		const uint32_t cs = c * PC;
		const uint32_t mtot = parse_chunk_nodes<M512>(S, /*rank_at*/ S.jl[PEL - 1], /*npos*/ S.jl[PEL], eo, nullptr, raw, bpos, cs, lane);
		const uint32_t k0 = cs + o <= bpos ? S.jl[PEL - 1][o] : mtot;
		for (uint32_t k = lane; k < mtot; k += 64) mark[k] = 0;
		wave_lds_sync();
		if (k0 < mtot) {
			// PEL rounds of pointer doubling, then one lane walks the true chain 2^PEL nodes at a time and the kept
			// levels fill in the nodes between (every node 2^lv steps behind a marked one)
#pragma unroll
			for (int lv = 0; lv < PEL; lv++) {
				for (uint32_t k = lane; k < mtot; k += 64) {
					uint32_t j = S.jl[lv][k];
					if (j < J_EXIT) j = S.jl[lv][j];
					S.jl[lv + 1][k] = (uint16_t)j;
				}
				wave_lds_sync();
			}
			if (lane == 0)
				for (uint32_t k = k0; k < J_EXIT; k = S.jl[PEL][k]) mark[k] = 1;
			wave_lds_sync();
#pragma unroll
			for (int lv = PEL - 1; lv >= 0; lv--) {
				for (uint32_t k = lane; k < mtot; k += 64) {
					const uint32_t j = S.jl[lv][k];
					if (mark[k] && j < J_EXIT) mark[j] = 1;
				}
				wave_lds_sync();
			}
			// nodes are in stream order, so a counting node's rank on the chain is the number of marked counting
			// nodes before it; it is block kb+rank and ends where block kb+rank+1 is entered
			uint32_t base = kb + 1u;
			for (uint32_t kg = 0; kg < mtot; kg += 64) {
				const uint32_t k = kg + lane;
				const uint32_t ev = k < mtot ? eo[k] : 0u;
				const bool on = k < mtot && mark[k] && (ev & 0x8000u);
				const unsigned long long m = __ballot(on);
				const uint32_t kk = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
				if (on && kk < A.nblk) {
					const uint32_t pos = cs + (ev & 0x7FFFu);
					if (fvm) atomicOr(fvm + (pos >> 6), 1ull << (pos & 63u)); else off[kk] = pos;
				}
				base += (uint32_t)__popcll(m);
			}
		}
		wave_lds_sync();
	}
	}
}

// ----------------------------------------------------------------------------------------------
// K2 (fast form): speculate, then PROVE.  The chain of block entries of a frame is unique: if a set of walks, one per
// 64-byte piece of the stream, is such that every walk starts exactly where the walk of the piece before left off and
// the first one starts at byte 0, their concatenation IS the reference's parse.  Chains that start at different bytes
// merge within a few blocks (every block start the true chain passes is a flag byte the other chain will usually hit),
// so a lane that walks its piece from "the first flag byte of the piece" almost always ends where the true chain ends:
//   k_fp_walk   one wave per REGION of 59 pieces (+4 pieces of run-in before it, +1 behind it for the spill of the
//               last block).  Every lane walks its piece from the first flag byte (types and lengths from bit masks
//               built once per piece: flag bytes F, COPY bytes C, two-byte FILLs L, escape codes E; a step takes a whole
//               run of COPYs or of two-byte FILLs; NORMAL lengths are computed for many lanes at once).  Then each lane
//               takes the exit of the lane before it as its true entry: if that entry slides onto a node of the walk it
//               already has, the walk is trimmed; otherwise it walks from there until it hits a node of the old walk
//               (merge) or leaves the piece.  Repeated until no lane's exit changes (1-2 rounds).
//               Per piece: the bitmap V of block ENTRY positions (what offsets[] holds); per region: E (exit of the
//               run-in = assumed entry of the region), X (exit of its last piece), N (entries).
//   k_fp_finish one wave per frame: region r is proven when E[r] == X[r-1] (region 0 starts at byte 0 by definition).
//               Regions that are not are walked again, in order, with X[r-1] as a FORCED entry (an exit that changes
//               carries on into the next region); a frame that needs more than FP_REPAIRS of those is left to the robust
//               parser above.  Proven frames: exclusive sums of N -> first block number of every region, nentered.
//   k_fp_expand bitmaps -> offsets[]: per piece, the lanes whose bit is set write their position at the rank of the bit.
// Exit / entry codes: 0..33 = the next block is entered at that byte of the next piece; FX_SLIDE = no new entry, the
// resync (src/agmv_decode.c:236-243) continues into the next piece; FX_END = the chain ended.
// ----------------------------------------------------------------------------------------------
constexpr int FROW = FC / 4 + 1;        // LDS dwords per piece (odd stride: no bank conflicts between the lanes' pieces)
constexpr uint32_t FX_SLIDE = 64u, FX_END = 65u, FX_UNSET = 66u, FX_MERGE = 128u;
constexpr int FP_REPAIRS = 24;          // regions of one frame walked again (serially, by the frame's wave) before the frame is given up
constexpr int FP_LDS = 64 * FROW + 1;   // (+1: lane 63's look at "the piece behind" stays inside)

struct FpArgs {
	const uint8_t* bits;
	unsigned long long stride;
	const uint32_t* bpos;
	uint4* rec;                 // [n_frames][maxR]  x = E, y = X, z = N
	unsigned long long* vm;     // [n_frames][maxR][FOWN] entry bitmaps
	uint32_t* kb;               // [n_frames][maxR] first block number of the region
	uint32_t* fstate;           // [n_frames] FS_OK / FS_BAD
	uint32_t* offsets;
	uint32_t* nentered;
	uint32_t n_frames, nblk, maxR;
	uint32_t* nbad;             // frames given up (FS_BAD), counted by k_fp_finish
	uint32_t* tidx;             // [n_frames][tpfd + 1] byte position at which the first block of every k_decode tile is entered (TIDX_NONE: not entered)
	uint32_t tpfd;              // k_decode tiles per frame
	uint32_t* dirty;            // != NULL: k_decode's repair bitmap, cleared by k_fp_tiles (the last parser launch in front of it)
	uint32_t ndirty;
};
constexpr uint32_t TIDX_NONE = 0xFFFFFFFFu;

// buffer descriptor from wave-uniform inputs, made PROVABLY uniform (readfirstlane on both pointer halves and the size): otherwise
// hipcc wraps every buffer op in a waterfall loop
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* p, uint32_t bytes)
{
	const uint64_t a = (uint64_t)p;
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
	return __builtin_amdgcn_make_buffer_rsrc((void*)((uint64_t)hi << 32 | lo), 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

__device__ __forceinline__ uint32_t ctz64(unsigned long long m) { return (uint32_t)__builtin_ctzll(m); }       // m != 0
__device__ __forceinline__ unsigned long long above(uint32_t q) { return (~0ull << q) << 1; }     // bits > q (q <= 63)

// one region (see above) by one wave; forced = FX_UNSET: the entry of the region is what the run-in pieces give
template <bool M512>
__device__ __forceinline__ void fp_walk_region(const FpArgs& A, uint32_t* s_b, uint32_t f, uint32_t r, uint32_t forced, uint32_t bpos, int lane)
{
	const uint8_t* fbits = A.bits + (size_t)f * A.stride;
	const uint32_t cap = (uint32_t)A.stride;
	// ---- stage the 64 pieces (run-in, own, one behind); bytes before the frame or past the slab read as 0
	const long sb = (long)r * FRB - FH * FC;
	uint32_t raw[16];
	{
		// The range check is the buffer descriptor's, not the lanes': the resource is the frame's row, cap bytes of it (a multiple
		// of 4, and so is every offset: a dword in range lies wholly inside).  A dword at or past cap reads 0 and fetches nothing;
		// a row never sees its neighbour's bytes.  Only region 0 has bytes in front of the row (sb = -FH * FC: exactly the 64
		// dwords of k = 0): their offsets, 0xFFFFFF00 .. 0xFFFFFFFC, are >= the resource's size for any stride below 4 GB - 256,
		// so they read 0.  No offset relies on wrapping around 2^32: o1 < stride + 2 FRB and o1 + 3584 stay far below it,
		// whether or not the compiler folds the constant 256 (k - 1) into the instruction.
		const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(fbits, cap & ~3u);
		const uint32_t o0 = (sb < 0 ? 0xFFFFFF00u : (uint32_t)sb) + 4u * (uint32_t)lane;   // (sb is uniform: a scalar select)
		const uint32_t o1 = (uint32_t)(sb + FH * FC) + 4u * (uint32_t)lane;
		raw[0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, o0, 0, 0);
#pragma unroll
		for (int k = 1; k < 16; k++) raw[k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, o1 + 256u * (uint32_t)(k - 1), 0, 0);
	}
	{
		// dword i = 64 k + lane of the span is dword j = lane & 15 of piece 4 k + (lane >> 4): one base address + constants
		uint32_t* row = s_b + (lane >> 4) * FROW + (lane & 15);
#pragma unroll
		for (int k = 0; k < 16; k++) row[k * 4 * FROW] = raw[k];
	}
	wave_lds_sync();
	// ---- this lane's piece as bit masks, four bytes at a time: F flag bytes, C = 0x5E, L = 0x4E, E escape codes
	const long cb = sb + (long)lane * FC;                      // first byte of the piece
	unsigned long long F, C, L, E = 0;
	{
		// bit 7 of every byte that is 0 (exact per byte)
		auto zero7 = [](uint32_t v) -> uint32_t { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u; };
		// the four bits (bit 7 of each byte) of two dwords as one byte: a dot product of the bytes {0, 0x80} with the weights
		// 1, 2, 4, 8 / 16, 32, 64, 128 is 128 x that byte (v_dot4_u32_u8: two instructions where shifts and ors take a dozen).
		// FILL (0x4E) and COPY (0x5E) differ in bit 4 only: one zero test finds both, bit 4 tells them apart; the packed byte of a
		// pair of dwords comes out of the dot products times 128 and goes to its place with ONE shift
		uint32_t f2[2] = {0, 0}, c2[2] = {0, 0}, lc2[2] = {0, 0}, e2[2] = {0, 0};
		auto place = [](uint32_t acc, uint32_t x128, int sh) -> uint32_t { return acc | (sh == 0 ? x128 >> 7 : x128 << (sh - 7)); };
		auto pair128 = [](uint32_t z0, uint32_t z1) -> uint32_t {
			return __builtin_amdgcn_udot4(z1, 0x80402010u, __builtin_amdgcn_udot4(z0, 0x08040201u, 0u, false), false);
		};
#pragma unroll
		for (int j = 0; j < 16; j += 2) {
			const uint32_t w0 = s_b[lane * FROW + j], w1 = s_b[lane * FROW + j + 1];
			const uint32_t zlc0 = zero7((w0 | 0x10101010u) ^ 0x5E5E5E5Eu), zn0 = zero7(w0 ^ 0x2F2F2F2Fu);
			const uint32_t zlc1 = zero7((w1 | 0x10101010u) ^ 0x5E5E5E5Eu), zn1 = zero7(w1 ^ 0x2F2F2F2Fu);
			const int h = j >> 3, sh = 4 * (j & 7);
			lc2[h] = place(lc2[h], pair128(zlc0, zlc1), sh);
			c2[h] = place(c2[h], pair128(zlc0 & (w0 << 3), zlc1 & (w1 << 3)), sh);
			f2[h] = place(f2[h], pair128(zlc0 | zn0, zlc1 | zn1), sh);
			if (M512) e2[h] = place(e2[h], pair128(((w0 & 0x7F7F7F7Fu) + 0x01010101u) & 0x80808080u, ((w1 & 0x7F7F7F7Fu) + 0x01010101u) & 0x80808080u), sh);   // (byte & 0x7f) == 127
		}
		F = (unsigned long long)f2[1] << 32 | f2[0]; C = (unsigned long long)c2[1] << 32 | c2[0];
		L = ((unsigned long long)lc2[1] << 32 | lc2[0]) ^ C; E = (unsigned long long)e2[1] << 32 | e2[0];
	}
	const long lim_l = (long)bpos - cb;                        // a block of this piece counts when it ends at or before this offset
	const int lim = lim_l > 1000 ? 1000 : (lim_l < -1000 ? -1000 : (int)lim_l);
	unsigned long long safe;                                   // positions at which any COPY / FILL ends at or before bpos
	{
		const long nv = lim_l + 1;                             // bytes of the piece at positions <= bpos: only those are nodes
		const unsigned long long ok = nv <= 0 ? 0ull : (nv < 64 ? (1ull << nv) - 1ull : ~0ull);
		F &= ok;
		safe = ok >> 3;
	}
	const bool more = lim >= FC;                               // the stream goes on behind this piece
	unsigned long long En = 0;                                 // escape codes of the piece behind (a NORMAL body spills <= 33 bytes)
	unsigned long long D;
	{
		unsigned long long L3 = 0;                             // FILLs whose index byte is an escape code: three bytes (L: the two-byte ones)
		if (M512) {
			const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)E, 1, 64), hi = (uint32_t)__shfl_down((int)(uint32_t)(E >> 32), 1, 64);
			En = lane < 63 ? ((unsigned long long)hi << 32 | lo) : 0ull;
			L3 = L & ((E >> 1) | (En << 63));
			L &= ~L3;
		}
		D = (F & ~(C | L | L3)) | (F & ((L << 1) | (L3 << 1) | (L3 << 2))) | (F & ~safe);
	}
	// A STRETCH of the stream in which every flag byte is a COPY or a FILL that ends at or before bpos, and no flag-valued byte
	// lies inside the body of one of them, is walked in ONE step: the chain through it is exactly its flag bytes (a block's
	// successor is entered right behind its body and slides to the next flag byte -- which is the next flag byte of the stretch).
	// D = where a stretch must end: NORMAL blocks (their length needs the escape count), flag-valued bytes inside the body of a
	// FILL (which of the two is a block depends on the chain), blocks too close to bpos.  Conservative on purpose: a D bit
	// only hands the block at that byte to the one-block step below.  (D is computed above, where the three-byte FILLs are known.)
	const int first = forced != FX_UNSET ? FH : 0;              // first lane that walks (its entry: forced, or speculative)
	const bool walker = lane >= first && lane < 63 && cb >= 0;
	const uint32_t* mine = s_b + lane * FROW;
	const uint32_t behind = mine[FROW];                        // first dword of the piece behind
	unsigned long long V = 0, Q = 0;                           // entries / nodes of the lane's walk
	uint32_t xo = FX_UNSET, applied = FX_UNSET;
	uint32_t want = (lane == first && forced != FX_UNSET) ? forced : FX_SLIDE;
	for (int round = 0; round < 66; round++) {
		const bool need = walker && want != applied;
		if (__ballot(need) == 0) break;
		// ---- apply the entry `want`: trim the walk the lane has, or walk from the entry until it merges / leaves
		bool go = false;
		uint32_t q = 0, res = xo;
		unsigned long long Vw = 0, Qw = 0;
		if (need) {
			applied = want;
			if (want == FX_END) { V = 0; Q = 0; res = FX_END; }
			else {
				const uint32_t x = want == FX_SLIDE ? 0u : want;
				Vw = want == FX_SLIDE ? 0ull : 1ull << x;
				const unsigned long long m = F >> x;
				if (m == 0) { V = Vw; Q = 0; res = more ? FX_SLIDE : FX_END; }
				else {
					q = x + ctz64(m);
					if ((Q >> q) & 1ull) { V = Vw | (V & above(q)); Q &= ~0ull << q; }   // same chain from q on, same exit
					else go = true;
				}
			}
		}
		// The walk, written without divergent branches (selects on every lane).  One step takes a whole stretch (see D above;
		// it also ends where the old walk has a node) and then, if the chain arrives at a D byte, the one block there.
		uint32_t wres = FX_UNSET;
		for (;;) {
			if (__ballot(go) == 0) break;
			{
				const bool merged = go && ((Q >> q) & 1ull);
				wres = merged ? FX_MERGE + q : wres;
				go = go && !merged;
			}
			const unsigned long long hiq = ~0ull << q;             // bytes >= q
			const unsigned long long dq = (D & hiq) | (Q & (hiq << 1));
			const uint32_t d = dq ? ctz64(dq) : 64u;
			const bool str = go && d != q;
			if (__ballot(str) != 0) {                              // (wave-uniform: NORMAL-heavy streams rarely come here)
				const unsigned long long nodes = F & hiq & (d >= 64u ? ~0ull : ~(~0ull << d));
				const uint32_t last = 63u - (uint32_t)__builtin_clzll(nodes | 1ull);
				const uint32_t e = last + (((C >> last) & 1ull) ? 1u : (((L >> last) & 1ull) ? 2u : 3u));
				Qw |= str ? nodes : 0ull;
				// an entry behind every node (three-byte FILLs: what is neither COPY nor two-byte FILL); those at byte 64 and beyond belong to the next piece
				Vw |= str ? ((nodes & C) << 1) | ((nodes & L) << 2) | ((nodes & ~(C | L)) << 3) : 0ull;
				const unsigned long long m = F >> (e & 63u);
				const bool inside = e < 64u && m != 0;
				const uint32_t stop = e >= 64u ? e - 64u : (more ? FX_SLIDE : FX_END);
				wres = (str && !inside) ? stop : wres;
				const uint32_t p = e + ctz64(m | (1ull << 63));
				const bool arrived = str && inside;
				const bool merged = arrived && ((Q >> (p & 63u)) & 1ull);
				wres = merged ? FX_MERGE + p : wres;
				q = arrived ? p : q;
				go = go && (!str || (inside && !merged));
			}
			const bool sing = go && ((D >> q) & 1ull);
			if (__ballot(sing) != 0) {
				const uint32_t d0 = mine[q >> 2], d1 = mine[(q >> 2) + 1];
				const uint32_t two = __builtin_amdgcn_alignbyte((q >> 2) == 15u ? behind : d1, d0, q & 3u);
				const uint32_t t = two & 0xFFu;
				const bool isN = t == NORMAL_FLAG, isC = t == COPY_FLAG;
				uint32_t l1 = isC ? 1u : 2u + ((M512 && ((two >> 8) & 0x7Fu) == 127u) ? 1u : 0u);
				if (__ballot(sing && isN) != 0) {                  // NORMAL lengths: 16 dependent steps on the escape mask
					uint32_t len = 16;
					if (M512) {
						const uint32_t q1 = q + 1u;
						const uint32_t m = (uint32_t)((q1 < 64u ? E >> q1 : 0ull) | (En << (63u - q)));
						uint32_t pos = 0;
#pragma unroll
						for (int i = 0; i < 16; i++) pos += 1u + ((m >> pos) & 1u);
						len = pos;
					}
					if (isN) l1 = 1u + len;
				}
				const uint32_t e = q + l1;
				const bool over = (int)e > lim;                    // entered, not counted: the chain ends
				const bool cnt = sing && !over;
				Qw |= cnt ? 1ull << q : 0ull;
				Vw |= cnt ? (1ull << q) << l1 : 0ull;
				const unsigned long long m = F >> (e & 63u);
				const bool inside = cnt && e < 64u && m != 0;
				const uint32_t stop = over ? FX_END : (e >= 64u ? e - 64u : (more ? FX_SLIDE : FX_END));
				wres = (sing && !inside) ? stop : wres;
				q = inside ? e + ctz64(m) : q;
				go = go && (!sing || inside);
			}
		}
		if (need && wres != FX_UNSET) {
			if (wres >= FX_MERGE) {
				const uint32_t mq = wres - FX_MERGE;
				V = Vw | (V & above(mq)); Q = Qw | (Q & (~0ull << mq));
			} else { V = Vw; Q = Qw; res = wres; }
		}
		if (need) xo = res;
		// ---- next round: every lane's true entry is the exit of the lane before it
		const uint32_t px = (uint32_t)__shfl_up((int)xo, 1, 64);
		if (walker && lane > first) want = px;
	}
	// ---- results
	const bool own = lane >= FH && lane < 63;
	if (own) A.vm[((size_t)f * A.maxR + r) * FOWN + (lane - FH)] = walker ? V : 0ull;
	const uint32_t n = wave_sum(own && walker ? (uint32_t)__popcll(V) : 0u);
	const uint32_t ein = forced != FX_UNSET ? forced : (uint32_t)__builtin_amdgcn_readlane((int)xo, FH - 1);
	const uint32_t xout = (uint32_t)__builtin_amdgcn_readlane((int)xo, 62);
	if (lane == 0) A.rec[(size_t)f * A.maxR + r] = make_uint4(ein, xout, n, 0u);
	wave_lds_sync();
}

template <bool M512>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_fp_walk(FpArgs A)
{
	__shared__ uint32_t s_b[FP_LDS];
	const int lane = threadIdx.x;
	if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) *A.nbad = 0;   // (k_fp_finish, the next launch, counts the frames it gives up; saves a fill launch)
	for (uint32_t f = blockIdx.y; f < A.n_frames; f += gridDim.y) {   // (many small frames: the grid is capped, rows stride over the frames)
		const uint32_t bpos = A.bpos[f];
		const uint32_t nreg = min(bpos / FRB + 1u, A.maxR);    // positions 0 .. bpos can hold nodes
		for (uint32_t r = blockIdx.x; r < nreg; r += gridDim.x)
			fp_walk_region<M512>(A, s_b, f, r, r == 0 ? 0u : FX_UNSET, bpos, lane);   // block 0 is entered at byte 0
	}
}

// one wave per frame: prove the regions (see above), walk again those that are not, number the blocks
template <bool M512>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fp_finish(FpArgs A)
{
	__shared__ uint32_t s_b[FP_LDS];
	const uint32_t f = blockIdx.x;
	const int lane = threadIdx.x;
	const uint32_t bpos = A.bpos[f];
	const uint32_t nreg = min(bpos / FRB + 1u, A.maxR);
	uint4* rec = A.rec + (size_t)f * A.maxR;
	if (A.tidx)                                                // bitmap form: the frame's tile entries start out as "not entered" (k_fp_tiles, a later launch, writes those that are)
		for (uint32_t t = lane; t <= A.tpfd; t += 64) A.tidx[(size_t)f * (A.tpfd + 1) + t] = TIDX_NONE;
	// the first region at or behind `start` whose entry is not the exit of the region before it is walked again with that
	// exit forced; its own exit may have changed, so the search goes on right behind it
	int budget = FP_REPAIRS;
	for (uint32_t start = 1;;) {
		uint32_t bad = 0xFFFFFFFFu;
		for (uint32_t r0 = start & ~63u; r0 < nreg && bad == 0xFFFFFFFFu; r0 += 64) {
			const uint32_t r = r0 + lane;
			const bool in = r < nreg && r >= start;
			const uint32_t x = in ? __hip_atomic_load(&rec[r].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
			const uint32_t yp = in ? __hip_atomic_load(&rec[r - 1].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
			const unsigned long long bm = __ballot(in && x != yp);
			if (bm) bad = r0 + ctz64(bm);
		}
		if (bad == 0xFFFFFFFFu) break;
		if (budget-- == 0) {
			if (lane == 0) { A.fstate[f] = FS_BAD; atomicAdd(A.nbad, 1u); }
			return;
		}
		const uint32_t want = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&rec[bad - 1].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
		fp_walk_region<M512>(A, s_b, f, bad, want, bpos, lane);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
		start = bad + 1;
	}
	uint32_t run = 0;
	for (uint32_t r0 = 0; r0 < nreg; r0 += 64) {
		const uint32_t r = r0 + lane;
		const uint32_t n = r < nreg ? __hip_atomic_load(&rec[r].z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
		const uint32_t incl = wave_incl_scan(n, lane);
		if (r < nreg) A.kb[(size_t)f * A.maxR + r] = run + incl - n;
		run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
	}
	if (lane == 0) { A.fstate[f] = FS_OK; A.nentered[f] = run < A.nblk ? run : A.nblk; }
}

// entry bitmaps -> offsets[]: the region's entries are listed in LDS (byte position inside the region, in order) and go
// out as coalesced rows.
__global__ __launch_bounds__(64) void k_fp_expand(FpArgs A)
{
	__shared__ uint16_t s_pos[FRB];
	const int lane = threadIdx.x;
	const uint32_t f = blockIdx.y;
	if (A.fstate[f] != FS_OK) return;
	const uint32_t nreg = min(A.bpos[f] / FRB + 1u, A.maxR);
	uint32_t* off = A.offsets + (size_t)f * A.nblk;
	// a wave takes every gridDim.x-th region of its frame; the next one's bitmaps and block number are requested before
	// this one's entries are listed
	uint32_t kb_n = 0;
	unsigned long long V_n = 0;
	if (blockIdx.x < nreg) {
		kb_n = A.kb[(size_t)f * A.maxR + blockIdx.x];
		V_n = lane < FOWN ? A.vm[((size_t)f * A.maxR + blockIdx.x) * FOWN + lane] : 0ull;
	}
	for (uint32_t r = blockIdx.x; r < nreg; r += gridDim.x) {
		const uint32_t kb = kb_n;
		unsigned long long V = V_n;
		if (r + gridDim.x < nreg) {
			kb_n = A.kb[(size_t)f * A.maxR + r + gridDim.x];
			V_n = lane < FOWN ? A.vm[((size_t)f * A.maxR + r + gridDim.x) * FOWN + lane] : 0ull;
		}
		if (kb >= A.nblk) break;                                // (uniform) blocks beyond the frame are never entered
		const uint32_t vlo = (uint32_t)V, vhi = (uint32_t)(V >> 32);
		const uint32_t n = (uint32_t)__popc(vlo) + (uint32_t)__popc(vhi);
		const uint32_t incl = wave_incl_scan(n, lane);
		const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
		const uint32_t first = incl - n;
		// pieces with few entries: every lane walks the set bits of its own (32 bits at a time: one-instruction bit scans);
		// dense pieces (a run of COPYs: up to 64 entries) one by one by the whole wave, each lane whose bit is set writing at
		// the rank of its bit
		unsigned long long dense = __ballot(n >= 32u);
		if (n < 32u) {
			uint32_t j = first, m = vlo;
			const uint32_t base = (uint32_t)lane * FC;
			while (m) { s_pos[j++] = (uint16_t)(base + (uint32_t)__builtin_ctz(m)); m &= m - 1u; }
			m = vhi;
			while (m) { s_pos[j++] = (uint16_t)(base + 32u + (uint32_t)__builtin_ctz(m)); m &= m - 1u; }
		}
		while (dense) {                                        // (uniform)
			const int c = (int)ctz64(dense);
			dense &= dense - 1ull;
			const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)vlo, c), hi = (uint32_t)__builtin_amdgcn_readlane((int)vhi, c);
			const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)first, c);
			if ((((unsigned long long)hi << 32 | lo) >> lane) & 1ull)
				s_pos[at + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u))] = (uint16_t)(c * FC + lane);
		}
		wave_lds_sync();
		for (uint32_t i = lane; i < tot; i += 64)
			if (kb + i < A.nblk) off[kb + i] = r * FRB + s_pos[i];
		wave_lds_sync();
	}
}

// position of the k-th set bit (k = 0: the lowest) of v; k < popcount(v)
__device__ __forceinline__ uint32_t select64(unsigned long long v, uint32_t k)
{
	uint32_t w = (uint32_t)v, base = 0, c = (uint32_t)__popc(w);
	if (k >= c) { k -= c; w = (uint32_t)(v >> 32); base = 32; }
	c = (uint32_t)__popc(w & 0xFFFFu); if (k >= c) { k -= c; w >>= 16; base += 16; }
	w &= 0xFFFFu;
	c = (uint32_t)__popc(w & 0xFFu);   if (k >= c) { k -= c; w >>= 8;  base += 8; }
	w &= 0xFFu;
	c = (uint32_t)__popc(w & 0xFu);    if (k >= c) { k -= c; w >>= 4;  base += 4; }
	w &= 0xFu;
	c = (uint32_t)__popc(w & 0x3u);    if (k >= c) { k -= c; w >>= 2;  base += 2; }
	return base + ((k >= (w & 1u)) ? 1u : 0u);
}

// Entry bitmaps -> where the first block of every k_decode tile (DEC_T consecutive blocks) is entered.  This is all
// k_decode needs besides the bitmaps themselves: it ranks its own blocks in the bitmap words between two tile entries
// (offsets[] -- 4 bytes per block written by k_fp_expand and read back -- never exists on this path).
// One wave per region, like k_fp_expand; tidx is pre-filled with TIDX_NONE.
__global__ __launch_bounds__(64) void k_fp_tiles(FpArgs A)
{
	const int lane = threadIdx.x;
	if (A.dirty && blockIdx.x == 0 && blockIdx.y == 0)         // (saves the fill launch in front of k_decode)
		for (uint32_t i = lane; i < A.ndirty; i += 64) A.dirty[i] = 0;
	for (uint32_t f = blockIdx.y; f < A.n_frames; f += gridDim.y) {
	const bool fell_back = A.fstate[f] == FS_BAD;              // its entry bits come from the robust kernels (k_parse_emit), nobody has numbered its blocks yet
	const uint32_t nreg = min(A.bpos[f] / FRB + 1u, A.maxR);
	uint32_t* tx = A.tidx + (size_t)f * (A.tpfd + 1);
	for (uint32_t r = blockIdx.x; r < nreg; r += gridDim.x) {
		uint32_t kb;
		if (fell_back) {
			// first block number of the region = entries in the regions before it: counted here, by the region's own wave (the
			// exception path: a launch of its own for this cost 5 us on every decode call that had nothing to count)
			const unsigned long long* v = A.vm + (size_t)f * A.maxR * FOWN;
			uint32_t n = 0;
			for (uint32_t i = lane; i < r * FOWN; i += 64) n += (uint32_t)__popcll(v[i]);
			kb = wave_sum(n);
			if (lane == 0) A.kb[(size_t)f * A.maxR + r] = kb;
		} else kb = A.kb[(size_t)f * A.maxR + r];
		if (kb >= A.nblk) {                                     // (uniform) blocks beyond the frame are never entered
			if (fell_back) continue;                            // (its later regions still get their number: bm_offset_of searches kb[] of the whole frame)
			break;
		}
		const unsigned long long V = lane < FOWN ? A.vm[((size_t)f * A.maxR + r) * FOWN + lane] : 0ull;
		const uint32_t n = (uint32_t)__popcll(V);
		const uint32_t incl = wave_incl_scan(n, lane);
		const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
		const uint32_t first = incl - n;
		uint32_t end = kb + tot;
		if (end > A.nblk) end = A.nblk;
		// tiles whose first block is entered in this region: m0 .. m0 + nt - 1 (uniform).  The kernel is bound by VALU issue, so
		// the bit select runs ONCE, on lane j for tile m0 + j: per tile only the piece that holds its first block is found (the
		// pieces' inclusive counts are monotone: it is the number of pieces that end at or before the target) and its bitmap
		// word and rank are handed to lane j.
		const uint32_t m0 = (kb + DEC_T - 1) / DEC_T;
		uint32_t nt = end > m0 * DEC_T ? (end - m0 * DEC_T + DEC_T - 1) / DEC_T : 0u;
		for (uint32_t j0 = 0; j0 < nt; j0 += 64) {                 // (more than 64 tiles per region: never with DEC_T = 256)
			const uint32_t cnt = min(nt - j0, 64u);
			uint32_t xlo = 0, xhi = 0, xr = 0, xo = 0;
			for (uint32_t j = 0; j < cnt; j++) {
				const uint32_t target = (m0 + j0 + j) * DEC_T - kb;
				const int ol = (int)__popcll(__ballot(incl <= target));     // < 64: target < tot
				const uint32_t vl = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)V, ol), vh = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(V >> 32), ol);
				const uint32_t fo = (uint32_t)__builtin_amdgcn_readlane((int)first, ol);
				const bool me = (uint32_t)lane == j;
				xlo = me ? vl : xlo; xhi = me ? vh : xhi; xr = me ? target - fo : xr; xo = me ? (uint32_t)ol : xo;
			}
			if ((uint32_t)lane < cnt)
				tx[m0 + j0 + lane] = r * FRB + xo * FC + select64((unsigned long long)xhi << 32 | xlo, xr);
		}
	}
	}
}

// entry position of block b of frame f from the bitmaps (b < nentered[f]); the slow, self-contained form: k_fixup and
// the tiles of k_decode whose entries span more bitmap words than the workgroup has lanes
__device__ uint32_t bm_offset_of(const unsigned long long* vm, const uint32_t* kb, uint32_t maxR, uint32_t bpos, uint32_t f, uint32_t b)
{
	const uint32_t nreg = min(bpos / FRB + 1u, maxR);
	const uint32_t* kbp = kb + (size_t)f * maxR;
	uint32_t lo = 0, hi = nreg - 1;
	while (lo < hi) {                                          // the last region whose first block number is <= b
		const uint32_t mid = (lo + hi + 1) >> 1;
		if (kbp[mid] <= b) lo = mid; else hi = mid - 1;
	}
	uint32_t rem = b - kbp[lo];
	const unsigned long long* v = vm + ((size_t)f * maxR + lo) * FOWN;
	for (int k = 0; k < FOWN; k++) {
		const unsigned long long w = v[k];
		const uint32_t c = (uint32_t)__popcll(w);
		if (rem < c) return lo * FRB + (uint32_t)k * FC + select64(w, rem);
		rem -= c;
	}
	return 0;                                                  // (not reached for b < nentered)
}

struct DecArgs {
	const uint8_t* bits;
	unsigned long long stride;
	const uint32_t* bpos;
	const uint32_t* offsets;
	const uint32_t* nentered;
	uint32_t* out;
	const uint32_t* pal;
	const uint32_t* prev;
	const uint32_t* prev_iframe;
	uint32_t* dirty;
	uint32_t n_frames, w, h, bw, nblk, tpf, first_fc, phase, n_groups;
	uint32_t grp0;          // first GOP of this launch (its items cover GOPs grp0 .. grp0 + n_items / tpf - 1)
	uint32_t n_items;       // k_decode: (GOP, tile) pairs of this launch
	// bitmap form (BM kernels): the parser's entry bitmaps, first block number per region, tile entries -- no offsets[]
	const unsigned long long* vm;
	const uint32_t* kb;
	const uint32_t* tidx;
	uint32_t maxR;
};

// one 4x4 block of D2 (512 colours, src/agmv_decode.c:234-319) or D3 (256 colours, :335-396).
// `cur` is the block's img_data, `icol` the block's iframe->img_data.  fill_written reports a
// FILL that stored pixels (the caller applies the last-block quirk, :264-266).  stale / istale: bit k set when pixel k of
// cur / icol still derives from the state before the GOP (per pixel: a NORMAL block cut off by bpos stores a prefix).
template <bool M512, class Src>
__device__ __forceinline__ void decode_block(const Src& src, uint32_t bitpos, const uint32_t bpos,
                                             const uint32_t* pal, uint32_t (&cur)[16], const uint32_t (&icol)[16],
                                             uint32_t istale, uint32_t& stale, bool& fill_written)
{
	fill_written = false;
	uint32_t byte = src(bitpos++);
	bool invalid = false;
	while (!is_flag(byte)) {                                   // flag resync, :236-243
		byte = src(bitpos++);
		if (bitpos > bpos) break;
	}
	if (!is_flag(byte)) invalid = true;
	if (byte == FILL_FLAG) {
		uint32_t idx = src(bitpos++), color;
		if (M512) {
			const uint32_t base = (idx & 0x80u) ? 256u : 0u;
			if ((idx & 0x7fu) < 127u) color = pal[base + (idx & 0x7fu)];
			else color = pal[base + src(bitpos++)];
		} else {
			color = pal[idx];
		}
		if (!(bitpos > bpos)) {
#pragma unroll
			for (int k = 0; k < 16; k++) cur[k] = color;
			stale = 0;
			fill_written = true;
		}
	} else if (byte == COPY_FLAG) {                            // no over-run check, :281-290
#pragma unroll
		for (int k = 0; k < 16; k++) cur[k] = icol[k];
		stale = istale;
	} else {
		bool dead = false;                                     // once a row broke, nothing more is stored
#pragma unroll
		for (int j = 0; j < 4; j++) {
			bool rowbreak = false;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				if (!rowbreak) {
					uint32_t idx = src(bitpos++), color;
					if (M512) {
						const uint32_t base = (idx & 0x80u) ? 256u : 0u;
						if ((idx & 0x7fu) < 127u) color = pal[base + (idx & 0x7fu)];
						else color = pal[base + src(bitpos++)];
					} else {
						color = pal[idx];
					}
					if (bitpos > bpos || invalid) { invalid = false; rowbreak = true; dead = true; }
					else { cur[j * 4 + i] = color; stale &= ~(1u << (j * 4 + i)); }
				}
			}
		}
		(void)dead;
	}
}

// decode_block for a block whose bytes sit in the workgroup's LDS window, with the dependent byte -> byte -> palette
// round trips of the reference walk taken apart: ONE round of reads fetches the flag, the two bytes behind it and the
// 36 bytes a NORMAL body can span; which of those are escape codes ((b & 0x7f) == 127) becomes a bit mask, the 16
// code positions are walked in registers, and the 32 code bytes and then the 16 palette entries are fetched as
// independent reads.  Anything unusual (no flag at the entry offset, a block that over-runs bpos, bytes outside the
// window) takes the generic walk above, which is the reference's loop verbatim.
template <bool M512>
__device__ __forceinline__ void decode_block_staged(const StagedSrc& src, uint32_t off, const uint32_t bpos,
                                                    const uint32_t* pal, uint32_t (&cur)[16], const uint32_t (&icol)[16],
                                                    uint32_t istale, uint32_t& stale, bool& fill_written)
{
	typedef const __attribute__((address_space(3))) uint8_t* lds8;
	typedef const __attribute__((address_space(3))) uint32_t* lds32;
	const uint32_t d = off - src.lo;
	bool slow = true;
	fill_written = false;
	if (off >= src.lo && d + 44u <= src.len) {                 // flag + 33 bytes + alignment slack inside the window
		const lds8 p = src.lds + d;
		const uint32_t b0 = p[0], b1 = p[1], b2 = p[2];
		uint32_t m = 0;                                        // bit t: the byte at off+1+t is an escape code
		if (M512) {
			const uint32_t d1 = d + 1u, a = d1 & ~3u;
			unsigned long long em = 0;
#pragma unroll
			for (int k = 0; k < 9; k++) {
				const uint32_t w = *(lds32)(src.lds + a + 4u * k);
				const uint32_t z = ((w & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u;     // bit 7 of every byte equal to 127
				const uint32_t nib = __builtin_amdgcn_udot4(z, 0x08040201u, 0u, false) >> 7;    // those four bits, adjacent (bytes {0, 0x80} . weights 1, 2, 4, 8)
				em |= (unsigned long long)nib << (4 * k);
			}
			m = (uint32_t)(em >> (d1 & 3u));
		}
		if (b0 == COPY_FLAG) {                                 // no over-run check, :281-290
#pragma unroll
			for (int k = 0; k < 16; k++) cur[k] = icol[k];
			stale = istale;
			slow = false;
		} else if (b0 == FILL_FLAG) {
			uint32_t ci = b1, end = off + 2u;
			if (M512) {
				const bool esc = (b1 & 0x7fu) == 127u;
				ci = ((b1 & 0x80u) << 1) + (esc ? b2 : (b1 & 0x7fu));
				end += esc ? 1u : 0u;
			}
			const uint32_t color = pal[ci];
			if (!(end > bpos)) {
#pragma unroll
				for (int k = 0; k < 16; k++) cur[k] = color;
				stale = 0;
				fill_written = true;
			}
			slow = false;
		} else if (b0 == NORMAL_FLAG) {
			uint32_t ci[16], pos = 0;
#pragma unroll
			for (int i = 0; i < 16; i++) {
				const uint32_t f0 = p[1u + pos], f1 = p[2u + pos];
				if (M512) {
					const uint32_t esc = (m >> pos) & 1u;
					ci[i] = ((f0 & 0x80u) << 1) + (esc ? f1 : (f0 & 0x7fu));
					pos += 1u + esc;
				} else {
					ci[i] = f0;
					pos += 1u;
				}
			}
			if (off + 1u + pos <= bpos) {                      // every code ends inside the stream: all 16 pixels are stored
#pragma unroll
				for (int k = 0; k < 16; k++) cur[k] = pal[ci[k]];
				stale = 0;
				slow = false;
			}
		}
	}
	if (slow) decode_block<M512>(src, off, bpos, pal, cur, icol, istale, stale, fill_written);
}

__device__ __forceinline__ void load_block(const uint32_t* frame, uint32_t poff, uint32_t w, uint32_t (&v)[16])
{
#pragma unroll
	for (int r = 0; r < 4; r++) {
		uint4 q = *(const uint4*)(frame + poff + r * w);
		v[r * 4 + 0] = q.x; v[r * 4 + 1] = q.y; v[r * 4 + 2] = q.z; v[r * 4 + 3] = q.w;
	}
}

__device__ __forceinline__ void store_block(uint32_t* frame, uint32_t poff, uint32_t w, const uint32_t (&v)[16])
{
#pragma unroll
	for (int r = 0; r < 4; r++) {
		uint4 q;
		q.x = v[r * 4 + 0]; q.y = v[r * 4 + 1]; q.z = v[r * 4 + 2]; q.w = v[r * 4 + 3];
		// written once, read by nobody on the device: non-temporal (measured 0.474 -> 0.386 ms per 256 x 1080p frames)
		typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
		__builtin_nontemporal_store((u32x4){q.x, q.y, q.z, q.w}, (u32x4*)(frame + poff + r * w));
	}
}

// K3: one lane = one 4x4 block carried through the <=4 frames of its GOP (img_data and
// iframe->img_data of the block live in registers).  A block whose value depends on a frame
// outside the GOP (not rewritten since the GOP started) is flagged in `dirty` and repaired by
// k_fixup; everything else is final.
//
// Everything the GOP needs is loaded UP FRONT, in two dependent round trips: (1) the block's entry offset in each
// of the four frames (+ nentered/bpos, palette, previous state), (2) after the workgroup has exchanged the byte
// range its entered blocks span in each frame, the four byte windows into a quad-buffered LDS stage.  The frame
// loop then reads LDS only -- no global load, no wait on the vector-memory counter, no barrier (except the last
// tile's neighbour exchange) -- so the 64 B/lane pixel stores of one frame drain while the next is reconstructed.
// (A wave's memory counter retires in order: with per-frame staging every wait for the next frame's bytes also
// waited for the previous frame's stores, and under saturating writes those round trips take 2-3 us.)
#ifndef DEC_WPE
#define DEC_WPE 5         // waves per SIMD: 87 VGPRs, no spills; 6 spills and is slower
#endif
template <bool M512, bool BM, bool LOOP>   // (the looping form, a test and tuning aid, would spill at DEC_WPE waves: it gets the registers of one wave fewer)
__global__ __launch_bounds__(DEC_T, LOOP ? DEC_WPE - 1 : DEC_WPE) void k_decode(DecArgs A)
{
	__shared__ uint32_t s_pal[512];
	__shared__ uint32_t s_nb[DEC_T];        // neighbour exchange for the last-block quirk
	__shared__ uint32_t s_nbstale[DEC_T];
	__shared__ __attribute__((aligned(16))) uint8_t s_bytes[4][DEC_STAGE];   // the tile's slice of each frame's bitstream
	__shared__ uint32_t s_rng[4][2];        // per frame: [0] lowest, [1] highest entry offset of the tile's entered blocks
	const int tid = threadIdx.x;
	const uint32_t npx = A.w * A.h;
	for (int i = tid; i < 512; i += DEC_T) s_pal[i] = A.pal[i];

	// items = (GOP, tile) pairs of the launch.  The grid has one workgroup per item (LOOP false: straight-line code) unless
	// AGMV_DEC_GRID caps it: workgroup g then takes items g, g + gridDim.x, ... one after the other (a static assignment:
	// nothing to wait for).  Everything below is per item; only the palette copy is the workgroup's.
	// Items run from the launch's LAST GOP to its first.  The parser in front of this kernel reads the batch's bitstreams
	// first frame to last and writes their entry bitmaps in that order, and a batch is larger than the memory-side cache
	// (c3: 446 MB of stream): what the cache still holds when this kernel starts is the END of the batch.  GOPs are
	// independent here (k_fixup repairs what is not), so the order is free; first GOP first, every window load of c3
	// missed the cache and k_decode + k_fixup took 1.85 ms instead of 1.69 (profiles/decode_pipeline/).
	for (uint32_t item = blockIdx.x;;) {
	const uint32_t lgroup = (A.n_items - 1 - item) / A.tpf, tile = item % A.tpf, group = lgroup + A.grp0;
	const int f_lo = group == 0 ? 0 : (int)(group * 4 - A.phase);
	int f_hi = (int)(group * 4 - A.phase) + 4;
	if (f_hi > (int)A.n_frames) f_hi = (int)A.n_frames;
	const int nf = f_hi - f_lo;                                // 1..4 frames

	const uint32_t blk = tile * DEC_T + tid;
	const bool valid = blk < A.nblk;
	const uint32_t b = valid ? blk : A.nblk - 1;
	const uint32_t by = b / A.bw, bx = b - by * A.bw;
	const uint32_t poff = by * 4 * A.w + bx * 4;
	const bool has_last = (tile == A.tpf - 1);                 // this workgroup holds block nblk-1
	const bool is_last = valid && blk == A.nblk - 1;

	uint32_t off[4], ne[4], bp[4];
	uint32_t r_lo[4], r_len[4];
	uint32_t cur[16], icol[16];
	uint32_t stale, istale;
	// stale / istale (a bit per pixel): the block's img_data / iframe->img_data still derive from the state before this GOP.  For the first
	// GOP of the batch that state is the caller's (prev / prev_iframe) and the pixels are right as they are; what the
	// flags then tell is whether the batch DEPENDS on the state handed in (reported through agmv_hip_decode_prior_dependent).
	auto load_prior = [&]() {
		if (group == 0) {                                      // state of the decoder before the batch
			if (A.prev) load_block(A.prev, poff, A.w, cur);
			else {
#pragma unroll
				for (int k = 0; k < 16; k++) cur[k] = 0;
			}
			if (A.prev_iframe) load_block(A.prev_iframe, poff, A.w, icol);
			else {
#pragma unroll
				for (int k = 0; k < 16; k++) icol[k] = 0;
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) { cur[k] = 0; icol[k] = 0; }
		}
		stale = 0xFFFFu; istale = 0xFFFFu;
	};
	uint32_t st[4][DEC_SR];                                    // the byte windows on their way from global memory to LDS
	// The first DEC_T dwords of every window go out as unconditional buffer loads (a lane beyond the window is out of range: 0,
	// no fetch, NO BRANCH), LAST; the rest -- needed only where a tile's blocks average more than 4 bytes -- under uniform
	// branches ahead of them.  The compiler waits for an earlier load with the count of loads that follow it on EVERY path,
	// i.e. those four: the bitmap words are then awaited with the windows still in flight.  (With all of them under branches it
	// has to assume none was issued, and the first wait drains everything.)
	auto load_windows = [&]() {
		__amdgpu_buffer_rsrc_t rs[4];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint8_t* fb = A.bits + (size_t)(i < nf ? f_lo + i : f_lo) * A.stride + r_lo[i];
			uint32_t nrec = r_lo[i] < (uint32_t)A.stride ? (uint32_t)A.stride - r_lo[i] : 0u;
			if (nrec > r_len[i]) nrec = r_len[i];
			rs[i] = uniform_rsrc(fb, nrec & ~3u);
		}
#pragma unroll
		for (int i = 0; i < 4; i++) {
#pragma unroll
			for (int k = 1; k < DEC_SR; k++) {
				st[i][k] = 0;
				if ((uint32_t)(k * DEC_T) * 4u < r_len[i])         // (uniform)
					st[i][k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs[i], (uint32_t)(k * DEC_T + tid) * 4u, 0, 0);
			}
		}
#pragma unroll
		for (int i = 0; i < 4; i++) st[i][0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs[i], (uint32_t)tid * 4u, 0, 0);
	};
	auto store_windows = [&]() {
#pragma unroll
		for (int i = 0; i < 4; i++) {
#pragma unroll
			for (int k = 0; k < DEC_SR; k++) {
				const uint32_t j = (uint32_t)(k * DEC_T + tid) * 4u;
				if (j < r_len[i]) *(uint32_t*)(s_bytes[i] + j) = st[i][k];
			}
		}
	};
	if (!BM) {
		// ---- round trip 1: entry offsets, nentered, bpos of every frame of the GOP; previous state of the block
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int fi = i < nf ? f_lo + i : f_hi - 1;
			off[i] = A.offsets[(size_t)fi * A.nblk + b];            // (non-temporal here and in k_fp_expand's stores: 0.375 -> 0.39-0.41 ms, not kept)
			ne[i] = A.nentered[fi]; bp[i] = A.bpos[fi];
		}
		// the range the tile's entered blocks can touch in frame i: [first entry, last entry + 33 + 8]; entry offsets
		// increase with the block index, so it is [offset of lane 0, offset of the last entered lane]
#pragma unroll
		for (int i = 0; i < 4; i++) {
			if (i < nf && valid && blk < ne[i]) {
				if (tid == 0) s_rng[i][0] = off[i];
				if (blk + 1 == ne[i] || tid == DEC_T - 1 || blk + 1 == A.nblk) s_rng[i][1] = off[i];   // exactly one lane
			}
		}
		__syncthreads();                                       // ranges (and the palette) visible
		// ---- round trip 2: the four byte windows, all in flight together
#pragma unroll
		for (int i = 0; i < 4; i++) {
			r_lo[i] = 0; r_len[i] = 0;
			if (i < nf && tile * DEC_T < ne[i]) {              // uniform: at least the first block of the tile is entered
				r_lo[i] = s_rng[i][0] & ~3u;
				uint32_t len = s_rng[i][1] + 48u - r_lo[i];
				if (len > (uint32_t)DEC_STAGE) len = DEC_STAGE;
				r_len[i] = len & ~3u;
			}
		}
	} else {
		// ---- bitmap form.  Round trip 1 (uniform, scalar loads): where this tile and the next one are entered in each frame.
		// Round trip 2, all in flight together: the entry bitmap words between the two (one per lane, 64 bytes of stream
		// each) and the byte windows.  The lanes then rank their blocks in the bitmap: block j of the tile is entered at
		// the j-th set bit behind the tile's entry -- an exclusive scan of the words' popcounts through LDS, a binary search
		// of the lane's rank in it, a bit select.
		uint32_t t0[4], t1[4], P0[4];
		bool wide[4];
		{
			// one vector load for the sixteen words (lane = kind * 4 + frame), broadcast by v_readlane: as scalar loads they
			// are sixteen scalar-cache misses, and every tile's are different
			const int q = tid & 3, kind = (tid >> 2) & 3;
			const int fq = q < nf ? f_lo + q : f_hi - 1;
			const uint32_t* hp = kind == 0 ? A.nentered + fq : (kind == 1 ? A.bpos + fq : A.tidx + (size_t)fq * (A.tpf + 1) + tile + (kind == 3 ? 1 : 0));
			const uint32_t hv = *hp;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				ne[i] = (uint32_t)__builtin_amdgcn_readlane((int)hv, i); bp[i] = (uint32_t)__builtin_amdgcn_readlane((int)hv, 4 + i);
				t0[i] = (uint32_t)__builtin_amdgcn_readlane((int)hv, 8 + i); t1[i] = (uint32_t)__builtin_amdgcn_readlane((int)hv, 12 + i);
			}
		}
		unsigned long long vw[4];
		bool usew[4];
		const unsigned long long* vp[4];
		uint32_t npmax = 1;                                    // words of the longest range (uniform)
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int fi = i < nf ? f_lo + i : f_hi - 1;
			const bool has = i < nf && tile * DEC_T < ne[i] && t0[i] != TIDX_NONE;   // uniform
			r_lo[i] = 0; r_len[i] = 0; P0[i] = 0; wide[i] = false; off[i] = 0; usew[i] = false;
			uint32_t pc = 0;
			if (has) {
				P0[i] = t0[i] >> 6;
				const uint32_t last = (t1[i] != TIDX_NONE ? t1[i] - 1u : bp[i]) >> 6;   // last word that can hold an entry of this tile
				wide[i] = last - P0[i] >= (uint32_t)DEC_T;     // (garbage between blocks: the resync can skip any number of bytes)
				if (!wide[i] && last - P0[i] + 1u > npmax) npmax = last - P0[i] + 1u;
				pc = P0[i] + (uint32_t)tid;
				usew[i] = !wide[i] && pc <= last;
				r_lo[i] = t0[i] & ~3u;
				uint32_t hi = (t1[i] != TIDX_NONE ? t1[i] : bp[i] + 1u) + 48u;
				uint32_t len = hi > r_lo[i] ? hi - r_lo[i] : 0u;
				if (len > (uint32_t)DEC_STAGE) len = DEC_STAGE;
				r_len[i] = len & ~3u;
			}
			vp[i] = A.vm + (size_t)fi * A.maxR * FOWN + (usew[i] ? pc : 0u);   // always a readable word: the four loads go out back to back, unconditionally
		}
#pragma unroll
		for (int i = 0; i < 4; i++) vw[i] = *vp[i];
		asm volatile("" ::: "memory");                      // the four bitmap loads stay AHEAD of the windows: the first wait then leaves the windows in flight
		load_windows();
#pragma unroll
		for (int i = 0; i < 4; i++) {
			vw[i] = usew[i] ? vw[i] : 0ull;
			if (tid == 0) vw[i] &= ~0ull << (t0[i] & 63u);
		}
		// scan + search, with the LDS of the byte windows (not yet written) as scratch: [frame][lane] prefix (u16) | word (u64)
		uint16_t* s_pre = (uint16_t*)&s_bytes[0][0];               // 4 * DEC_T * 2 bytes
		unsigned long long* s_w = (unsigned long long*)(&s_bytes[0][0] + 4 * DEC_T * 2);
		uint32_t* s_wt = s_nb;                                 // [frame][wave] entries per wave
		static_assert(4 * DEC_T * 10 <= 4 * DEC_STAGE && DEC_T / 64 * 4 <= DEC_T, "scratch fits the stage");
		uint32_t incl[4], cnt[4];
		const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
		for (int i = 0; i < 4; i++) {
			cnt[i] = (uint32_t)__popcll(vw[i]);
			incl[i] = wave_incl_scan(cnt[i], lane);
			if (lane == 63) s_wt[i * (DEC_T / 64) + wave] = incl[i];
		}
		lds_barrier();                                         // wave totals visible (an LDS-only barrier: the byte windows stay in flight under the scan and the search)
#pragma unroll
		for (int i = 0; i < 4; i++) {
			uint32_t base = 0;
#pragma unroll
			for (int wv = 0; wv < DEC_T / 64; wv++) base += wv < wave ? s_wt[i * (DEC_T / 64) + wv] : 0u;
			s_pre[i * DEC_T + tid] = (uint16_t)(base + incl[i] - cnt[i]);
			s_w[i * DEC_T + tid] = vw[i];
		}
		lds_barrier();
		{
			// the four frames' searches step together (four independent chains of LDS reads); a lane that is not entered
			// searches too and its result is not used
			uint32_t st0 = DEC_T / 2;
			while (st0 >= npmax && st0 > 1) st0 >>= 1;             // largest power of two below npmax (index 0 needs no test)
			uint32_t pz[4] = {0, 0, 0, 0};                         // the last word whose prefix is <= the lane's rank
			// (uniform) as many halvings as the longest of the four word ranges needs: a tile of the benchmark clip spans ~14 words
			for (uint32_t st = st0; st >= 1; st >>= 1) {
				uint32_t v[4];
#pragma unroll
				for (int i = 0; i < 4; i++) v[i] = s_pre[i * DEC_T + pz[i] + st];
#pragma unroll
				for (int i = 0; i < 4; i++) pz[i] += v[i] <= (uint32_t)tid ? st : 0u;
			}
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const uint32_t pre = s_pre[i * DEC_T + pz[i]];
				const unsigned long long wv = s_w[i * DEC_T + pz[i]];
				off[i] = ((P0[i] + pz[i]) << 6) + select64(wv, (uint32_t)tid - pre);
			}
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const int fi = i < nf ? f_lo + i : f_hi - 1;
				if (wide[i] && i < nf && valid && blk < ne[i]) off[i] = bm_offset_of(A.vm, A.kb, A.maxR, bp[i], (uint32_t)fi, blk);   // (uniform branch; exotic)
			}
		}
		lds_barrier();                                         // scratch read: the byte windows may land
	}
	if (!BM) { load_windows(); store_windows(); }
	else store_windows();
	load_prior();                                              // (only the first GOP of a batch reads anything here: kept out of the prologue, whose registers hold the byte windows)
	__syncthreads();                                           // the last wait on global loads in this kernel

	bool anystale = false, needfix = false, depstale = false;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		if (i >= nf) break;
		const int f = f_lo + i;
		bool fill_written = false;
		const bool entered = valid && blk < ne[i];
		const uint32_t own3 = cur[3];                          // the block's pixel (3,0) and staleness before this frame
		const uint32_t stale0 = stale;
		if (entered) {
			StagedSrc src{(const __attribute__((address_space(3))) uint8_t*)s_bytes[i], r_lo[i], r_len[i], A.bits + (size_t)f * A.stride, (uint32_t)A.stride};
			decode_block_staged<M512>(src, off[i], bp[i], s_pal, cur, icol, istale, stale, fill_written);
		}
		if (has_last) {                                        // img_data[(x-1)+(y+1)*w] of the block to the left
			s_nb[tid] = cur[7];
			s_nbstale[tid] = (stale >> 7) & 1u;
			lds_barrier();
			if (is_last && fill_written) {
				if (A.bw == 1) {                                   // one block per row: the reference's 64-bit (x-1) wraps to the
#pragma unroll                                                     // block's own pixel (3,0), not yet written in this frame
					for (int k = 0; k < 16; k++) cur[k] = own3;
					stale = ((stale0 >> 3) & 1u) ? 0xFFFFu : 0u;
				} else if (tid > 0) {
					uint32_t c = s_nb[tid - 1];
#pragma unroll
					for (int k = 0; k < 16; k++) cur[k] = c;
					stale = s_nbstale[tid - 1] ? 0xFFFFu : 0u;
				} else {
					stale = 0xFFFFu; needfix = true;          // neighbour lives in another tile: fix-up (the pixels here are NOT final,
				}                                              // and k_fixup tells whether they depend on the batch's prior state)
			}
			lds_barrier();
		}
		if (((A.first_fc + f) & 3u) == 0) {                    // I-frame snapshot, :401-405
#pragma unroll
			for (int k = 0; k < 16; k++) icol[k] = cur[k];
			istale = stale;
		}
		anystale |= stale != 0;
		if (!needfix) depstale |= stale != 0;
		if (valid) store_block(A.out + (size_t)f * npx, poff, A.w, cur);
	}
	if (valid && (anystale || needfix)) {
		if (group != 0 || needfix) {                           // stale in any frame of a later GOP: k_fixup replays the block
			atomicOr(A.dirty + (blk >> 5), 1u << (blk & 31u));
			A.dirty[(A.nblk + 31) >> 5] = 1u;                   // "anything to repair" word behind the bitmap
		}
		if (group == 0 && depstale) A.dirty[((A.nblk + 31) >> 5) + 1] = 1u;   // the batch depends on the decoder state before it
	}
	if (!LOOP) break;
	item += gridDim.x;
	if (item >= A.n_items) break;
	__syncthreads();                                           // the next item's ranges, scratch and windows go where this one's are still being read
	}
}

// K4: repair of the blocks k_decode flagged.  The blocks are independent of each other (a block's pixels in frame f derive
// from the SAME block in earlier frames) with one exception, the last block of the frame, whose FILL takes a pixel of its
// left neighbour (src/agmv_decode.c:264-266).  So the grid is one wave per 64 consecutive block positions; a wave whose
// 64 bitmap bits are clear exits at once, the others replay ALL frames in order for their flagged positions from the true
// pre-batch state and overwrite the output.  The wave that holds block nblk-1 also replays block nblk-2 (flagged or not:
// a replay from the true state writes the true pixels), in the lane below when both sit in one wave, else in lane 1.
// The replay follows, pixel by pixel, what still derives from the pre-batch state, which k_decode cannot tell beyond the
// batch's first GOP (a batch that starts inside a GOP hands the caller's I-frame snapshot on to a COPY in its first
// I-frame) nor for a last block whose left neighbour sits in another tile: every block it leaves to this kernel is replayed.
template <bool M512, bool BM>
__global__ __launch_bounds__(64) void k_fixup(DecArgs A)
{
	__shared__ uint32_t s_pal[512];
	const int lane = threadIdx.x;
	const uint32_t npx = A.w * A.h;
	const uint32_t nwords = (A.nblk + 31) >> 5;
	if (A.dirty[nwords] == 0) return;                          // nothing depends on an earlier GOP: done
	const uint32_t base = blockIdx.x * 64u;
	const uint32_t w0 = A.dirty[base >> 5], w1 = (base >> 5) + 1 < nwords ? A.dirty[(base >> 5) + 1] : 0u;
	if ((w0 | w1) == 0) return;
	uint32_t blk = base + (uint32_t)lane;
	bool active = blk < A.nblk && (((lane < 32 ? w0 : w1) >> (lane & 31)) & 1u);
	// the last block's left neighbour rides along
	const uint32_t last = A.nblk - 1;
	const bool have_last = last >= base && last < base + 64 && ((((last - base) < 32 ? w0 : w1) >> ((last - base) & 31)) & 1u);
	int nb_lane = -1;                                          // lane that holds block nblk-2 when this wave repairs nblk-1
	if (have_last && A.nblk >= 2) {
		if (last > base) { nb_lane = (int)(last - base) - 1; if (lane == nb_lane) active = true; }
		else { nb_lane = 1; if (lane == 1) { blk = last - 1; active = true; } }       // nblk-1 is lane 0: lane 1 (a block beyond the frame) takes nblk-2
	}
	for (int i = lane; i < 512; i += 64) s_pal[i] = A.pal[i];
	__syncthreads();
	if (!active) blk = 0;
	const uint32_t by = blk / A.bw, bx = blk - by * A.bw;
	const uint32_t poff = by * 4 * A.w + bx * 4;
	const bool is_last = active && blk == last;
	uint32_t cur[16], icol[16];
	if (A.prev) load_block(A.prev, poff, A.w, cur);
	else {
#pragma unroll
		for (int k = 0; k < 16; k++) cur[k] = 0;
	}
	if (A.prev_iframe) load_block(A.prev_iframe, poff, A.w, icol);
	else {
#pragma unroll
		for (int k = 0; k < 16; k++) icol[k] = 0;
	}
	uint32_t stale = 0xFFFFu, istale = 0xFFFFu;                // per pixel, as in k_decode
	bool dep = false;
	for (uint32_t f = 0; f < A.n_frames; f++) {
		bool fill_written = false;
		const uint32_t own3 = cur[3], own3s = (stale >> 3) & 1u;
		if (active && blk < A.nentered[f]) {
			ByteSrc src{A.bits + (size_t)f * A.stride, (uint32_t)A.stride};
			const uint32_t o = BM ? bm_offset_of(A.vm, A.kb, A.maxR, A.bpos[f], f, blk) : A.offsets[(size_t)f * A.nblk + blk];
			decode_block<M512>(src, o, A.bpos[f], s_pal, cur, icol, istale, stale, fill_written);
		}
		const int nbl = nb_lane < 0 ? 0 : nb_lane;
		const uint32_t left = (uint32_t)__builtin_amdgcn_readlane((int)cur[7], nbl);   // img_data[(x-1)+(y+1)*w] of the left neighbour
		const uint32_t lefts = ((uint32_t)__builtin_amdgcn_readlane((int)stale, nbl) >> 7) & 1u;
		if (is_last && fill_written) {
			const uint32_t c = A.bw == 1 ? own3 : left;            // one block per row: see k_decode
#pragma unroll
			for (int k = 0; k < 16; k++) cur[k] = c;
			stale = (A.bw == 1 ? own3s : lefts) ? 0xFFFFu : 0u;
		}
		if (((A.first_fc + f) & 3u) == 0) {
#pragma unroll
			for (int k = 0; k < 16; k++) icol[k] = cur[k];
			istale = stale;
		}
		if (active) store_block(A.out + (size_t)f * npx, poff, A.w, cur);
		if (active && stale) dep = true;
	}
	if (dep) A.dirty[nwords + 1] = 1u;                         // the batch depends on the decoder state before it
}

static int check_slab(const uint8_t* d_bits, size_t stride)
{
	if ((stride & 3u) || stride < 4 || ((uintptr_t)d_bits & 3u)) return agmv_hip_err("agmv_hip: bitstream slab and stride must be 4-byte aligned");
	return 0;
}

// these rows of a batch, one frame per row: its bitstream in the slab, bpos[], nentered[] and (two-call form) nblk offsets[]
struct DecRows {
	const uint8_t* bits;
	size_t stride;
	const uint32_t* bpos;
	uint32_t *offsets, *nentered;   // offsets == NULL: the bitmap form
	uint32_t n_frames, nblk;
};
static DecRows rows_range(DecRows r, uint32_t f0, uint32_t f1)   // rows [f0, f1)
{
	r.bits += (size_t)f0 * r.stride; r.bpos += f0; r.nentered += f0; r.n_frames = f1 - f0;
	if (r.offsets) r.offsets += (size_t)f0 * r.nblk;
	return r;
}
// where the rows' pixels go and the decoder state they continue from
struct DecPix {
	uint32_t w, h, first_fc;
	uint32_t* out;
	const uint32_t *prev, *prev_iframe;
};

// words of the context's bitmap of positions to repair: the bitmap + the "anything to repair" word + the "depends on the prior state" word
static uint32_t dirty_words(uint32_t nblk) { return (nblk + 31) / 32 + 2; }

enum ParseMode { PARSE_FAST, PARSE_ROBUST, PARSE_SERIAL };
static ParseMode parse_mode()                                  // AGMV_HIP_PARSE (include/agmv_hip.h), read by every call
{
	const char* m = getenv("AGMV_HIP_PARSE");
	return !m ? PARSE_FAST : strcmp(m, "robust") == 0 ? PARSE_ROBUST : strcmp(m, "serial") == 0 ? PARSE_SERIAL : PARSE_FAST;
}

// width of a parser grid whose rows are frames: one wave per workgroup, each striding over the chunks or regions of one
// frame (at most `cap` of them are worth a workgroup): ~512 waves per CU in the grid (measured on 1024 x 1080p:
// 8 / 16 / 32 / 64 / 128 / 256 per frame -> 2.85 / 2.30 / 1.96 / 1.87 / 1.83 / 1.84 ms)
static uint32_t parse_grid_x(agmv_hip_ctx* c, uint32_t n_frames, size_t cap)
{
	uint32_t gx = (uint32_t)(((size_t)c->n_cu * 512 + n_frames - 1) / n_frames);
	if (gx < 32) gx = 32;
	if (gx > 256) gx = 256;
	if (gx > cap) gx = (uint32_t)cap;
	return gx < 1 ? 1 : gx;
}

// the robust parser kernels over the rows r on stream s (workspace of the context, sized for ws_frames rows: launches that
// share it must be ordered); fstate != NULL: only the frames marked FS_BAD (nbad of them); vm != NULL: entry bits, no offsets[]
static int parse_launch_robust(agmv_hip_ctx* c, const DecRows& r, size_t ws_frames, hipStream_t s,
                               const uint32_t* fstate, const uint32_t* nbad, unsigned long long* vm, uint32_t maxR)
{
	const size_t cpf = (r.stride + PC) / PC, maxchunks = cpf * ws_frames;
	if (maxchunks >> 32) return agmv_hip_err("agmv_hip: parser batch too large (%zu chunk rows)", maxchunks);
	dec_ws* d = dec_area(c);
	CK(agmv_hip_dev_grow(&d->d_parse_ws, &d->parse_ws_cap, (maxchunks + (maxchunks * 33 + 1) / 2 + 16) * 4, 1));   // dwords: centry | summ (u16)
	ParseArgs A;
	memset(&A, 0, sizeof(A));
	A.bits = r.bits; A.stride = r.stride; A.bpos = r.bpos; A.offsets = r.offsets; A.nentered = r.nentered;
	A.cpf = (uint32_t)cpf; A.centry = d->d_parse_ws; A.summ = (uint16_t*)(A.centry + maxchunks);
	A.n_frames = r.n_frames; A.nblk = r.nblk; A.fstate = fstate; A.vm = vm; A.maxR = maxR; A.nbad = nbad;
	// the exception path (fstate): a few rows of workgroups, 32 wide, stride over the frames and leave those that are not
	// FS_BAD at once -- with one row per frame the three gated launches cost 0.03 ms per 1024 frames for zero frames to parse
	const uint32_t n = r.n_frames;
	const dim3 grid(parse_grid_x(c, n, fstate && cpf > 32 ? 32 : cpf), fstate ? (n < 64u ? n : 64u) : (n < 65535u ? n : 65535u));
	const int m512 = c->mode512;
	DEC_LAUNCH(k_parse_chunks, grid, dim3(64), s, A, m512);
	hipLaunchKernelGGL(k_parse_stitch, dim3(fstate ? (n < 1024u ? n : 1024u) : n), dim3(64), 0, s, A);
	CK(hipGetLastError());
	DEC_LAUNCH(k_parse_emit, grid, dim3(64), s, A, m512);
	return 0;
}

// the parser: speculative walks proven per frame (k_fp_*), the robust kernels for the frames that could not be proven.
// AGMV_HIP_PARSE=robust runs the robust kernels alone.  bm != NULL: the bitmap form (no offsets[]) for these arguments of
// k_decode -- their bitmap of positions to repair is cleared; entry bitmaps, first block per region, tile entries come back.
// fstate != NULL: the frame states go there (n_frames words of the caller's) and not into the workspace
static int parse_launch(agmv_hip_ctx* c, const DecRows& r, size_t ws_frames, hipStream_t s, DecArgs* bm, uint32_t* fstate = nullptr)
{
	const bool robust_only = parse_mode() == PARSE_ROBUST;
	const uint32_t n_frames = r.n_frames;
	dec_ws* d = dec_area(c);
	d->d_fp_fstate = nullptr; d->fp_frames = 0;
	if (!bm && (n_frames > 65535u || robust_only)) return parse_launch_robust(c, r, ws_frames, s, nullptr, nullptr, nullptr, 0);
	if (n_frames > 65535u) return agmv_hip_err("agmv_hip: more than 65535 frames in one parser launch");
	const size_t maxR = (r.stride + FRB - 1) / FRB + 1, nreg = maxR * ws_frames;
	const uint32_t tpfd = (r.nblk + DEC_T - 1) / DEC_T;
	const size_t b_rec = nreg * sizeof(uint4), b_vm = nreg * FOWN * 8, b_kb = nreg * 4, b_fs = ((ws_frames * 4 + 15) & ~(size_t)15);
	const size_t b_tx = bm ? (((size_t)ws_frames * (tpfd + 1) * 4 + 15) & ~(size_t)15) : 0;
	CK(agmv_hip_dev_grow(&d->d_fp_ws, &d->fp_ws_cap, b_rec + b_vm + b_kb + b_fs + b_tx + 16, 1));
	FpArgs A;
	memset(&A, 0, sizeof(A));
	A.bits = r.bits; A.stride = r.stride; A.bpos = r.bpos; A.offsets = r.offsets; A.nentered = r.nentered;
	uint8_t* w = (uint8_t*)d->d_fp_ws;
	A.rec = (uint4*)w; A.vm = (unsigned long long*)(w + b_rec); A.kb = (uint32_t*)(w + b_rec + b_vm); A.fstate = (uint32_t*)(w + b_rec + b_vm + b_kb);
	if (fstate) A.fstate = fstate;
	A.tidx = bm ? (uint32_t*)(w + b_rec + b_vm + b_kb + b_fs) : nullptr; A.tpfd = tpfd;
	A.nbad = (uint32_t*)(w + b_rec + b_vm + b_kb + b_fs + b_tx);
	A.n_frames = n_frames; A.nblk = r.nblk; A.maxR = (uint32_t)maxR;
	if (bm) { A.dirty = bm->dirty; A.ndirty = dirty_words(r.nblk); }
	uint32_t gx = parse_grid_x(c, n_frames, maxR);
	// many small frames (8192 x 320x240: 7 regions each): one row of gx workgroups per frame would launch a quarter of a million
	// one-wave workgroups of which most find nothing to do; the rows stride over the frames instead
	uint32_t gy = n_frames;
	if ((size_t)gx * gy > 131072u) {
		const uint32_t want = (uint32_t)(((size_t)r.stride / 8 + FRB - 1) / FRB) + 1;   // regions of a frame whose stream is an eighth of the worst case
		if (gx > want) gx = want;
		if ((size_t)gx * gy > 131072u) gy = 131072u / gx;
	} else if (bm) {
		// A long range of large frames (bitmap form; k_fp_expand was not measured): as wide as a frame whose stream is an
		// eighth of the geometry's worst case (agmv_hip_max_usize; not the caller's stride, which changes with the slab's
		// padding) has regions -- 143 columns for 1080p, 512 colours, where parse_grid_x gives 256 -- wherever that grid
		// still holds four waves for every wave slot of the device, so that its tail stays short.  Measured at 512 x 1080p
		// (profiles/parser_staging/): k_fp_walk 142 -> 131 us and k_fp_tiles 24.8 -> 21.4 us on the synthetic clip (117 regions
		// a frame: one turn per workgroup as before), 396 -> 386 and 48.3 -> 45.2 on NORMAL-heavy content (356 regions: three
		// turns instead of two).  Frames of more regions than that (up to 1133 at 1080p: eight turns instead of five) were not measured.
		const size_t worst = (size_t)r.nblk * (c->mode512 ? 33 : 17) + 64;
		const uint32_t want = (uint32_t)((worst / 8 + FRB - 1) / FRB) + 1;
		if (gx > want && (size_t)want * gy >= (size_t)c->n_cu * 32 * 4) gx = want;
	}
	const dim3 grid(gx, gy);
	if (robust_only) {                                         // debugging aid: every frame through the robust kernels (bitmap form)
		CK(hipMemsetAsync(A.tidx, 0xFF, (size_t)n_frames * (tpfd + 1) * 4, s));   // TIDX_NONE (otherwise k_fp_finish's job; nbad: k_fp_walk's)
		// k_parse_chunks clears the entry bitmap words up to a frame's last chunk, k_fp_tiles / k_decode read up to the end of
		// its last region: without k_fp_walk (which writes every word of a region) the words in between are cleared here
		CK(hipMemsetAsync(A.vm, 0, (size_t)n_frames * maxR * FOWN * 8, s));
		CK(hipMemsetD32Async((hipDeviceptr_t)A.fstate, (int)FS_BAD, n_frames, s));
		CK(hipMemsetD32Async((hipDeviceptr_t)A.nbad, (int)n_frames, 1, s));
	} else {
		DEC_LAUNCH(k_fp_walk, grid, dim3(64), s, A, c->mode512);
		DEC_LAUNCH(k_fp_finish, dim3(n_frames), dim3(64), s, A, c->mode512);
	}
	d->d_fp_fstate = A.fstate; d->fp_frames = n_frames;
	if (!bm) {
		hipLaunchKernelGGL(k_fp_expand, dim3(gx, n_frames), dim3(64), 0, s, A);   // one row per frame (a quarter / an eighth of gx: 0.179 / 0.188 against 0.169 ms per 256 frames)
		CK(hipGetLastError());
		return parse_launch_robust(c, r, ws_frames, s, A.fstate, A.nbad, nullptr, 0);
	}
	// bitmap form: the frames that could not be proven get their entry BITS from the robust kernels, are counted and
	// numbered by k_fp_tiles, which then looks up every frame's tile entries
	bm->vm = A.vm; bm->kb = A.kb; bm->tidx = A.tidx; bm->maxR = A.maxR;
	if (parse_launch_robust(c, r, ws_frames, s, A.fstate, A.nbad, A.vm, A.maxR)) return -1;
	hipLaunchKernelGGL(k_fp_tiles, dim3(gx / 2 ? gx / 2 : 1, gy), dim3(64), 0, s, A);
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_parse_frames_dev(agmv_hip_ctx* c, const uint8_t* d_bits, size_t stride, const uint32_t* d_bpos,
                                         uint32_t n_frames, uint32_t w, uint32_t h, uint32_t* d_offsets, uint32_t* d_nentered,
                                         void* stream)
{
	if (need_dec_ctx(c, true)) return -1;
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (n_frames == 0) return 0;
	const DecRows r = {d_bits, stride, d_bpos, d_offsets, d_nentered, n_frames, (w / 4) * (h / 4)};
	hipStream_t s = (hipStream_t)stream;
	if (parse_mode() == PARSE_SERIAL) {                        // debugging aid: one lane per frame
		hipLaunchKernelGGL(k_parse_serial, dim3((n_frames + 63) / 64), dim3(64), 0, s, d_bits,
		                   (unsigned long long)stride, d_bpos, n_frames, r.nblk, c->mode512, d_offsets, d_nentered);
		CK(hipGetLastError());
		return 0;
	}
	if (check_slab(d_bits, stride)) return -1;
	agmv_hip_ev_mark(c, 2, s);
	if (parse_launch(c, r, n_frames, s, nullptr)) return -1;
	agmv_hip_ev_mark(c, 3, s);
	return 0;
}

extern "C" int agmv_hip_parse_fallback_frames(agmv_hip_ctx* c, void* stream)
{
	if (need_dec_ctx(c, false)) return -1;
	const dec_ws* d = dec_area(c);
	if (!d || !d->d_fp_fstate || d->fp_frames == 0) return 0;
	CK(hipStreamSynchronize((hipStream_t)stream));
	uint32_t* h = (uint32_t*)malloc((size_t)d->fp_frames * 4);
	if (!h) return agmv_hip_err("agmv_hip: out of host memory");
	if (hipMemcpy(h, d->d_fp_fstate, (size_t)d->fp_frames * 4, hipMemcpyDeviceToHost) != hipSuccess) { free(h); agmv_hip_err("agmv_hip: D2H failed"); return -1; }
	int n = 0;
	for (uint32_t i = 0; i < d->fp_frames; i++) n += h[i] != FS_OK;
	free(h);
	return n;
}

// arguments of k_decode / k_fixup for the rows r; grows the context's bitmap of positions to repair and, unless the
// caller has that done (k_fp_tiles), clears it.  The context holds TWO sets of those words.  Range 0 of a call cut into ranges
// takes the second (`second`): its "depends on the prior state" word is the call's, and the later ranges, which depend on
// the ranges before them and not on the caller, clear and write the first set only
static int decode_prepare(agmv_hip_ctx* c, DecArgs& A, const DecRows& r, const DecPix& px, hipStream_t s, bool clear, bool second = false)
{
	if (((uintptr_t)px.out & 15u) || ((uintptr_t)px.prev & 15u) || ((uintptr_t)px.prev_iframe & 15u)) return agmv_hip_err("agmv_hip: pixel buffers must be 16-byte aligned");
	if (check_slab(r.bits, r.stride)) return -1;
	memset(&A, 0, sizeof(A));
	A.bits = r.bits; A.stride = r.stride; A.bpos = r.bpos; A.offsets = r.offsets; A.nentered = r.nentered;
	A.out = px.out; A.pal = c->d_pal; A.prev = px.prev; A.prev_iframe = px.prev_iframe;
	A.n_frames = r.n_frames; A.w = px.w; A.h = px.h; A.bw = px.w / 4; A.nblk = r.nblk;
	A.tpf = (A.nblk + DEC_T - 1) / DEC_T;
	A.first_fc = px.first_fc; A.phase = px.first_fc & 3u; A.n_groups = (r.n_frames + A.phase + 3) / 4;
	const size_t nwords = dirty_words(A.nblk);
	dec_ws* d = dec_area(c);
	CK(agmv_hip_dev_grow(&d->d_dirty, &d->dirty_cap, 2 * nwords * 4, 1));
	A.dirty = d->d_dirty + (second ? nwords : 0); d->dep_split = false;
	if (clear) CK(hipMemsetAsync(A.dirty, 0, nwords * 4, s));
	return 0;
}

static int decode_launch(agmv_hip_ctx* c, DecArgs A, uint32_t g0, uint32_t g1, hipStream_t s)   // GOPs [g0, g1) of the batch
{
	A.grp0 = g0; A.n_items = (g1 - g0) * A.tpf;
	uint32_t nwg = A.n_items;
	if (const char* e = getenv("AGMV_DEC_GRID")) {             // tuning / test aid: at most n workgroups, each looping over its items
		const long n = atol(e);
		if (n > 0 && (unsigned long)n < nwg) nwg = (uint32_t)n;
	}
	DEC_LAUNCH(k_decode, dim3(nwg), dim3(DEC_T), s, A, c->mode512, A.vm != nullptr, nwg < A.n_items);   // <mode512, bitmap form, looping>
	return 0;
}

static int fixup_launch(agmv_hip_ctx* c, const DecArgs& A, hipStream_t s)
{
	DEC_LAUNCH(k_fixup, dim3((A.nblk + 63) / 64), dim3(64), s, A, c->mode512, A.vm != nullptr);   // <mode512, bitmap form>
	return 0;
}

extern "C" int agmv_hip_decode_frames_dev(agmv_hip_ctx* c, const uint8_t* d_bits, size_t stride, const uint32_t* d_bpos,
                                          const uint32_t* d_offsets, const uint32_t* d_nentered, uint32_t n_frames,
                                          uint32_t w, uint32_t h, uint32_t first_fc, uint32_t* d_out,
                                          const uint32_t* d_prev, const uint32_t* d_prev_iframe, void* stream)
{
	if (need_dec_ctx(c, true)) return -1;
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (n_frames == 0) return 0;
	hipStream_t s = (hipStream_t)stream;
	const DecRows r = {d_bits, stride, d_bpos, const_cast<uint32_t*>(d_offsets), const_cast<uint32_t*>(d_nentered), n_frames, (w / 4) * (h / 4)};   // (only read: no parser runs here)
	const DecPix px = {w, h, first_fc, d_out, d_prev, d_prev_iframe};
	DecArgs A;
	if (decode_prepare(c, A, r, px, s, true)) return -1;
	agmv_hip_ev_mark(c, 4, s);
	if (decode_launch(c, A, 0, A.n_groups, s)) return -1;
	if (fixup_launch(c, A, s)) return -1;
	agmv_hip_ev_mark(c, 5, s);
	return 0;
}

// Parse + reconstruct as ONE call; optionally (AGMV_DEC_SLICES=n) cut into n ranges of GOPs with the parser on a stream of
// the context's own, so that the parse of range k+1 runs beside the reconstruction of range k (k_fixup needs every
// frame's offsets and runs last).  Measured (profiles/r02/k_decode_experiments.txt): the kernels do run side by side but
// take from each other what they gain -- k_decode needs its full occupancy -- so the default is one range.
extern "C" int agmv_hip_parse_decode_frames_dev(agmv_hip_ctx* c, const uint8_t* d_bits, size_t stride, const uint32_t* d_bpos,
                                                uint32_t n_frames, uint32_t w, uint32_t h, uint32_t first_fc,
                                                uint32_t* d_offsets, uint32_t* d_nentered, uint32_t* d_out,
                                                const uint32_t* d_prev, const uint32_t* d_prev_iframe, void* stream)
{
	if (need_dec_ctx(c, true)) return -1;
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (n_frames == 0) return 0;
	hipStream_t s = (hipStream_t)stream;
	const DecRows r = {d_bits, stride, d_bpos, d_offsets, d_nentered, n_frames, (w / 4) * (h / 4)};
	const DecPix px = {w, h, first_fc, d_out, d_prev, d_prev_iframe};
	DecArgs A;
	if (decode_prepare(c, A, r, px, s, true)) return -1;
	uint32_t nsl = 1;
	if (getenv("AGMV_DEC_SLICES")) nsl = (uint32_t)atoi(getenv("AGMV_DEC_SLICES"));
	if (nsl > A.n_groups) nsl = A.n_groups;
	if (nsl > (uint32_t)DEC_MAX_SLICES) nsl = DEC_MAX_SLICES;
	if (nsl < 1) nsl = 1;
	const uint32_t gps = (A.n_groups + nsl - 1) / nsl;         // GOPs per range
	auto first_frame = [&](uint32_t g) -> uint32_t { const long f = (long)g * 4 - (long)A.phase; return f < 0 ? 0u : ((uint32_t)f > n_frames ? n_frames : (uint32_t)f); };
	const size_t ws_frames = (size_t)gps * 4;
	agmv_hip_ev_mark(c, 6, s);
	if (nsl == 1) {
		if (parse_launch(c, r, n_frames, s, nullptr)) return -1;
		if (decode_launch(c, A, 0, A.n_groups, s)) return -1;
	} else {
		dec_ws* d = dec_area(c);
		if (!d->aux_stream) {
			CK(hipStreamCreateWithFlags(&d->aux_stream, hipStreamNonBlocking));
			CK(hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming));
			for (int i = 0; i < DEC_MAX_SLICES; i++) CK(hipEventCreateWithFlags(&d->ev_slice[i], hipEventDisableTiming));
		}
		CK(hipEventRecord(d->ev_fork, s));                     // the bitstreams are complete on the caller's stream
		CK(hipStreamWaitEvent(d->aux_stream, d->ev_fork, 0));
		uint32_t k = 0;
		for (uint32_t g0 = 0; g0 < A.n_groups; g0 += gps, k++) {
			const uint32_t g1 = g0 + gps < A.n_groups ? g0 + gps : A.n_groups;
			if (parse_launch(c, rows_range(r, first_frame(g0), first_frame(g1)), ws_frames, d->aux_stream, nullptr)) return -1;
			CK(hipEventRecord(d->ev_slice[k], d->aux_stream));
			CK(hipStreamWaitEvent(s, d->ev_slice[k], 0));
			if (decode_launch(c, A, g0, g1, s)) return -1;
		}
	}
	if (fixup_launch(c, A, s)) return -1;
	agmv_hip_ev_mark(c, 7, s);
	return 0;
}

// Frames per range of agmv_hip_decode_bitstreams_dev: as many whole GOPs as decode to at most DEC_RANGE_PIXEL_BYTES of
// pixels, at least one; 0 = cut only where the parser's grid makes it (65532 frames).  Derived from what the host knows: the
// stream sizes live on the device.  AGMV_DEC_RANGE_FRAMES=n (read per call, a test and tuning aid) forces n frames, rounded
// up to whole GOPs; 0 = never cut below 65532.
// The constant is 512 frames of 1920x1080: on the 1024 x 1080p clip (profiles/decode_ranges/sweep.txt, row "synth ... range
// 512") parser + k_decode + k_fixup take 1.870 ms against 2.093 ms uncut, 1.932 / 1.990 ms with 256 / 340 frames and 1.932 with
// 768 -- k_decode is as fast as with 256 (1.49 ms: a range's streams, 223 MB, are still in the 256 MiB memory-side cache behind
// its parser) and the parser pays for one extra set of launches, not three.  In bytes of pixels, not frames, so that other
// frame sizes are cut at the same footprint (rows "range -1"): a fixed frame count costs small frames a parser round each.
constexpr uint32_t DEC_PART_MAX = 65532u;                      // a multiple of 4: the parser's grid has one row per frame
constexpr size_t DEC_RANGE_PIXEL_BYTES = (size_t)512 * 1920 * 1080 * 4;
static uint32_t dec_range_frames(uint32_t w, uint32_t h)
{
	size_t n = DEC_PART_MAX;
	if (const char* e = getenv("AGMV_DEC_RANGE_FRAMES")) {
		const long v = atol(e);
		if (v > 0) n = ((size_t)v + 3) & ~(size_t)3;
	} else if (DEC_RANGE_PIXEL_BYTES) {
		const size_t gops = DEC_RANGE_PIXEL_BYTES / ((size_t)w * h * 16);
		n = (gops ? gops : 1) * 4;
	}
	return n < DEC_PART_MAX ? (uint32_t)n : DEC_PART_MAX;
}

// Parse + reconstruct without offsets[]: the parser's entry bitmaps go straight to k_decode, which ranks its own blocks in
// them (k_fp_tiles tells every tile where it starts).  Against agmv_hip_parse_decode_frames_dev this drops k_fp_expand and
// the 4 bytes per block it writes and k_decode reads back.  A batch longer than dec_range_frames() is cut at GOP
// boundaries into ranges that run one after the other on the caller's stream -- parser, k_decode, k_fixup -- so that
// k_decode finds the streams its parser has just read still in the memory-side cache, and the parser's work areas are one
// range long; each range continues from the decoder state the range before it left.
extern "C" int agmv_hip_decode_bitstreams_dev(agmv_hip_ctx* c, const uint8_t* d_bits, size_t stride, const uint32_t* d_bpos,
                                              uint32_t n_frames, uint32_t w, uint32_t h, uint32_t first_fc,
                                              uint32_t* d_nentered, uint32_t* d_out,
                                              const uint32_t* d_prev, const uint32_t* d_prev_iframe, void* stream)
{
	if (need_dec_ctx(c, true)) return -1;
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (n_frames == 0) return 0;
	hipStream_t s = (hipStream_t)stream;
	dec_ws* d = dec_area(c);
	if (!d_nentered) {
		CK(agmv_hip_dev_grow(&d->d_nent_own, &d->nent_cap, (size_t)n_frames * 4, 1));
		d_nentered = d->d_nent_own;
	}
	const DecRows all = {d_bits, stride, d_bpos, nullptr, d_nentered, n_frames, (w / 4) * (h / 4)};
	const size_t npx = (size_t)w * h;
	const uint32_t range = dec_range_frames(w, h);
	const bool cut = n_frames > range;
	const size_t ws_frames = (size_t)range + 3;                // the longest range: a first one with the frames of a GOP cut short in front
	uint32_t* fstate = nullptr;                                // cut: the frame states of every range, for agmv_hip_parse_fallback_frames
	if (cut) {
		CK(agmv_hip_dev_grow(&d->d_fstate_call, &d->fstate_call_cap, (size_t)n_frames * 4, 1));
		fstate = d->d_fstate_call;
	}
	// timing marks: one per boundary (the end of a parser is the start of its k_decode, the end of a range the start of the
	// next, the first and the last are the call's)
	int k = 0;
	for (uint32_t f0 = 0; f0 < n_frames; k++) {
		uint32_t f1 = n_frames;
		if (f1 - f0 > range) {
			f1 = f0 + range; f1 -= (first_fc + f1) & 3u;           // the next range starts with an I-frame
			// ... and never with the batch's first one (a range of one GOP, a batch that starts inside a GOP): it would take the
			// caller's I-frame snapshot, and the call's prior dependence is range 0's alone -- that GOP rides with range 0
			if (f1 < 4) f1 = f1 + 4 < n_frames ? f1 + 4 : n_frames;
		}
		const DecRows r = rows_range(all, f0, f1);
		// state before frame f0: the frame before it, and the snapshot taken at the last I-frame (the decoded I-frame itself, :401-405)
		const DecPix px = {w, h, first_fc + f0, d_out + (size_t)f0 * npx, f0 == 0 ? d_prev : d_out + (size_t)(f0 - 1) * npx,
		                   f0 == 0 ? d_prev_iframe : d_out + (size_t)(f0 - 4) * npx};
		DecArgs A;
		if (decode_prepare(c, A, r, px, s, false, cut && f0 == 0)) return -1;
		if (agmv_hip_ev_mark_seq(c, 2 * k, s)) return -1;     // (k > 0: also the end of the range before)
		// work areas sized for the longest range, not for this one: growing them in mid-call would wait for the device
		if (parse_launch(c, r, cut ? ws_frames : r.n_frames, s, &A, fstate ? fstate + f0 : nullptr)) return -1;   // fills in A.vm, A.kb, A.tidx, A.maxR
		if (agmv_hip_ev_mark_seq(c, 2 * k + 1, s)) return -1;
		if (decode_launch(c, A, 0, A.n_groups, s)) return -1;
		if (fixup_launch(c, A, s)) return -1;
		f0 = f1;
	}
	if (agmv_hip_ev_mark_seq(c, 2 * k, s)) return -1;
	d->dep_split = cut;
	if (cut) { d->d_fp_fstate = fstate; d->fp_frames = n_frames; }
	return 0;
}

extern "C" int agmv_hip_decode_prior_dependent(agmv_hip_ctx* c, uint32_t w, uint32_t h, void* stream)
{
	if (need_dec_ctx(c, false)) return -1;
	const dec_ws* d = dec_area(c);
	if (!d || !d->d_dirty) return agmv_hip_err("agmv_hip: no decode has run on this context");
	const size_t nblk = (size_t)(w / 4) * (h / 4);
	uint32_t v = 0;
	CK(hipStreamSynchronize((hipStream_t)stream));
	CK(hipMemcpy(&v, d->d_dirty + (d->dep_split ? dirty_words((uint32_t)nblk) : 0u) + (nblk + 31) / 32 + 1, 4, hipMemcpyDeviceToHost));
	return v ? 1 : 0;
}

extern "C" int agmv_hip_decode_frames(agmv_hip_ctx* c, const uint8_t* h_bits, size_t stride, const uint32_t* h_bpos,
                                      uint32_t n_frames, uint32_t w, uint32_t h, uint32_t first_fc, uint32_t* h_out,
                                      const uint32_t* h_prev, const uint32_t* h_prev_iframe)
{
	if (need_dec_ctx(c, true)) return -1;
	if (agmv_hip_check_geometry(w, h)) return -1;
	if (n_frames == 0) return 0;
	const size_t npx = (size_t)w * h, nblk = npx / 16;
	uint8_t* d_bits = nullptr;
	uint32_t *d_bpos = nullptr, *d_off = nullptr, *d_ne = nullptr, *d_out = nullptr, *d_prev = nullptr, *d_pi = nullptr;
	int rc = -1;
	do {
		if (hipMalloc(&d_bits, stride * n_frames) != hipSuccess || hipMalloc(&d_bpos, 4 * (size_t)n_frames) != hipSuccess ||
		    hipMalloc(&d_off, 4 * nblk * n_frames) != hipSuccess || hipMalloc(&d_ne, 4 * (size_t)n_frames) != hipSuccess ||
		    hipMalloc(&d_out, 4 * npx * n_frames) != hipSuccess || (h_prev && hipMalloc(&d_prev, 4 * npx) != hipSuccess) ||
		    (h_prev_iframe && hipMalloc(&d_pi, 4 * npx) != hipSuccess)) {
			agmv_hip_err("agmv_hip: device allocation failed"); break;
		}
		if (hipMemcpy(d_bits, h_bits, stride * n_frames, hipMemcpyHostToDevice) != hipSuccess ||
		    hipMemcpy(d_bpos, h_bpos, 4 * (size_t)n_frames, hipMemcpyHostToDevice) != hipSuccess ||
		    (h_prev && hipMemcpy(d_prev, h_prev, 4 * npx, hipMemcpyHostToDevice) != hipSuccess) ||
		    (h_prev_iframe && hipMemcpy(d_pi, h_prev_iframe, 4 * npx, hipMemcpyHostToDevice) != hipSuccess)) {
			agmv_hip_err("agmv_hip: H2D failed"); break;
		}
		if (agmv_hip_parse_frames_dev(c, d_bits, stride, d_bpos, n_frames, w, h, d_off, d_ne, nullptr)) break;
		if (agmv_hip_decode_frames_dev(c, d_bits, stride, d_bpos, d_off, d_ne, n_frames, w, h, first_fc, d_out, d_prev, d_pi, nullptr)) break;
		if (hipMemcpy(h_out, d_out, 4 * npx * n_frames, hipMemcpyDeviceToHost) != hipSuccess) { agmv_hip_err("agmv_hip: D2H failed"); break; }
		rc = 0;
	} while (0);
	(void)hipFree(d_bits); (void)hipFree(d_bpos); (void)hipFree(d_off); (void)hipFree(d_ne); (void)hipFree(d_out); (void)hipFree(d_prev); (void)hipFree(d_pi);
	return rc;
}

