// libagmv_amd/csrc/agmv_hip_impl.h -- what the translation units of libagmv_hip.so share and include/agmv_hip.h does not show:
// the context, the error path, the entry prologue, the per-stage work areas, device-buffer growth, and the few kernel helpers
// that the encoder and the decoder both use.  Included by the .hip files only; what needs a definition has it in agmv_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "../../include/agmv_hip.h"

// ---- the context ----
// A stage's work area is a host struct that the stage defines; it is created by the stage's first call on the context, and
// agmv_hip_destroy frees it through the destructor registered with it.
enum agmv_hip_area_kind { AREA_DEC, AREA_LZSS, AREA_LZ77, AREA_LZ_DECODE, AREA_PALETTE, AREA_KINDS };

struct agmv_hip_ctx {
	int device;
	int mode512;
	int have_palette;
	uint16_t* d_lut;                // 2^24 entries
	uint32_t* d_mtx;                // 512 rows of the +-2 bit matrix
	uint32_t* d_pal;                // 512 colours (p0 | p1)
	struct lut_share* share;        // owner of the three tables above, private to agmv_hip.hip
	unsigned long long* d_status;   // look-back words
	size_t status_cap;              // in words
	uint32_t* d_ctrl;               // [0] ticket, [1] error, padded to 16 B
	uint16_t* d_ient_tmp;           // encode: I-frame entries written by a batch that also READS the caller's plane
	size_t ient_cap;                // in entries
	int enc_grid;                   // resident workgroups for the persistent encode kernel
	int n_cu;
	int timing;                     // record HIP events around the three hot kernels
	hipEvent_t ev[8];               // encode, parse, decode, parse||decode pipeline: start/stop
	hipEvent_t* ev_seq;             // agmv_hip_decode_bitstreams_dev: one mark per boundary -- [2k] in front of range k's parser, [2k + 1] between
	                                // it and the range's k_decode, [2n] behind the last k_fixup; grown on demand
	int ev_seq_cap;                 // ... events in the pool
	int ev_seq_n[3];                // ... ranges n whose marks hold the last parse / decode / whole-call times (0: ev[2..7] do)
	hipEvent_t ev_enc;              // end of the last encode launch (encodes of one context share status / control words)
	hipStream_t enc_stream;         // ... and the stream it went to
	int have_enc;
	uint32_t* d_nn_pal;             // agmv_hip_nearest: palette, pixels, entries (grown on demand)
	uint32_t* d_nn_pix;
	uint16_t* d_nn_ent;
	size_t nn_cap;
	void* ws[AREA_KINDS];           // the work areas, by kind
	void (*ws_free[AREA_KINDS])(void*);   // ... and what frees each (the device of the context is current)
};

// ---- errors: every message is the calling thread's agmv_hip_last_error() text; both functions return -1 ----
int agmv_hip_err(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int agmv_hip_hip_failed(const char* what, hipError_t e, const char* file, int line);
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return agmv_hip_hip_failed(#x, e_, __FILE_NAME__, __LINE__); } while (0)
#define CKP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { agmv_hip_hip_failed(#x, e_, __FILE_NAME__, __LINE__); return nullptr; } } while (0)

// ---- what opens an entry point: refuses a NULL context (and, with `palette`, one without a palette), then makes the
// context's device current ----
int agmv_hip_enter(agmv_hip_ctx* c, bool palette = false);

// The context's work area of a kind: `bytes` of zeroed host memory on first use, the same memory afterwards.
// NULL: out of host memory (the error text is set).
void* agmv_hip_area(agmv_hip_ctx* c, agmv_hip_area_kind kind, size_t bytes, void (*destroy)(void*));

void agmv_hip_ev_mark(agmv_hip_ctx* c, int which, hipStream_t s);   // a timing mark: encode 0/1, the decoder 2..7
// boundary `i` of a decode that runs parser, k_decode + k_fixup, parser, ... back to back (see ev_seq): ONE mark where an
// interval ends and the next begins.  Behind mark 2n, agmv_hip_last_kernel_ms(1..3) are the sums over the n ranges
int agmv_hip_ev_mark_seq(agmv_hip_ctx* c, int i, hipStream_t s);
int agmv_hip_check_geometry(uint32_t w, uint32_t h);

// Grow the device buffer *p of *cap units (of `unit` bytes) to at least `need` units.  The contents are not kept; on failure
// *p is null and *cap 0.  Buffers that share one capacity pass cap = nullptr: they are allocated anew, and their owner
// commits the capacity once all of them exist.
template <class T>
static inline hipError_t agmv_hip_dev_grow(T** p, size_t* cap, size_t need, size_t unit = sizeof(T))
{
	if (cap && need <= *cap) return hipSuccess;
	if (cap) *cap = 0;
	hipError_t e = hipFree(*p);
	*p = nullptr;
	if (e == hipSuccess) e = hipMalloc((void**)p, need * unit);
	if (e == hipSuccess && cap) *cap = need;
	return e;
}

// ---- kernel helpers of the encoder and the decoder ----
#define FILL_FLAG   0x4Eu   /* include/agmv_defines.h:49 */
#define NORMAL_FLAG 0x2Fu   /* :50 */
#define COPY_FLAG   0x5Eu   /* :51 */
#define FILL_COUNT  14u     /* :52 */
#define COPY_COUNT  13u     /* :53 */

// Workgroup barrier that orders LDS only.  __syncthreads() also carries a global-memory fence, i.e. an
// s_waitcnt vmcnt(0): every prefetch and every output store in flight would have to land before the barrier.
__device__ __forceinline__ void lds_barrier()
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Wave-wide scans on the VALU's DPP lanes (row shifts inside the 16-lane rows, then the two row broadcasts gfx9 has
// for exactly this) -- six dependent adds, no LDS round trips (__shfl_up compiles to ds_bpermute + a wait per step).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or0(uint32_t x)       // lanes without a source (or masked off) read 0
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xF, false);
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, int)
{
	x += dpp_or0<0x111, 0xF>(x);                               // row_shr:1
	x += dpp_or0<0x112, 0xF>(x);                               // row_shr:2
	x += dpp_or0<0x114, 0xF>(x);                               // row_shr:4
	x += dpp_or0<0x118, 0xF>(x);                               // row_shr:8
	x += dpp_or0<0x142, 0xA>(x);                               // row_bcast:15 -> rows 1 and 3
	x += dpp_or0<0x143, 0xC>(x);                               // row_bcast:31 -> rows 2 and 3
	return x;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)      // the same value in every lane
{
	return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(x, 0), 63);
}
