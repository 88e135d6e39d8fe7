// libagmv_amd/csrc/agmv_palette_hip.hip -- the palette refinement: weighted k-means (Lloyd's algorithm) over the histogram of
// AGMV_QuantizeColor codes, agmv_hip_palette_refine_dev of include/agmv_hip.h.  include/agmv.h ("palette refinement") holds
// the definition; tests/palette_cases.py states it in numpy.
//
//   k_pal_assign   one lane per bin of the histogram.  A lane whose bin is empty drops out; the others walk the k centroids,
//                  which sit in LDS and are read as broadcasts (every lane of a wave reads centroid j at the same time), keep the
//                  nearest (strict <, so the lowest index wins a tie) and add w, w*R, w*G, w*B to the workgroup's partial sums
//                  with 64-bit LDS atomics.  The 256 bins of a workgroup are neighbours in colour and fall into a few
//                  clusters, so a workgroup flushes only the clusters it touched, with 64-bit global atomic adds.
//   k_pal_update   one workgroup, one lane per centroid: divide, round half up, compare with the old colour, count the round,
//                  raise the "converged" flag, publish the distortion and clear the sums for the next pass.
// Integer adds commute: the result is exact and the same from run to run.  No float anywhere.
// The host enqueues iterations + 1 pairs of launches and never waits: once the flag is up every later launch returns at once.
// Pass p measures the distortion of the centroids of round p's start, so the last pass (update with `last`) only measures.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "agmv_hip_impl.h"

constexpr uint32_t PAL_MAX_K = 512;
constexpr uint32_t PAL_T = 256;                // lanes, and bins, of a k_pal_assign workgroup
constexpr uint32_t PAL_MAX_ITERATIONS = 4096;  // 2 * (iterations + 1) launches are enqueued per call

// the work area of a context: the sums of one pass (cluster j: w*R, w*G, w*B, w), its distortion and the flag
struct pal_ws {
	unsigned long long acc[PAL_MAX_K * 4];
	unsigned long long sse;
	uint32_t done;
	uint32_t pad;
};

// the centre of the bin of an AGMV_QuantizeColor code: AGMV_ReverseQuantizeColor plus half a step per channel
__device__ __forceinline__ void bin_centre(uint32_t code, int quality, int& r, int& g, int& b)
{
	if (quality == 2) { r = (int)((code >> 12) & 31) * 8 + 4; g = (int)((code >> 6) & 63) * 4 + 2; b = (int)(code & 63) * 4 + 2; }         // MID
	else if (quality == 3) { r = (int)((code >> 11) & 31) * 8 + 4; g = (int)((code >> 5) & 63) * 4 + 2; b = (int)(code & 31) * 8 + 4; }   // LOW
	else { r = (int)((code >> 13) & 63) * 4 + 2; g = (int)((code >> 7) & 63) * 4 + 2; b = (int)(code & 127) * 2 + 1; }                    // HIGH
}

// grid: n_codes / PAL_T workgroups (n_codes is 2^19, 2^17 or 2^16: every lane has a bin)
__global__ __launch_bounds__(PAL_T) void k_pal_assign(const uint32_t* __restrict__ hist, int quality, const uint32_t* __restrict__ pal,
                                                      uint32_t k, pal_ws* __restrict__ ws)
{
	__shared__ uint32_t s_c[PAL_MAX_K];
	__shared__ unsigned long long s_acc[PAL_MAX_K * 4];
	__shared__ unsigned long long s_sse;
	if (ws->done) return;                                      // converged in an earlier pass (the same for every lane)
	const uint32_t w = hist[blockIdx.x * PAL_T + threadIdx.x];
	if (!__syncthreads_or(w != 0)) return;                     // a workgroup of empty bins
	for (uint32_t j = threadIdx.x; j < k; j += PAL_T) s_c[j] = pal[j];
	for (uint32_t j = threadIdx.x; j < k * 4; j += PAL_T) s_acc[j] = 0;
	if (threadIdx.x == 0) s_sse = 0;
	__syncthreads();
	if (w) {
		int r, g, b;
		bin_centre(blockIdx.x * PAL_T + threadIdx.x, quality, r, g, b);
		uint32_t best = 0xFFFFFFFFu, bj = 0;
		for (uint32_t j = 0; j < k; j++) {
			const uint32_t c = s_c[j];
			const int dr = r - (int)((c >> 16) & 0xff), dg = g - (int)((c >> 8) & 0xff), db = b - (int)(c & 0xff);
			const uint32_t d = (uint32_t)(dr * dr + dg * dg + db * db);
			if (d < best) { best = d; bj = j; }
		}
		atomicAdd(&s_acc[bj * 4 + 0], (unsigned long long)w * (uint32_t)r);
		atomicAdd(&s_acc[bj * 4 + 1], (unsigned long long)w * (uint32_t)g);
		atomicAdd(&s_acc[bj * 4 + 2], (unsigned long long)w * (uint32_t)b);
		atomicAdd(&s_acc[bj * 4 + 3], (unsigned long long)w);
		atomicAdd(&s_sse, (unsigned long long)w * best);
	}
	__syncthreads();
	for (uint32_t j = threadIdx.x; j < k; j += PAL_T) {
		if (s_acc[j * 4 + 3] == 0) continue;                   // no point of this workgroup fell into cluster j
		atomicAdd(&ws->acc[j * 4 + 0], s_acc[j * 4 + 0]);
		atomicAdd(&ws->acc[j * 4 + 1], s_acc[j * 4 + 1]);
		atomicAdd(&ws->acc[j * 4 + 2], s_acc[j * 4 + 2]);
		atomicAdd(&ws->acc[j * 4 + 3], s_acc[j * 4 + 3]);
	}
	if (threadIdx.x == 0) atomicAdd(&ws->sse, s_sse);
}

// one workgroup of PAL_MAX_K lanes; lane j owns centroid j
__global__ __launch_bounds__(PAL_MAX_K) void k_pal_update(uint32_t* __restrict__ pal, uint32_t k, uint32_t n_free, pal_ws* __restrict__ ws,
                                                          uint32_t* __restrict__ rounds, unsigned long long* __restrict__ sse, int first, int last)
{
	__shared__ uint32_t s_changed;
	const uint32_t j = threadIdx.x;
	if (ws->done) return;                                      // (nobody writes the flag before the barrier below)
	const unsigned long long e = ws->sse;
	if (j == 0) s_changed = 0;
	__syncthreads();
	if (!last && j < n_free) {
		const unsigned long long W = ws->acc[j * 4 + 3];
		if (W) {                                               // an empty cluster keeps its colour
			const uint32_t r = (uint32_t)((ws->acc[j * 4 + 0] + W / 2) / W), g = (uint32_t)((ws->acc[j * 4 + 1] + W / 2) / W),
			               b = (uint32_t)((ws->acc[j * 4 + 2] + W / 2) / W);
			const uint32_t c = r << 16 | g << 8 | b;
			if (c != (pal[j] & 0xFFFFFFu)) { pal[j] = c; s_changed = 1; }
		}
	}
	__syncthreads();
	if (j < k) { ws->acc[j * 4 + 0] = 0; ws->acc[j * 4 + 1] = 0; ws->acc[j * 4 + 2] = 0; ws->acc[j * 4 + 3] = 0; }
	if (j == 0) {
		if (first) sse[0] = e;
		sse[1] = e;                                            // of the centroids this pass started from: the final ones when it stops here
		ws->sse = 0;
		if (last || !s_changed) ws->done = 1;
		else rounds[0] += 1;
	}
}

// the context's area of this stage holds the device memory of a pass
struct pal_area { pal_ws* d; };

static void pal_area_free(void* p)
{
	(void)hipFree(((pal_area*)p)->d);
	free(p);
}

extern "C" int agmv_hip_palette_refine_dev(agmv_hip_ctx* c, const uint32_t* d_hist, int quality, uint32_t* d_pal, uint32_t k, uint32_t n_free,
                                           uint32_t iterations, uint32_t* d_rounds, uint64_t* d_sse, void* stream)
{
	if (!c) return agmv_hip_err("agmv_hip: NULL context");
	if (!d_hist || !d_pal || !d_rounds || !d_sse) return agmv_hip_err("agmv_hip_palette_refine_dev: NULL pointer");
	if (quality < 1 || quality > 3) return agmv_hip_err("agmv_hip_palette_refine_dev: quality %d is not 1 (HIGH), 2 (MID) or 3 (LOW)", quality);
	if (k < 1 || k > PAL_MAX_K) return agmv_hip_err("agmv_hip_palette_refine_dev: k = %u centroids, 1 .. %u are possible", k, PAL_MAX_K);
	if (n_free > k) return agmv_hip_err("agmv_hip_palette_refine_dev: n_free = %u exceeds k = %u", n_free, k);
	if (iterations > PAL_MAX_ITERATIONS) return agmv_hip_err("agmv_hip_palette_refine_dev: %u iterations, at most %u are possible", iterations, PAL_MAX_ITERATIONS);
	CK(hipSetDevice(c->device));
	pal_area* area = (pal_area*)agmv_hip_area(c, AREA_PALETTE, sizeof(pal_area), pal_area_free);
	if (!area) return -1;
	if (!area->d) CK(hipMalloc(&area->d, sizeof(pal_ws)));
	pal_ws* ws = area->d;
	const hipStream_t s = (hipStream_t)stream;
	const uint32_t n_codes = quality == 2 ? 1u << 17 : (quality == 3 ? 1u << 16 : 1u << 19);
	CK(hipMemsetAsync(ws, 0, sizeof(pal_ws), s));
	CK(hipMemsetAsync(d_rounds, 0, sizeof(uint32_t), s));
	for (uint32_t p = 0; p <= iterations; p++) {
		hipLaunchKernelGGL(k_pal_assign, dim3(n_codes / PAL_T), dim3(PAL_T), 0, s, d_hist, quality, (const uint32_t*)d_pal, k, ws);
		hipLaunchKernelGGL(k_pal_update, dim3(1), dim3(PAL_MAX_K), 0, s, d_pal, k, n_free, ws, d_rounds, (unsigned long long*)d_sse, p == 0, p == iterations);
	}
	CK(hipGetLastError());
	return 0;
}
