// libagmv_amd/csrc/agmv_audio_hip.hip -- audio tracks on the GPU: agmv_hip_audio_compand_async / agmv_hip_audio_expand_async of
// include/agmv_hip.h.  The arithmetic is agmv_audio.h's, the same functions the host library calls; include/agmv.h ("audio
// tracks") holds the definitions; tests/audio_cases.py states them in numpy.
//
// Streaming kernels: no LDS, no atomics, nothing kept between calls.  A track is cut into a head, a body of whole units of 16
// samples (per channel, for the planar layout) and a tail.  A lane takes one unit at a time: it reads and writes it with 16-byte
// accesses (S16: 32 bytes in, 16 out; F32P with C channels: C x 64 bytes in, C x 16 out, interleaved in registers -- the kernel is
// instantiated per channel count so that every register index is a constant).  The head is what brings the caller's pointers to a
// 16-byte boundary; head and tail go one sample per lane.  Pointers whose 16-byte phases cannot be met together (and planes that do
// not start on 16-byte boundaries, samples_per_channel % 4 != 0) make the whole track "head".  The grid is capped and strides.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "agmv_hip_impl.h"
#include "agmv_audio.h"

constexpr uint32_t AUD_T = 256;              // lanes of a workgroup
constexpr uint32_t AUD_MAX_BLOCKS = 2048;    // 256 CUs x 8 workgroups; the rest of a long track is reached by the stride
constexpr uint32_t AUD_MAX_PLANES = 8;
enum { PCM_S16 = 1, PCM_U8 = 2, PCM_F32P = 3 };   // AGMV_PCMFMT of include/agmv.h, by value

// how a track of n samples (per channel) is cut: [0, head) and [head + 16 * units, n) one sample per lane, the units in between
struct aud_cut { uint64_t n, head, units; };

// the i-th sample outside the body
__device__ __forceinline__ uint64_t edge_sample(const aud_cut& k, uint64_t i) { return i < k.head ? i : i + k.units * 16; }
__device__ __forceinline__ uint64_t edge_count(const aud_cut& k) { return k.n - k.units * 16; }

__device__ __forceinline__ uint32_t compand2(uint32_t w) { return agmv_audio_compand((uint16_t)w) | (uint32_t)agmv_audio_compand((uint16_t)(w >> 16)) << 8; }
__device__ __forceinline__ uint32_t compand4(uint32_t lo, uint32_t hi) { return compand2(lo) | compand2(hi) << 16; }
__device__ __forceinline__ uint32_t expand2(uint32_t b) { return agmv_audio_expand((uint8_t)b) | (uint32_t)agmv_audio_expand((uint8_t)(b >> 8)) << 16; }

__global__ __launch_bounds__(AUD_T) void k_aud_compand_s16(const uint16_t* __restrict__ pcm, uint8_t* __restrict__ codes, aud_cut k)
{
	const uint64_t tid = (uint64_t)blockIdx.x * AUD_T + threadIdx.x, stride = (uint64_t)gridDim.x * AUD_T;
	for (uint64_t u = tid; u < k.units; u += stride) {
		const uint4* src = (const uint4*)(pcm + k.head + u * 16);
		const uint4 a = src[0], b = src[1];
		*(uint4*)(codes + k.head + u * 16) = make_uint4(compand4(a.x, a.y), compand4(a.z, a.w), compand4(b.x, b.y), compand4(b.z, b.w));
	}
	for (uint64_t e = tid; e < edge_count(k); e += stride) {
		const uint64_t i = edge_sample(k, e);
		codes[i] = agmv_audio_compand(pcm[i]);
	}
}

__global__ __launch_bounds__(AUD_T) void k_aud_expand_s16(const uint8_t* __restrict__ codes, uint16_t* __restrict__ pcm, aud_cut k)
{
	const uint64_t tid = (uint64_t)blockIdx.x * AUD_T + threadIdx.x, stride = (uint64_t)gridDim.x * AUD_T;
	for (uint64_t u = tid; u < k.units; u += stride) {
		const uint4 c = *(const uint4*)(codes + k.head + u * 16);
		uint4* dst = (uint4*)(pcm + k.head + u * 16);
		dst[0] = make_uint4(expand2(c.x), expand2(c.x >> 16), expand2(c.y), expand2(c.y >> 16));
		dst[1] = make_uint4(expand2(c.z), expand2(c.z >> 16), expand2(c.w), expand2(c.w >> 16));
	}
	for (uint64_t e = tid; e < edge_count(k); e += stride) {
		const uint64_t i = edge_sample(k, e);
		pcm[i] = agmv_audio_expand(codes[i]);
	}
}

// planes [CH][n] of float -> codes [n][CH]
template <int CH>
__global__ __launch_bounds__(AUD_T) void k_aud_compand_f32p(const float* __restrict__ pcm, uint8_t* __restrict__ codes, aud_cut k)
{
	const uint64_t tid = (uint64_t)blockIdx.x * AUD_T + threadIdx.x, stride = (uint64_t)gridDim.x * AUD_T;
	for (uint64_t u = tid; u < k.units; u += stride) {
		const uint64_t s0 = k.head + u * 16;
		uint32_t o[4 * CH];
#pragma unroll
		for (int w = 0; w < 4 * CH; w++) o[w] = 0;
#pragma unroll
		for (int c = 0; c < CH; c++) {
			const float4* src = (const float4*)(pcm + (uint64_t)c * k.n + s0);
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const float4 v = src[q];
				const float x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const int at = (q * 4 + j) * CH + c;          // the byte of the unit's 16 * CH: a constant after unrolling
					o[at >> 2] |= (uint32_t)agmv_audio_compand(agmv_audio_from_f32(x[j])) << ((at & 3) * 8);
				}
			}
		}
		uint4* dst = (uint4*)(codes + s0 * CH);
#pragma unroll
		for (int w = 0; w < CH; w++) dst[w] = make_uint4(o[4 * w], o[4 * w + 1], o[4 * w + 2], o[4 * w + 3]);
	}
	for (uint64_t e = tid; e < edge_count(k) * CH; e += stride) {
		const uint64_t s = edge_sample(k, e / CH);
		const uint32_t c = (uint32_t)(e % CH);
		codes[s * CH + c] = agmv_audio_compand(agmv_audio_from_f32(pcm[(uint64_t)c * k.n + s]));
	}
}

// codes [n][CH] -> planes [CH][n] of float
template <int CH>
__global__ __launch_bounds__(AUD_T) void k_aud_expand_f32p(const uint8_t* __restrict__ codes, float* __restrict__ pcm, aud_cut k)
{
	const uint64_t tid = (uint64_t)blockIdx.x * AUD_T + threadIdx.x, stride = (uint64_t)gridDim.x * AUD_T;
	for (uint64_t u = tid; u < k.units; u += stride) {
		const uint64_t s0 = k.head + u * 16;
		const uint4* src = (const uint4*)(codes + s0 * CH);
		uint32_t in[4 * CH];
#pragma unroll
		for (int w = 0; w < CH; w++) {
			const uint4 v = src[w];
			in[4 * w] = v.x; in[4 * w + 1] = v.y; in[4 * w + 2] = v.z; in[4 * w + 3] = v.w;
		}
#pragma unroll
		for (int c = 0; c < CH; c++) {
			float4* dst = (float4*)(pcm + (uint64_t)c * k.n + s0);
#pragma unroll
			for (int q = 0; q < 4; q++) {
				float x[4];
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const int at = (q * 4 + j) * CH + c;
					x[j] = agmv_audio_to_f32(agmv_audio_expand((uint8_t)(in[at >> 2] >> ((at & 3) * 8))));
				}
				dst[q] = make_float4(x[0], x[1], x[2], x[3]);
			}
		}
	}
	for (uint64_t e = tid; e < edge_count(k) * CH; e += stride) {
		const uint64_t s = edge_sample(k, e / CH);
		const uint32_t c = (uint32_t)(e % CH);
		pcm[(uint64_t)c * k.n + s] = agmv_audio_to_f32(agmv_audio_expand(codes[s * CH + c]));
	}
}

// the cut of n samples whose sample s lies at pcm + s * pcm_step bytes (planes: plane c at pcm + c * plane_bytes) and at
// codes + s * code_step bytes: the smallest head that puts all of them on 16-byte boundaries, or the whole track
static aud_cut cut_of(uint64_t n, uintptr_t pcm, uint32_t pcm_step, uint64_t plane_bytes, uint32_t planes, uintptr_t codes, uint32_t code_step)
{
	aud_cut k = { n, n, 0 };
	for (uint64_t h = 0; h < 16 && h + 16 <= n; h++) {
		bool ok = (codes + h * code_step) % 16 == 0;
		for (uint32_t c = 0; ok && c < planes; c++) ok = (pcm + c * plane_bytes + h * pcm_step) % 16 == 0;
		if (ok) { k.head = h; k.units = (n - h) / 16; break; }
	}
	return k;
}

static dim3 grid_of(const aud_cut& k, uint32_t per_sample)
{
	const uint64_t edge = (k.n - k.units * 16) * per_sample, work = k.units > edge ? k.units : edge;
	const uint64_t blocks = (work + AUD_T - 1) / AUD_T;
	return dim3((uint32_t)(blocks > AUD_MAX_BLOCKS ? AUD_MAX_BLOCKS : (blocks ? blocks : 1)));
}

// what both directions refuse; *total = samples over all channels
static int check_args(const char* who, agmv_hip_ctx* c, int pcmfmt, const void* d_pcm, uint32_t channels, uint64_t n, const void* d_codes, uint64_t* total)
{
	if (!c) return agmv_hip_err("agmv_hip: NULL context");
	if (pcmfmt != PCM_S16 && pcmfmt != PCM_U8 && pcmfmt != PCM_F32P) return agmv_hip_err("%s: %d is no AGMV_PCMFMT (1 S16, 2 U8, 3 F32P)", who, pcmfmt);
	if (!d_pcm || !d_codes) return agmv_hip_err("%s: NULL pointer", who);
	if (channels == 0) return agmv_hip_err("%s: zero channels", who);
	if (pcmfmt == PCM_F32P && channels > AUD_MAX_PLANES) return agmv_hip_err("%s: %u planar channels, 1 .. %u are possible", who, channels, AUD_MAX_PLANES);
	if (n > (UINT64_MAX >> 4) / channels) return agmv_hip_err("%s: %llu samples in %u channels cannot be addressed", who, (unsigned long long)n, channels);
	if ((uintptr_t)d_pcm % (pcmfmt == PCM_S16 ? 2 : pcmfmt == PCM_F32P ? 4 : 1))
		return agmv_hip_err("%s: the PCM pointer is not aligned to its sample size", who);
	*total = n * channels;
	return 0;
}

#define AUD_PER_CHANNELS(KERNEL, ...) \
	switch (channels) { \
	case 1: hipLaunchKernelGGL(KERNEL<1>, grid_of(k, 1), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	case 2: hipLaunchKernelGGL(KERNEL<2>, grid_of(k, 2), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	case 3: hipLaunchKernelGGL(KERNEL<3>, grid_of(k, 3), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	case 4: hipLaunchKernelGGL(KERNEL<4>, grid_of(k, 4), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	case 5: hipLaunchKernelGGL(KERNEL<5>, grid_of(k, 5), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	case 6: hipLaunchKernelGGL(KERNEL<6>, grid_of(k, 6), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	case 7: hipLaunchKernelGGL(KERNEL<7>, grid_of(k, 7), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	default: hipLaunchKernelGGL(KERNEL<8>, grid_of(k, 8), dim3(AUD_T), 0, s, __VA_ARGS__); break; \
	}

extern "C" int agmv_hip_audio_compand_async(agmv_hip_ctx* c, int pcmfmt, const void* d_pcm, uint32_t channels, uint64_t samples_per_channel,
                                            uint8_t* d_codes, void* stream)
{
	uint64_t total = 0;
	if (check_args("agmv_hip_audio_compand_async", c, pcmfmt, d_pcm, channels, samples_per_channel, d_codes, &total)) return -1;
	if (total == 0) return 0;
	CK(hipSetDevice(c->device));
	const hipStream_t s = (hipStream_t)stream;
	if (pcmfmt == PCM_U8) {
		CK(hipMemcpyAsync(d_codes, d_pcm, total, hipMemcpyDeviceToDevice, s));
		return 0;
	}
	if (pcmfmt == PCM_S16) {
		const aud_cut k = cut_of(total, (uintptr_t)d_pcm, 2, 0, 1, (uintptr_t)d_codes, 1);
		hipLaunchKernelGGL(k_aud_compand_s16, grid_of(k, 1), dim3(AUD_T), 0, s, (const uint16_t*)d_pcm, d_codes, k);
	} else {
		const aud_cut k = cut_of(samples_per_channel, (uintptr_t)d_pcm, 4, samples_per_channel * 4, channels, (uintptr_t)d_codes, channels);
		AUD_PER_CHANNELS(k_aud_compand_f32p, (const float*)d_pcm, d_codes, k)
	}
	CK(hipGetLastError());
	return 0;
}

extern "C" int agmv_hip_audio_expand_async(agmv_hip_ctx* c, int pcmfmt, const uint8_t* d_codes, uint32_t channels, uint64_t samples_per_channel,
                                           void* d_pcm, void* stream)
{
	uint64_t total = 0;
	if (check_args("agmv_hip_audio_expand_async", c, pcmfmt, d_pcm, channels, samples_per_channel, d_codes, &total)) return -1;
	if (total == 0) return 0;
	CK(hipSetDevice(c->device));
	const hipStream_t s = (hipStream_t)stream;
	if (pcmfmt == PCM_U8) {
		CK(hipMemcpyAsync(d_pcm, d_codes, total, hipMemcpyDeviceToDevice, s));
		return 0;
	}
	if (pcmfmt == PCM_S16) {
		const aud_cut k = cut_of(total, (uintptr_t)d_pcm, 2, 0, 1, (uintptr_t)d_codes, 1);
		hipLaunchKernelGGL(k_aud_expand_s16, grid_of(k, 1), dim3(AUD_T), 0, s, d_codes, (uint16_t*)d_pcm, k);
	} else {
		const aud_cut k = cut_of(samples_per_channel, (uintptr_t)d_pcm, 4, samples_per_channel * 4, channels, (uintptr_t)d_codes, channels);
		AUD_PER_CHANNELS(k_aud_expand_f32p, d_codes, (float*)d_pcm, k)
	}
	CK(hipGetLastError());
	return 0;
}
