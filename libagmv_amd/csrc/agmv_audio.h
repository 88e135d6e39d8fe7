/* libagmv_amd/csrc/agmv_audio.h -- the audio codec of the container, stated once: the host library (agmv_audio.c) and the kernels
 * (agmv_audio_hip.hip) both call these.  Internal, not installed.  include/agmv.h ("audio tracks") holds the definitions.
 *
 *   agmv_audio_compand   one sample of a 16-bit track (its u16 is the WAV sample's bit pattern) -> its code byte: the loop body of
 *                        AGMV_CompressAudio (reference src/agmv_encode.c:659-699) in integers, with its three quirks: the second
 *                        minimum overwrites the first (the rounded root only wins when it is the floor root), roundUpEven wraps
 *                        from 255 to 0, and a root of 256 converts to 0.
 *   agmv_audio_expand    a code -> the sample: an even code is a root, an odd one the high byte (src/agmv_decode.c:429-443; the two
 *                        tables it reads are these closed forms).
 *   agmv_audio_from_f32  a float sample -> the track's u16 (AGMV_PCM_F32P);  agmv_audio_to_f32 the way back.
 * No table, and no float in the companding. */
#ifndef AGMV_AUDIO_H
#define AGMV_AUDIO_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define AGMV_AUDIO_FN __host__ __device__ static inline
#else
#define AGMV_AUDIO_FN static inline
#endif

/* floor(sqrt(s)) for s < 65536 */
AGMV_AUDIO_FN uint32_t agmv_audio_isqrt(uint32_t s)
{
#ifdef __HIP_DEVICE_COMPILE__
	uint32_t k = (uint32_t)sqrtf((float)s);                   /* within 1 of the root whatever the rounding of sqrtf */
	k -= k * k > s;
	k += (k + 1) * (k + 1) <= s;
	return k;
#else
	uint32_t k = 0, bit;
	for (bit = 128; bit; bit >>= 1)
		if ((k | bit) * (k | bit) <= s) k |= bit;
	return k;
#endif
}

AGMV_AUDIO_FN uint8_t agmv_audio_compand(uint16_t sample)
{
	const int32_t s = sample;
	const uint32_t k = agmv_audio_isqrt(sample);
	const uint32_t e1 = k & 1u ? (k + 1u) & 255u : k;
	const uint32_t r = ((uint32_t)s > k * k + k ? k + 1u : k) & 255u;
	const uint32_t e2 = r & 1u ? (r + 1u) & 255u : r;
	const uint32_t e3 = (uint32_t)(s >> 8) | 1u;
	int32_t d1 = (int32_t)(e1 * e1) - s, d2 = (int32_t)(e2 * e2) - s, d3 = (int32_t)(e3 << 8) - s, d;
	d1 = d1 < 0 ? -d1 : d1; d2 = d2 < 0 ? -d2 : d2; d3 = d3 < 0 ? -d3 : d3;
	d = d1 < d3 ? d1 : d3;
	return (uint8_t)(d == d1 ? e1 : d == d2 ? e2 : e3);
}

AGMV_AUDIO_FN uint16_t agmv_audio_expand(uint8_t code)
{
	return (uint16_t)(code & 1u ? (uint32_t)code << 8 : (uint32_t)code * code);
}

/* clamp to [-1, 1], scale by 32767, round half to even; NaN is 0; the bit pattern of the int16 */
AGMV_AUDIO_FN uint16_t agmv_audio_from_f32(float x)
{
	if (x != x) return 0;
	return (uint16_t)(int16_t)(int)rintf(fminf(fmaxf(x, -1.0f), 1.0f) * 32767.0f);
}

AGMV_AUDIO_FN float agmv_audio_to_f32(uint16_t u) { return (float)(int16_t)u / 32768.0f; }

#endif
