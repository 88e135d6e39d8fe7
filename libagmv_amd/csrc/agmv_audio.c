/*
 * libagmv_amd/csrc/agmv_audio.c -- audio tracks on the host: companding, the AGAC chunks, the WAV / raw importers and the
 * WAV / AIFF / AIFC exporters of the reference API (reference src/agmv_encode.c:636-717, src/agmv_decode.c:412-453, :649-767,
 * src/agmv_utils.c:584-616, :916-918, :1035-1113, :1318-1344, :1403-1575).  include/agmv.h ("audio tracks") holds the format
 * and the places where this build reads zeros and stays in bounds where the reference reads memory it never set; the arithmetic
 * is agmv_audio.h's, shared with the kernels.  Plain host C.
 */
#include <stdlib.h>
#include <string.h>

#include "agmv.h"
#include "agmv_audio.h"
#include "agmv_pipeline.h"

void AGMV_SyncAudioTrack(AGMV* a, const void* pcm)
{
	const size_t n = (size_t)AGMV_GetAudioSize(a);
	if (AGMV_GetBitsPerSample(a) == 16) memcpy(a->audio_track->pcm, pcm, n * sizeof(u16));
	else memcpy(a->audio_track->pcm8, pcm, n);
}

void AGMV_SignedToUnsignedPCM(u8* pcm, u32 size) { u32 i; for (i = 0; i < size; i++) pcm[i] = (u8)(pcm[i] + 128); }
void AGMV_UnsigendToSignedPCM(u8* pcm, u32 size) { u32 i; for (i = 0; i < size; i++) pcm[i] = (u8)(pcm[i] - 128); }

u32 AGMV_CalculateTotalAudioDuration(u32 size, u32 sample_rate, u16 num_of_channels, u16 bits_per_sample)
{
	return (u32)(size / (f32)sample_rate * num_of_channels * (bits_per_sample / 8));
}

/* whole seconds of `bytes` of PCM; 0 (no track) where the reference divides by zero */
static u32 whole_seconds(u32 bytes, u32 sample_rate, u32 channels, u32 bits_per_sample)
{
	const u32 per_second = sample_rate * channels * (bits_per_sample / 8);
	return per_second ? bytes / per_second : 0;
}

void AGMV_CompressAudio(AGMV* a)
{
	const size_t n = (size_t)AGMV_GetAudioSize(a);
	u8* out = a->audio_chunk->atsample;
	size_t i;
	if (AGMV_GetBitsPerSample(a) == 16) {
		const u16* pcm = a->audio_track->pcm;
		for (i = 0; i < n; i++) out[i] = agmv_audio_compand(pcm[i]);
	} else
		memcpy(out, a->audio_track->pcm8, n);
}

/* `size` codes from start_point; zeros for samples past audio_size, and for an object without codes (then start_point stays) */
void AGMV_EncodeAudioChunk(FILE* f, AGMV* a)
{
	static const u8 zeros[256];
	const u32 size = a->audio_chunk ? a->audio_chunk->size : 0, total = a->header.audio_size;
	u32 held = 0, i;
	AGMV_WriteFourCC(f, 'A', 'G', 'A', 'C');
	AGMV_WriteLong(f, size);
	if (size && a->audio_chunk->atsample) {
		const u32 start = a->audio_track->start_point;
		held = start < total ? (size < total - start ? size : total - start) : 0;
		fwrite(a->audio_chunk->atsample + start, 1, held, f);
		a->audio_track->start_point = start + size;
	}
	for (i = held; i < size; i += sizeof(zeros)) fwrite(zeros, 1, size - i < sizeof(zeros) ? size - i : sizeof(zeros), f);
}

/* expands into audio_track->pcm / pcm8 when the object has that buffer (audio_size samples), else seeks over the payload */
int AGMV_DecodeAudioChunk(FILE* f, AGMV* a)
{
	const int wide = AGMV_GetBitsPerSample(a) == 16;
	u32 size, start, total, done = 0;
	u8 buf[4096];
	AGMV_ReadFourCC(f, a->audio_chunk->fourcc);
	a->audio_chunk->size = size = AGMV_ReadLong(f);
	if (!AGMV_IsCorrectFourCC(a->audio_chunk->fourcc, 'A', 'G', 'A', 'C')) return INVALID_HEADER_FORMATTING_ERR;
	if (!a->audio_track || !(wide ? (void*)a->audio_track->pcm : (void*)a->audio_track->pcm8)) {
		fseek(f, (long)size, SEEK_CUR);
		return NO_ERR;
	}
	start = a->audio_track->start_point; total = a->header.audio_size;
	while (done < size) {
		const u32 want = size - done < sizeof(buf) ? size - done : (u32)sizeof(buf);
		const size_t got = fread(buf, 1, want, f);
		u32 i;
		memset(buf + got, 0, want - got);                          /* a file that ends inside the payload: zeros */
		for (i = 0; i < want; i++) {
			const u32 at = start + done + i;
			if (at >= total) break;
			if (wide) a->audio_track->pcm[at] = agmv_audio_expand(buf[i]);
			else a->audio_track->pcm8[at] = buf[i];
		}
		done += want;
		if (got < want) break;
	}
	a->audio_track->start_point = start + size;
	return NO_ERR;
}

/* the object's track replaced by a zeroed one of n samples; 0 when there is nothing to hold or it cannot be allocated (then the
   object holds no track) */
static int new_track(AGMV* a, u32 n, int bits)
{
	void* p = n ? calloc(n, bits == 16 ? sizeof(u16) : 1) : NULL;
	free(a->audio_track->pcm); free(a->audio_track->pcm8);
	a->audio_track->pcm = NULL; a->audio_track->pcm8 = NULL;
	AGMV_SetBitsPerSample(a, (u16)bits);
	AGMV_SetAudioSize(a, p ? n : 0);
	if (!p) { AGMV_SetTotalAudioDuration(a, 0); return 0; }
	if (bits == 16) a->audio_track->pcm = (u16*)p; else a->audio_track->pcm8 = (u8*)p;
	return 1;
}

/* canonical 44-byte header only, like the reference; the RIFF size stands in for the data size (include/agmv.h) */
void AGMV_WavToAudioTrack(const char* filename, AGMV* a)
{
	FILE* wav = fopen(filename, "rb");
	u32 riff_size, channels, rate, bits, n;
	if (!wav) return;
	AGMV_ReadLong(wav);                                            /* "RIFF" */
	riff_size = AGMV_ReadLong(wav);
	AGMV_ReadLong(wav); AGMV_ReadLong(wav); AGMV_ReadLong(wav);    /* "WAVE", "fmt ", 16 */
	AGMV_ReadShort(wav);                                           /* format tag */
	channels = AGMV_ReadShort(wav);
	rate = AGMV_ReadLong(wav);
	AGMV_ReadLong(wav); AGMV_ReadShort(wav);                       /* byte rate, block align */
	bits = AGMV_ReadShort(wav) == 16 ? 16 : 8;
	AGMV_ReadLong(wav); AGMV_ReadLong(wav);                        /* "data", its size */
	n = bits == 16 ? riff_size / 2 : riff_size;
	AGMV_SetSampleRate(a, rate);
	AGMV_SetNumberOfChannels(a, (u8)channels);
	AGMV_SetTotalAudioDuration(a, whole_seconds(riff_size, rate, channels, bits));
	if (new_track(a, n, bits)) {
		const size_t got = bits == 16 ? fread(a->audio_track->pcm, 2, n, wav) : fread(a->audio_track->pcm8, 1, n, wav);
		(void)got;                                                 /* what the file does not hold stays 0 */
	}
	fclose(wav);
}

/* a file of signed bytes -> an 8-bit (unsigned) track */
void AGMV_RawSignedPCMToAudioTrack(const char* filename, AGMV* a, u8 num_of_channels, u32 sample_rate)
{
	FILE* f = fopen(filename, "rb");
	long len;
	if (!f) return;
	fseek(f, 0, SEEK_END); len = ftell(f); fseek(f, 0, SEEK_SET);
	if (len < 0) len = 0;
	AGMV_SetSampleRate(a, sample_rate);
	AGMV_SetNumberOfChannels(a, num_of_channels);
	AGMV_SetTotalAudioDuration(a, whole_seconds((u32)len, sample_rate, num_of_channels, 8));
	if (new_track(a, (u32)len, 8)) {
		const size_t got = fread(a->audio_track->pcm8, 1, (size_t)len, f);
		AGMV_SignedToUnsignedPCM(a->audio_track->pcm8, (u32)got);
	}
	fclose(f);
}

/* a file of signed bytes at 16 kHz mono -> audio_chunk->satsample, as they are (the GBA player's form) */
void AGMV_Raw8PCMToAudioTrack(const char* filename, AGMV* a)
{
	FILE* f = fopen(filename, "rb");
	long len;
	s8* data;
	if (!f) return;
	fseek(f, 0, SEEK_END); len = ftell(f); fseek(f, 0, SEEK_SET);
	if (len < 0) len = 0;
	data = (s8*)calloc(len ? (size_t)len : 1, 1);
	if (data) {
		const size_t got = fread(data, 1, (size_t)len, f);
		(void)got;
		AGMV_SetTotalAudioDuration(a, (u32)len / 16000);
		AGMV_SetSampleRate(a, 16000);
		AGMV_SetNumberOfChannels(a, 1);
		AGMV_SetAudioSize(a, (u32)len);
		a->audio_chunk->satsample = data;
	}
	fclose(f);
}

/* ------------------------------------------------------------------------------------------
 * export
 * ------------------------------------------------------------------------------------------ */
static void be16(FILE* f, u32 v) { AGMV_WriteByte(f, (u8)(v >> 8)); AGMV_WriteByte(f, (u8)v); }
static void be32(FILE* f, u32 v) { be16(f, v >> 16); be16(f, v & 0xFFFFu); }

/* the sample rate as the exporters write it: the first four bytes of the 80-bit float (sign and exponent, then the leading 16
   bits of the mantissa) and six zero bytes (reference src/agmv_decode.c:649-680, src/agmv_utils.c:1457-1466) */
static void rate80(FILE* f, u32 rate)
{
	u8 b[10];
	memset(b, 0, sizeof(b));
	if (rate <= 1) { b[0] = 0x3F; b[1] = 0xFF; b[2] = 0x80; }
	else if (rate >= 0x40000000ul) { b[0] = 0x40; b[1] = 0x1D; }
	else {
		int lead = 30;                                             /* the highest set bit of rate, below bit 30 */
		u32 m;
		while (!(rate >> lead & 1)) lead--;
		m = (rate << (31 - lead)) & 0xFFFFFFFFul;                  /* that bit moved to bit 31 */
		b[0] = 0x40; b[1] = (u8)(lead - 1); b[2] = (u8)(m >> 24); b[3] = (u8)(m >> 16);
	}
	fwrite(b, 1, 10, f);
}

static void samples_be(FILE* f, AGMV* a)
{
	const u32 n = AGMV_GetAudioSize(a);
	u32 i;
	if (AGMV_GetBitsPerSample(a) == 16) for (i = 0; i < n; i++) be16(f, a->audio_track->pcm[i]);
	else for (i = 0; i < n; i++) AGMV_WriteByte(f, (u8)(a->audio_track->pcm8[i] - 128));
}

void AGMV_ExportAudioType(FILE* f, AGMV* a, AGMV_AUDIO_TYPE type)
{
	const u32 n = AGMV_GetAudioSize(a), channels = AGMV_GetNumberOfChannels(a), bits = AGMV_GetBitsPerSample(a);
	const u32 bytes = bits == 16 ? n * 2 : n;
	if (type == AGMV_AUDIO_AIFF || type == AGMV_AUDIO_AIFC) {
		const int compressed_form = type == AGMV_AUDIO_AIFF;       /* the reference's names are swapped; kept */
		AGMV_WriteFourCC(f, 'F', 'O', 'R', 'M');
		be32(f, bytes + 32);
		if (compressed_form) {
			AGMV_WriteFourCC(f, 'A', 'I', 'F', 'C');
			AGMV_WriteFourCC(f, 'F', 'V', 'E', 'R');
			be32(f, 4);
			AGMV_WriteFourCC(f, (char)0xA2, (char)0x80, 0x51, 0x40);
		} else
			AGMV_WriteFourCC(f, 'A', 'I', 'F', 'F');
		AGMV_WriteFourCC(f, 'C', 'O', 'M', 'M');
		be32(f, compressed_form ? 26 : 18);
		be16(f, channels);
		be32(f, channels ? n / channels : 0);
		be16(f, bits);
		rate80(f, AGMV_GetSampleRate(a));
		if (compressed_form) { AGMV_WriteFourCC(f, 'N', 'O', 'N', 'E'); AGMV_WriteFourCC(f, 'N', 'O', 'N', 'E'); }
		AGMV_WriteFourCC(f, 'S', 'S', 'N', 'D');
		be32(f, bytes);
		AGMV_WriteLong(f, 0); AGMV_WriteLong(f, 0);
		samples_be(f, a);
		return;
	}
	/* WAV, also for any other type: both size fields are the data size, the byte rate is the constant 75600 */
	AGMV_WriteFourCC(f, 'R', 'I', 'F', 'F');
	AGMV_WriteLong(f, bytes);
	AGMV_WriteFourCC(f, 'W', 'A', 'V', 'E');
	AGMV_WriteFourCC(f, 'f', 'm', 't', ' ');
	AGMV_WriteLong(f, 16);
	AGMV_WriteShort(f, 1);
	AGMV_WriteShort(f, (u16)channels);
	AGMV_WriteLong(f, AGMV_GetSampleRate(a));
	AGMV_WriteLong(f, 75600);
	AGMV_WriteShort(f, (u16)(channels * bits / 8));
	AGMV_WriteShort(f, (u16)bits);
	AGMV_WriteFourCC(f, 'd', 'a', 't', 'a');
	AGMV_WriteLong(f, bytes);
	if (bits == 16) fwrite(a->audio_track->pcm, 2, n, f);
	else fwrite(a->audio_track->pcm8, 1, n, f);
}

/* the file's track to quick_export.wav / quick_export.aiff in the working directory; the video is skipped, not decoded.  The
   chunks are walked in the file's image by the decoder's locator (agmv_gather_audio: the walk of the reference's AGMV_DecodeAudio,
   src/agmv_decode.c:725-729), so a file that ends anywhere -- inside a payload, a size field or a fourcc -- gives what it holds */
int AGMV_DecodeAudio(const char* filename, AGMV_AUDIO_TYPE type)
{
	FILE* file = fopen(filename, "rb"), *out;
	AGMV* a;
	int err;
	if (!file) return FILE_NOT_FOUND_ERR;
	a = CreateAGMV(0, 0, 0, 0);
	err = AGMV_DecodeHeader(file, a);
	if (err == NO_ERR && AGMV_GetTotalAudioDuration(a) != 0) {
		const u32 duration = AGMV_GetTotalAudioDuration(a), total = AGMV_GetAudioSize(a);
		const size_t pos = (size_t)ftell(file);
		u8 *image = NULL, *codes = NULL;
		long len;
		fseek(file, 0, SEEK_END); len = ftell(file); fseek(file, 0, SEEK_SET);
		if (len < 0) len = 0;
		if (new_track(a, total, AGMV_GetBitsPerSample(a))) {
			image = (u8*)malloc((size_t)len + 1); codes = (u8*)malloc(total);
		}
		AGMV_SetTotalAudioDuration(a, duration);
		if (!image || !codes) err = MEMORY_CORRUPTION_ERR;
		else {
			const size_t got = fread(image, 1, (size_t)len, file);
			const size_t n = agmv_gather_audio(image, got, pos, (uint32_t)AGMV_GetNumberOfFrames(a), codes, total);
			const int aiff = type == AGMV_AUDIO_AIFF || type == AGMV_AUDIO_AIFC;
			size_t i;
			if (AGMV_GetBitsPerSample(a) == 16) for (i = 0; i < n; i++) a->audio_track->pcm[i] = agmv_audio_expand(codes[i]);
			else memcpy(a->audio_track->pcm8, codes, n);
			a->audio_track->start_point = (u32)n;
			out = fopen(aiff ? "quick_export.aiff" : "quick_export.wav", "wb");
			if (out) { AGMV_ExportAudioType(out, a, type); fclose(out); }
		}
		free(image); free(codes);
	}
	fclose(file);
	DestroyAGMV(a);
	return err;
}
