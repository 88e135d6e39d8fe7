/*
 * include/agmv_writer.h -- writer sessions: a clip encoded in pieces into the file the one-shot call writes.  Entry points of
 * libagmv.so beside those of include/agmv.h, whose types and conventions they use; the mirror image of include/agmv_reader.h.
 *
 * Every device encoder of include/agmv.h takes the whole clip in device memory in one call: the palette comes from a histogram
 * over every frame and the header that carries it is written before the first chunk.  A clip that does not fit beside its
 * producer, a producer that reuses one buffer, a tool with a bounded footprint cannot call them.  A writer takes the clip twice
 * in pieces: pass 1 (AGMV_WriterAnalyseDev) counts frames towards the palette, pass 2 (AGMV_WriterWriteDev) encodes them.
 *
 * The contract.
 *
 * 1. The same file as the one-shot call.  Analyse the frames F[0..N) in any number of calls of any sizes, then write the same
 *    F[0..N) in any number of calls of any sizes, then close: the file is, byte for byte, what AGMV_EncodeFramesFmtDev
 *    (desc.tensor == 0, no target), AGMV_EncodeFramesScaledDev (a target width x height) or AGMV_EncodeFramesTensorDev
 *    (desc.tensor == 1) writes for the contiguous clip F with the same fmt | yuv_flags or type, mean and std, sizes, filter, fps,
 *    opt, quality, compression and schedule, under the same AGMV_BATCH_FRAMES, with AGMV_SetPaletteRefine, AGMV_SetDither,
 *    AGMV_SetStabilise (and their environment forms) as they stand at the open, and with AGMV_LZ_DEVICE, AGMV_LZ77_DEVICE and
 *    AGMV_LZ_THREADS as the one-shot call reads them.  Writes cut GOPs and batches wherever the caller likes: the session's
 *    batches are the one-shot call's batches, `cap` frames in whole GOPs, so the stabilisation (whose reach is the batch), the
 *    dither and LZ77's persistent buffer see what they see there.
 *
 * 2. The palette is that of what was analysed: AGMV_BuildPalette / AGMV_BuildPaletteRefined over the histogram of the analysed
 *    frames, which is the histogram the one-shot call takes of the same frames -- of the frames as handed in (before the scale
 *    of a GBA / NDS opt), of the scaled frames for a target size, of the XRGB32 frames a tensor stands for.  The first write
 *    freezes the palette, creates the file and writes the header; an analyse after it is refused (-6), and so is a write before
 *    any analyse (-6).  Analysing a sample only -- the first chunk of a live source -- is legal: the file is then a valid .agmv
 *    whose header palette is, byte for byte, the one-shot call's for the sample.  The byte identity of item 1 is claimed only
 *    when the analysed and the written frames are the same.
 *
 * 3. Nothing of the caller's is held after a call returns.  d_frames may be overwritten or freed the moment an analyse or a
 *    write returns, and may be another buffer on every call (complete when the call is made, as for the one-shot calls).  Frames
 *    that do not yet fill a batch, or that the schedule still has to look at, live in the writer's own staging ring, as XRGB32
 *    at the encode size: a write converts (and scales) into the ring with one launch per contiguous stretch of it.
 *
 * 4. Bounded memory.  Everything the writer holds is made at the open and sized by the batch and the ring, not by the clip:
 *    the ring, the sequence engine with its workers and slots, the histogram, the stream.  A write larger than the free part of
 *    the ring proceeds in pieces and waits for batches to leave (`waits` counts the waits); it returns once its frames are in
 *    the ring, not once they are encoded.  AGMV_CloseWriter drains.  ring_frames: 0 is the library's choice (four batches'
 *    sources and the hold-back); the minimum is the sources of one batch -- cap frames for AGMV_SCHEDULE_FULL, 2 * cap for
 *    AGMV_SCHEDULE_PDIFS, where a frame has up to two -- plus the 6 frames PDIFS holds back; a smaller request is raised to it.
 *
 * 5. Schedules.  AGMV_SCHEDULE_FULL and AGMV_SCHEDULE_PDIFS.  AGMV_SCHEDULE_ADAPTIVE is refused at the open with the code of
 *    an unknown enum (-1): its decisions compare pairs of frames over the whole clip before the first is encoded, pairs a writer
 *    has not seen together; it is left for later.  PDIFS does not know the clip's end where the one-shot call does: its first
 *    group is always emitted, a later group starting at 0-based frame j exactly when frame j + 5 exists.  So the writer emits a
 *    group once frame j + 5 has arrived and at the close drops the trailing frames the one-shot call never encodes either.  The
 *    bytes of the file that depend on the clip's length are patched at the close to the one-shot call's values: the frame count
 *    at offset 4 (the frames handed in for FULL, the chunks written for PDIFS) and, for PDIFS, the frames per second at offset
 *    18.  No other byte depends on the length.
 *
 * 6. Refusals.  AGMV_OpenWriterDev applies every argument check of the corresponding one-shot call with the same codes in the
 *    same order (include/agmv.h lists them; a NULL desc is -1; the checks of the frame count wait for the close), all before a
 *    device is opened or a file is created: a refused open returns NULL and sets *error (may be NULL) to the negative code, else
 *    to 0.  A tensor writer takes no target size (-3).  AGMV_WriterAnalyseDev / AGMV_WriterWriteDev: 0; -1 for a NULL writer,
 *    or a NULL d_frames with n > 0; n == 0 runs nothing and returns 0; -6 for a call out of order (item 2); -2 past 2^31 - 1
 *    frames.  AGMV_CloseWriter: 0 with *frames_written (may be NULL) = the chunks in the file; a close with fewer written frames
 *    than the schedule's first group reads (1 for FULL, 4 for a light PDIFS opt, 2 for a heavy one) is -2, the one-shot call's
 *    code, and leaves no file behind; 0 for a NULL writer.  A GPU failure inside the encoder aborts with a message, as in the
 *    one-shot calls.
 *
 * 7. No audio track: a writer writes none, and a pending AGMV_SetAudioDev track is neither consumed nor cleared (a PDIFS file
 *    carries an AGAC chunk header behind every frame chunk; it is written empty, as the one-shot call writes it without a track).
 *    Crop windows and frame strides (AGMV_EncodeViewDev) are out of scope.  So is another frame rate (AGMV_EncodeViewRateDev): the
 *    taps of one output frame may straddle two write pieces, and a writer keeps no frames between its calls.
 *
 * AGMV_WRITER_STATS, all since the open: frames analysed, frames taken by writes, frames whose chunks are in the file so far,
 * write calls that ran (n > 0), batches handed to the workers, waits for ring space, and the ring's length.  Writers are
 * independent of the one-shot calls between their calls except for AGMV_GetStabiliseStats, which reports the sequence closed
 * last; like every call of this library they are made by one thread at a time.
 */
#ifndef AGMV_WRITER_H
#define AGMV_WRITER_H

#include "agmv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AGMV_WRITER AGMV_WRITER;
typedef struct AGMV_WRITER_DESC {
	int tensor;                                  /* 0: a byte clip in `fmt`; 1: a normalised tensor of `type` */
	AGMV_PIXFMT fmt; int yuv_flags;              /* as AGMV_EncodeFramesFmtDev */
	AGMV_TENSORFMT type; float mean[3], std[3];  /* as AGMV_EncodeFramesTensorDev */
	unsigned src_width, src_height;              /* of the frames handed in */
	unsigned width, height; AGMV_SCALE filter;   /* target size as AGMV_EncodeFramesScaledDev; 0,0 = none, filter is not read */
	unsigned frames_per_second;
	AGMV_OPT opt; AGMV_QUALITY quality; AGMV_COMPRESSION compression; AGMV_SCHEDULE schedule;
	unsigned ring_frames;                        /* staging capacity in frames, 0 = the library's choice */
} AGMV_WRITER_DESC;
typedef struct AGMV_WRITER_STATS { unsigned long long analysed, taken, written; unsigned writes, batches, waits, ring_frames; } AGMV_WRITER_STATS;

AGMV_WRITER* AGMV_OpenWriterDev(const char* filename, const AGMV_WRITER_DESC* desc, int* error);
int  AGMV_WriterAnalyseDev(AGMV_WRITER* writer, const void* d_frames, u32 n);   /* pass 1: these frames count towards the palette */
int  AGMV_WriterWriteDev(AGMV_WRITER* writer, const void* d_frames, u32 n);     /* pass 2: these frames are the next n of the clip */
int  AGMV_CloseWriter(AGMV_WRITER* writer, u32* frames_written);                /* finishes the file; NULL is fine */
void AGMV_GetWriterStats(const AGMV_WRITER* writer, AGMV_WRITER_STATS* stats);

#ifdef __cplusplus
}
#endif

#endif
