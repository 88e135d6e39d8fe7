/*
 * include/agmv_reader.h -- reader sessions: a file opened once, read and sought with the decoder's state kept.  Entry points of
 * libagmv.so beside those of include/agmv.h, whose types and conventions they use.
 *
 * Every decode entry point of include/agmv.h is a call on a file name: it reads the file, opens its buffers, stream, pool and
 * worker, runs the LZ stage from frame 0 and frees everything on return.  A loader that walks a file in chunks, a player, a tool
 * that walks a file longer than the memory it wants to spend pay that per call.  A reader pays it once: what survives a read is
 * the state of the reference's decoder -- the ONE persistent decompression buffer, the last frame, the I-frame snapshot, the
 * place in the file -- together with the buffers around it.
 *
 * The contract, for every file, damaged ones included: a read of n frames at position p writes into d_dst exactly what
 * AGMV_DecodeViewDev (desc.tensor == 0) / AGMV_DecodeViewTensorDev (desc.tensor == 1) write for the view
 *     {first = p, count = n, step, x, y, width = win_width, height = win_height}
 * with the same fmt | yuv_flags (the AGMV_YUV_ flags of include/agmv.h) or type, mean and std, the same target width x height
 * and filter (0 x 0: no scaling, filter is not read) and the same deblocking, and then leaves the position at
 * p + delivered * step.  A read delivers fewer than n frames only at the file's end, 0 at or behind it; it returns with the
 * frames complete on the device, as the one-shot calls do, and holds nothing of the caller's afterwards: the reader keeps its
 * own unfiltered last frame and I-frame snapshot, so d_dst may be another buffer on every read and may be freed in between.
 *
 * AGMV_OpenReaderDev applies every argument check of AGMV_DecodeViewDev / AGMV_DecodeViewTensorDev with the same codes in the
 * same order (include/agmv.h lists them; a NULL desc is -1; step 0 reads as 1), all before a device is opened: a refused open
 * returns NULL and sets *error (may be NULL) to the negative code, else to 0.  *info (may be NULL) receives the header's
 * AGMV_INFO whenever the header could be read.  deblock: 0 = AGMV_SetDeblock / AGMV_DEBLOCK as a decode call reads them at
 * its open, else the strength, values above 64 count as 64.  The environment (AGMV_BATCH_FRAMES, AGMV_LZ_THREADS,
 * AGMV_LZ_DECODE_DEVICE, AGMV_DEVICE) is read at open, as a decode reads it.  Everything the reader holds -- the file image,
 * device and pinned buffers, stream, pool, worker, the seek index -- is made at open; a read makes nothing.
 * AGMV_ReaderReadDev: the frames delivered; 0 for n == 0, which runs nothing; -1 for a NULL reader or a NULL d_dst with n > 0;
 * another negative Error when the GPU failed, after which every read fails.  Readers are independent of each other and of the
 * one-shot calls between their reads (AGMV_GetViewStats and AGMV_GetDeblockStats go on reporting the one-shot calls alone), but
 * like every call of this library they are made by one thread at a time.
 *
 * Sequential reads cost what the frames cost: a file read front to back, in reads of any sizes, sends every frame through the
 * LZ stage once and through the GPU stage once (lz_frames == gpu_frames == the frames of the file for step 1).  Reads cut GOPs
 * and batches wherever the caller likes.
 *
 * Seeking.  Resuming the LZ stage at frame c needs the persistent buffer as it stood before frame c (lz_cap = w * h * 33 / 16 +
 * 4096 bytes: bytes [bpos, bpos + 16) of a later row may come from any earlier frame) and the place of chunk c.  The reader
 * records such checkpoints whenever its LZ stage passes a multiple of `interval` frames in order; checkpoint 0, the zero buffer,
 * always exists.  interval is the smallest multiple of 4, at least 4, with ceil(frames / interval) * lz_cap <= index_bytes; a
 * budget below one lz_cap leaves checkpoint 0 alone.  Checkpoints live where the persistent buffer lives: in host memory, or
 * with AGMV_LZ_DECODE_DEVICE=1 in device memory.  AGMV_ReaderSeek(f) to the current position does nothing; to any other it
 * takes the greatest recorded checkpoint c <= g0 = f & ~3, runs the LZ stage from c in order (recording the checkpoints it
 * passes) and starts the GPU stage at g0 from the state of a fresh decoder; if agmv_hip_decode_prior_dependent says that the
 * first batch so decoded derives from the state before it, the reader runs again from frame 0 and counts one restart -- the
 * rule of a view.  The work is done by the next read.  A seek at or behind the file's end makes reads deliver 0.  Returns 0,
 * -1 for a NULL reader.
 *
 * AGMV_READER_STATS, all since the open: lz_frames and gpu_frames through the two stages (a run given up for a restart
 * included), delivered frames, reads that ran (n > 0), seeks, restarts, checkpoints recorded (checkpoint 0 not counted) and
 * the interval.
 */
#ifndef AGMV_READER_H
#define AGMV_READER_H

#include "agmv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AGMV_READER AGMV_READER;
typedef struct AGMV_READER_DESC {
	int tensor;                                  /* 0: a byte clip in `fmt`; 1: a normalised tensor of `type` */
	AGMV_PIXFMT fmt; int yuv_flags;              /* as AGMV_DecodeFramesFmtDev */
	AGMV_TENSORFMT type; float mean[3], std[3];  /* as AGMV_DecodeFramesTensorDev */
	unsigned width, height; AGMV_SCALE filter;   /* target size; 0,0 = none */
	unsigned step, x, y, win_width, win_height;  /* stride in frames and window, AGMV_VIEW's rules; step 0 reads as 1 */
	unsigned deblock;                            /* 0 = AGMV_SetDeblock / AGMV_DEBLOCK as a decode call reads them, else 1..64 */
	size_t index_bytes;                          /* budget of the seek index, 0 = 64 MiB */
} AGMV_READER_DESC;
typedef struct AGMV_READER_STATS { unsigned long long lz_frames, gpu_frames, delivered; unsigned reads, seeks, restarts, checkpoints, interval; } AGMV_READER_STATS;

AGMV_READER* AGMV_OpenReaderDev(const char* filename, const AGMV_READER_DESC* desc, AGMV_INFO* info, int* error);
int  AGMV_ReaderReadDev(AGMV_READER* reader, void* d_dst, u32 n);      /* frames delivered, 0 at the end, negative on error */
int  AGMV_ReaderSeek(AGMV_READER* reader, u32 frame);                  /* file frame index; at or behind the end: reads then deliver 0 */
u32  AGMV_ReaderTell(const AGMV_READER* reader);                       /* file frame the next read starts at */
void AGMV_GetReaderStats(const AGMV_READER* reader, AGMV_READER_STATS* stats);
void AGMV_CloseReader(AGMV_READER* reader);                            /* NULL is fine */

#ifdef __cplusplus
}
#endif

#endif
