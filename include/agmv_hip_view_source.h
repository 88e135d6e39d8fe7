/*
 * include/agmv_hip_view_source.h -- the view of a clip in the caller's layout, an entry point of libagmv_hip.so beside those of
 * include/agmv_hip.h and include/agmv_hip_view.h (same context, same conventions: plain pointers and sizes, non-zero with a message
 * in agmv_hip_last_error() on refusal).
 */
#ifndef AGMV_HIP_VIEW_SOURCE_H
#define AGMV_HIP_VIEW_SOURCE_H

#include "agmv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- a view of a source clip: every step-th frame, a window of each, read in the source's layout ------
 * d_dst[j][r][c] = P(first + j * step)[y + r][x + c] for j < count, r < h, c < w, where P(k) is the packed XRGB32 frame that
 * agmv_hip_pixels_to_xrgb_dev / agmv_hip_yuv_to_xrgb_dev give for frame k of the source: d_src holds frames of src_w x src_h pixels in
 * the layout fmt (an AGMV_PIXFMT of include/agmv.h, NV12 / I420 with their AGMV_YUV_ flags), d_dst receives a packed XRGB32 clip of
 * `count` frames of w x h.  A YUV pixel takes the chroma sample of its 2 x 2 cell of the source frame, so a window may start and
 * end anywhere, odd offsets and odd sizes included.  AGMV_PIXFMT_XRGB32 is agmv_hip_view_frames_async as it stands: the words are
 * copied as they are, bits 24 .. 31 included; every other layout gives 0 there.  The caller guarantees that frame
 * first + (count - 1) * step lies inside the source clip and that the two clips do not overlap.  One launch, asynchronous on
 * `stream`: a streaming convert-copy, no allocation, no host synchronisation, nothing of the context is used but its device.  A
 * lane owns 16 consecutive pixels of an output row (NV12 / I420: of two rows, a patch of 16 x 2).  The 16-byte non-temporal loads of
 * the whole-clip converters are used where the window's rows sit on 16-byte boundaries of the source -- d_src 16-byte aligned, x
 * and src_w multiples of 16 (RGBA32: of 4), for NV12 / I420 also an even y -- and 16-byte stores where w is a multiple of 4 and d_dst
 * is 16-byte aligned; everything else goes element by element, to the same words.  A launch spreads at most 65535 frames over the
 * grid; a longer view takes further trips round the kernel's frame loop.  Nothing outside the count target frames is written.
 * Returns non-zero with a message and launches nothing for a NULL pointer, a zero size, step == 0, a window that does not lie
 * inside the source frame, an unknown format, or an NV12 / I420 source of odd width or height; otherwise count == 0 is success and
 * launches nothing. */
int agmv_hip_view_source_async(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t src_w, uint32_t src_h, uint32_t first,
                               uint32_t step, uint32_t count, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t* d_dst,
                               void* stream);

#ifdef __cplusplus
}
#endif

#endif
