/*
 * include/agmv_hip_view.h -- the view of a decoded clip, an entry point of libagmv_hip.so beside those of include/agmv_hip.h (same
 * context, same conventions: plain pointers and sizes, non-zero with a message in agmv_hip_last_error() on refusal).
 */
#ifndef AGMV_HIP_VIEW_H
#define AGMV_HIP_VIEW_H

#include "agmv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- a view of a decoded clip: every step-th frame, a window of each ---------------------------------
 * d_dst[j][r][c] = d_src[first + j * step][y + r][x + c] for j < count, r < h, c < w: d_src holds packed XRGB32 frames of
 * src_w x src_h, d_dst receives a packed XRGB32 clip of `count` frames of w x h.  Whole 32-bit words are copied as they are,
 * bits 24 .. 31 included.  The caller guarantees that frame first + (count - 1) * step lies inside the source clip and that the
 * two clips do not overlap.  One launch, asynchronous on `stream`: a streaming copy, no allocation, no host synchronisation,
 * nothing of the context is used but its device.  A lane owns 4 consecutive pixels of an output row: one 16-byte load where x and
 * src_w are multiples of 4 and d_src is 16-byte aligned, one 16-byte store where w is a multiple of 4 and d_dst is 16-byte aligned,
 * else word by word, to the same words.  A launch spreads at most 65535 frames over the grid; a longer view takes further trips
 * round the kernel's frame loop.  Nothing outside the count target frames is written.  Returns non-zero with a message and
 * launches nothing for a NULL pointer, a zero size, step == 0, or a window that does not lie inside the source frame; otherwise
 * count == 0 is success and launches nothing. */
int agmv_hip_view_frames_async(agmv_hip_ctx* ctx, const uint32_t* d_src, uint32_t src_w, uint32_t src_h, uint32_t first,
                               uint32_t step, uint32_t count, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t* d_dst,
                               void* stream);

#ifdef __cplusplus
}
#endif

#endif
