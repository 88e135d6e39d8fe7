/*
 * include/agmv_hip_time.h -- the view of a clip at another frame rate, an entry point of libagmv_hip.so beside those of
 * include/agmv_hip.h and include/agmv_hip_view_source.h (same context, same conventions: plain pointers and sizes, non-zero with a
 * message in agmv_hip_last_error() on refusal).
 */
#ifndef AGMV_HIP_TIME_H
#define AGMV_HIP_TIME_H

#include "agmv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- frames j0 .. j0 + count - 1 of R, the view V of a source clip resampled in time (AGMV_RATE of include/agmv.h holds the rule) ------
 * V is the clip agmv_hip_view_source_async gives for the same fmt, d_src, src_w, src_h, first, step, x, y, win_w, win_h and
 * count = view_len: frame k of V is the window of source frame first + k * step, read by the layout's rule; bits 24 .. 31 of an
 * XRGB32 source are not read.  The rate rate_src : rate_dst is given reduced (gcd 1, both 1 .. 65535); R has
 * m = (view_len * rate_dst) div rate_src frames.  time_filter is an AGMV_TIME: AGMV_TIME_AREA (2, rate_dst <= rate_src) gives
 *   R[j] = (sum over k of wt(j, k) * V[k] + rate_src div 2) div rate_src   per channel of R, G, B,
 * wt(j, k) the overlap of [k * rate_dst, (k + 1) * rate_dst) and [j * rate_src, (j + 1) * rate_src); AGMV_TIME_NEAREST (1, any rate)
 * gives R[j] = V[((2j + 1) * rate_src) div (2 * rate_dst)].  d_dst receives count frames of win_w * win_h packed words
 * 0x00RRGGBB, frame j of R at d_dst + (j - j0) * win_w * win_h; bits 24 .. 31 are 0 for either filter.  One launch, asynchronous on
 * `stream`: no allocation, no host synchronisation, nothing of the context is used but its device.  A lane owns 16 consecutive
 * pixels of an output row (NV12 / I420: a patch of 8 x 2, which is what the registers hold) and walks the taps of its output frame with three 32-bit sums per
 * pixel, exact because 255 * 65535 + 32767 < 2^32.  The 16-byte non-temporal loads of the whole-clip converters are used where
 * d_src and the frames' size are multiples of 16 bytes and a group's 16 source pixels lie inside their row on a 16-byte boundary
 * (NV12 / I420: 8-byte loads, x and src_w multiples of 8 and an even y), 16-byte stores where win_w is a multiple of 4 and d_dst is 16-byte
 * aligned; everything else goes element by element, to the same words.  A launch spreads at most 65535 output frames over the
 * grid; a longer batch takes further trips round the kernel's frame loop.  Nothing outside the count target frames is written.
 * Returns non-zero with a message and launches nothing for a NULL pointer, a zero size, step == 0, a window that does not lie
 * inside the source frame, an unknown format, an NV12 / I420 source of odd width or height, an unknown filter, a rate that is
 * zero, above 65535 or not reduced, AGMV_TIME_AREA with rate_dst > rate_src, j0 + count > m, or a view that does not lie inside
 * the n_frames of the clip (first + (view_len - 1) * step >= n_frames: a tap outside the clip is refused, never read); otherwise
 * count == 0 is success and launches nothing. */
int agmv_hip_time_frames_async(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t src_w, uint32_t src_h, uint32_t n_frames,
                               uint32_t first, uint32_t step, uint32_t view_len, uint32_t x, uint32_t y, uint32_t win_w, uint32_t win_h,
                               uint32_t rate_src, uint32_t rate_dst, int time_filter, uint32_t j0, uint32_t count, uint32_t* d_dst,
                               void* stream);

#ifdef __cplusplus
}
#endif

#endif
