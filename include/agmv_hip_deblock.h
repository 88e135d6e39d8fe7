/*
 * include/agmv_hip_deblock.h -- deblocking of a decoded clip, an entry point of libagmv_hip.so beside those of include/agmv_hip.h
 * (same context, same conventions: plain pointers and sizes, non-zero with a message in agmv_hip_last_error() on refusal).
 */
#ifndef AGMV_HIP_DEBLOCK_H
#define AGMV_HIP_DEBLOCK_H

#include "agmv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- deblocking: the edges of the 4x4 block grid of a decoded clip smoothed, vertical edges first, then horizontal ones --------
 * The rule of include/agmv.h ("deblocking"), which holds the definition, from d_src to d_dst: n_frames packed XRGB32 frames of
 * w x h each.  d_dst == d_src is allowed; any other overlap is the caller's error.  d_counts may be NULL; otherwise it is two
 * device unsigned long long, [0] the weak and [1] the strong lines of both stages, to which the call's counts are ADDED (the
 * caller sets them to zero; integer adds, so the same clip gives the same counts from run to run).  One launch, asynchronous on
 * `stream`: no allocation, no host synchronisation, nothing of the context is used but its device.  One lane owns one 4x4 cell
 * around a block corner (pixels 4i-2 .. 4i+1 x 4j-2 .. 4j+1, clipped at the rim), whose output depends on its own input alone;
 * lanes run over a frame's (w/4 + 1) x (h/4 + 1) cells in row-major order and the frames lie on the grid's second axis, as many
 * rows as make 16384 workgroups and at most 65535, a longer clip taking further trips round the kernel's frame loop.  A row of
 * a cell is one 16-byte access at 8-byte alignment where both pointers are 8-byte aligned, and word accesses to the same words
 * otherwise.  Every frame offset is 64-bit.  Returns non-zero with a message and launches nothing for a NULL context, a NULL
 * d_src or d_dst or one that is not 4-byte aligned, a width or height that is zero or no multiple of 4 (or 2^31 pixels and
 * more), or a strength outside 1 .. 64; otherwise n_frames == 0 is success and launches nothing. */
int agmv_hip_deblock_frames_async(agmv_hip_ctx* ctx, uint32_t strength, const uint32_t* d_src, uint32_t w, uint32_t h, uint32_t n_frames,
                                  uint32_t* d_dst, unsigned long long* d_counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif
