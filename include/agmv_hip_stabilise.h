/*
 * include/agmv_hip_stabilise.h -- temporal stabilisation of a batch of frames, an entry point of libagmv_hip.so beside those of
 * include/agmv_hip.h (same context, same conventions: plain pointers and sizes, non-zero with a message in agmv_hip_last_error()
 * on refusal).
 */
#ifndef AGMV_HIP_STABILISE_H
#define AGMV_HIP_STABILISE_H

#include "agmv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- temporal stabilisation: still blocks of a P-frame take the pixels of their GOP's I-frame --------
 * The rule of include/agmv.h ("temporal stabilisation"), which holds the definition, on d_pix: n_frames packed XRGB32 frames of
 * w x h with frame counts first_fc, first_fc + 1, ..., changed in place.  d_replaced may be NULL; otherwise it is a device
 * unsigned long long to which the number of replaced blocks is ADDED (the caller sets it to zero; integer adds, so the same
 * clip gives the same count from run to run).  One launch, asynchronous on `stream`: no allocation, no host synchronisation,
 * nothing of the context is used but its device.  One lane owns one 4x4 block of one GOP, lanes run over a frame's blocks in
 * row-major order and the GOPs lie on the grid's second axis (at most 65535 per trip round the kernel's GOP loop): four 16-byte
 * loads of the I-frame's rows and four per P-frame of the GOP that the batch holds, all issued before the first use, four
 * 16-byte stores per still block and none otherwise.  A d_pix that is not 16-byte aligned takes word accesses to the same words.
 * Every frame offset is 64-bit.  Returns non-zero with a message and launches nothing for a NULL context, a NULL d_pix or one
 * that is not 4-byte aligned, a width or height that is zero or no multiple of 4 (or 2^31 pixels and more), or a strength
 * outside 1 .. 64; otherwise n_frames == 0 is success and launches nothing, as is a batch without a P-frame whose I-frame it
 * holds. */
int agmv_hip_stabilise_frames_async(agmv_hip_ctx* ctx, uint32_t strength, uint32_t* d_pix, uint32_t w, uint32_t h, uint32_t n_frames,
                                    uint32_t first_fc, unsigned long long* d_replaced, void* stream);

#ifdef __cplusplus
}
#endif

#endif
