/*
 * include/agmv_hip.h -- the C-ABI drop-in boundary of the MI355X hot path.
 *
 * libagmv has no plugin/FFI layer: consumers call its C API directly
 * (reference include/agmv_encode.h:26-37, include/agmv_decode.h:21-26).  The
 * per-frame functions of that API are FILE*-coupled, one frame per call, and
 * take LP64 `unsigned long` pixels (8 B/px, reference include/agmv_defines.h:22)
 * -- a shape no GPU can be fed through.  This header therefore declares the
 * batch entry points that the reference-compatible host layer (include/agmv.h,
 * libagmv_amd/csrc/agmv_api.c) is built on, and that a maintainer of the
 * reference would bind.  Plain pointers and sizes only.
 *
 * Conventions
 *   pixel   4-byte 0x00RRGGBB (bits >= 24 ignored, reference src/agmv_utils.c:632-642)
 *   frame   w*h pixels, row-major, w and h multiples of 4 (reference src/agmv_encode.c:365-366)
 *   entry   u16 = pal_num << 8 | index   (GPU form of AGMV_ENTRY, include/agmv_defines.h:122-126)
 *   d_*     device pointers (HIP), h_* host pointers; `stream` is a hipStream_t (NULL = default)
 *   return  0 on success, negative on error (agmv_hip_last_error() gives the text).
 *           There is NO CPU fallback: without a usable GPU every entry point fails.
 */
#ifndef AGMV_HIP_H
#define AGMV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agmv_hip_ctx agmv_hip_ctx;

/* bytes a frame's pre-LZ bitstream can take at most: 33 (512-colour) or 17 (256-colour)
   bytes per 4x4 block (reference src/agmv_encode.c:381-403 / :420-431), rounded up to 256.
   NOTE the reference's own buffer (w*h*2, src/agmv_utils.c:338) is too small for the
   512-colour worst case. */
size_t agmv_hip_max_usize(uint32_t w, uint32_t h, int mode512);

int          agmv_hip_device_count(void);
agmv_hip_ctx* agmv_hip_create(int device);
void         agmv_hip_destroy(agmv_hip_ctx* ctx);
const char*  agmv_hip_last_error(void);

/* -- palette ------------------------------------------------------------------------------
 * Replaces the per-pixel 256/512-way search of AGMV_FindNearestColor / AGMV_FindNearestEntry
 * (reference src/agmv_utils.c:785-816, :851-895) by an exact 2^24-entry table built ONCE per
 * palette on the GPU with the same argmin and the same tie rules (lowest index inside a
 * palette, palette0 on cross-palette ties).  Also builds the 512x512 "within +-2 per channel"
 * bit matrix used by the block tests (reference src/agmv_encode.c:293, :345).
 * mode512: 1 = two palettes (OPT_I/III/GBA_I/GBA_III/NDS, container v1/v3),
 *          0 = palette0 only (OPT_II/ANIM/GBA_II, container v2/v4). */
int agmv_hip_set_palette(agmv_hip_ctx* ctx, const uint32_t p0[256], const uint32_t p1[256],
                         int mode512, void* stream);

/* exact nearest entries for n pixels (loop A of AGMV_EncodeFrame, src/agmv_encode.c:556-558 /
   :589-592) -- exposed for parity tests of the table. */
int agmv_hip_quantise_dev(agmv_hip_ctx* ctx, const uint32_t* d_pix, size_t n, uint16_t* d_entries,
                          void* stream);

/* -- pattern dithering ----------------------------------------------------------------------
 * The dither of include/agmv.h ("pattern dithering"), which holds the definition, against the context's palette and its exact
 * table: every pixel of n_frames packed frames of w x h at d_pix is replaced, in place, by one of 16 palette colours whose mean
 * approaches it, picked by the 4x4 threshold matrix at (x & 3, y & 3) of the pixel's position inside its own frame.  strength
 * 1 .. 64.  Any w, h >= 1 (not only multiples of 4); d_pix 4-byte aligned; bits >= 24 are ignored on input and 0 on output;
 * nothing outside the n_frames frames is written.  Asynchronous on `stream`: one launch, no allocation, no host synchronisation.
 * Returns non-zero with a message, touches nothing and launches nothing for a NULL pointer, a context without a palette,
 * strength 0 or above 64, a zero size, or w * h >= 2^31 (the index inside a frame is 32 bits wide; the frames' bases are 64-bit
 * offsets, so n_frames has no bound of its own).  n_frames == 0 is success and launches nothing. */
int agmv_hip_dither_frames_async(agmv_hip_ctx* ctx, uint32_t strength, uint32_t* d_pix,
                                 uint32_t w, uint32_t h, uint32_t n_frames, void* stream);

/* -- encode -------------------------------------------------------------------------------
 * Loops A+B of AGMV_EncodeFrame for n_frames consecutive frames (reference
 * src/agmv_encode.c:552-565 / :589-599, :626-630): quantise, I/P block classification
 * (CompareIFrameBlock :302-352, ComparePFrameBlock :240-300), byte assembly
 * (AssembleIFrameBitstream :354-436, AssemblePFrameBitstream :438-527).
 * Frame f of the batch has frame_count = first_frame_count + f; it is an I-frame when
 * frame_count % 4 == 0.  d_out receives frame f's pre-LZ bitstream at d_out + f*out_stride
 * (out_stride >= agmv_hip_max_usize), d_sizes[f] its length (`usize`).
 * d_iframe_entries (w*h u16, may be NULL): if the batch starts inside a GOP
 * (first_frame_count % 4 != 0) it supplies the entries of that GOP's I-frame
 * (agmv->iframe_entries); on return it holds the entries of the last I-frame of the batch. */
int agmv_hip_encode_frames_dev(agmv_hip_ctx* ctx, const uint32_t* d_pix, uint32_t n_frames,
                               uint32_t w, uint32_t h, uint32_t first_frame_count,
                               uint8_t* d_out, size_t out_stride, uint32_t* d_sizes,
                               uint16_t* d_iframe_entries, void* stream);
/* same from/to host memory (does the H2D/D2H itself, synchronous) */
int agmv_hip_encode_frames(agmv_hip_ctx* ctx, const uint32_t* h_pix, uint32_t n_frames,
                           uint32_t w, uint32_t h, uint32_t first_frame_count,
                           uint8_t* h_out, size_t out_stride, uint32_t* h_sizes,
                           uint16_t* h_iframe_entries);

/* The same on planes of ENTRIES instead of pixels: word k of frame f holds pal_num << 8 | index of pixel k.  The
   quantisation is skipped; classification and assembly are those of AGMV_AssembleIFrameBitstream /
   AGMV_AssemblePFrameBitstream on that AGMV_ENTRY plane (reference src/agmv_encode.c:354-436, :438-527). */
int agmv_hip_encode_entries_dev(agmv_hip_ctx* ctx, const uint32_t* d_entries, uint32_t n_frames,
                                uint32_t w, uint32_t h, uint32_t first_frame_count,
                                uint8_t* d_out, size_t out_stride, uint32_t* d_sizes,
                                uint16_t* d_iframe_entries, void* stream);
int agmv_hip_encode_entries(agmv_hip_ctx* ctx, const uint32_t* h_entries, uint32_t n_frames,
                            uint32_t w, uint32_t h, uint32_t first_frame_count,
                            uint8_t* h_out, size_t out_stride, uint32_t* h_sizes,
                            uint16_t* h_iframe_entries);

/* nearest colour / entry of n pixels against palettes that need not be the context's (no table is built):
   AGMV_FindNearestColor (mode512 = 0, entry = index in p0) / AGMV_FindNearestEntry (mode512 = 1), reference
   src/agmv_utils.c:785-816, :851-895.  Host buffers, synchronous; the device scratch is cached in the context. */
int agmv_hip_nearest(agmv_hip_ctx* ctx, const uint32_t p0[256], const uint32_t p1[256], int mode512,
                     const uint32_t* h_pix, size_t n, uint16_t* h_entries);

/* number of the 16 colour pairs (a[k], b[k]) that are within +-2 on R, G and B: the count AGMV_CompareIFrameBlock
   (b = the block's reference colour 16 times) and AGMV_ComparePFrameBlock (b = the I-frame entries' colours) return
   (reference src/agmv_encode.c:302-352, :240-300).  Returns 0..16, negative on error. */
int agmv_hip_within2_count(agmv_hip_ctx* ctx, const uint32_t a[16], const uint32_t b[16]);

/* Notes on a context:
 *  - device memory: 512 MiB of address space for the colour -> entry table (32 MiB of it populated, see
 *    k_lut_build in agmv_hip.hip), plus per-batch work areas grown on demand (look-back status 8 B per tile and
 *    frame, parser workspace <= 15 % of the bitstream slab; LZSS: about 29 bytes per position of the largest chunk of a
 *    batch, at most 2^24 positions, ~460 MiB; LZ77: 5 bytes per input byte of the largest chunk of a batch, at most
 *    2^26 bytes, 320 MiB);
 *  - agmv_hip_set_palette builds the tables on `stream` (contexts of a device that hold the same palette share one set: a
 *    context that finds it makes `stream` wait for the build, wherever that runs, and does not wait itself).  It is not
 *    asynchronous: a call that builds sends the colours up from the caller's memory and waits for `stream` once before
 *    its kernels; a call that replaces the context's palette waits for the device.  So it MAY wait, and need not.
 *    The tables are complete for work submitted to THAT stream afterwards; work of the context on another stream must
 *    be ordered behind it by the caller (an event, or a synchronisation of the stream);
 *  - the encode entry points of ONE context share its look-back status and control words: a second encode is
 *    ordered behind the first (on another stream it waits for it through an event); use one context per
 *    concurrent encoder;
 *  - likewise the parse / decode entry points of ONE context share its parser work areas and repair bitmap: calls on
 *    different streams of one context must not overlap; use one context per concurrent decoder;
 *  - the LZ-decode entry points of ONE context upload their per-call tables from one pinned staging buffer: a call returns
 *    without waiting for the stream (agmv_hip_lz_decode_frames_sized_dev: for nothing at all) only when the upload of the
 *    PREVIOUS call of that context has ended; otherwise it waits on the host for that upload (not for the kernels behind it)
 *    before it rewrites the buffer.  The results are the same either way;
 *  - agmv_hip_dither_frames_async reads the context's tables and nothing else of it: with respect to agmv_hip_set_palette
 *    it is ordered like an encode (the tables are complete for work submitted to the palette's stream afterwards), and it
 *    may run beside the context's encodes and decodes on other streams;
 *  - a device-side wait that runs into its bound (never observed on a healthy GPU) makes agmv_hip_check fail AND
 *    overwrites every size of that batch with 0xFFFFFFFF, so the bytes cannot be taken for valid ones. */

/* -- decode -------------------------------------------------------------------------------
 * The parse + reconstruct half of AGMV_DecodeFrameChunk (reference src/agmv_decode.c:224-407)
 * for n_frames consecutive frames whose LZ stage (:171-222, host) has already run.
 *   d_bits + f*bits_stride : frame f's decompressed bitstream; bytes [bpos, bpos+16) must hold
 *                            what the reference's persistent buffer holds there (stale bytes of
 *                            earlier frames, or 0) -- they are read on over-run.
 *   d_bpos[f]              : bitstream->pos after the LZ stage (may differ from usize).
 * agmv_hip_parse_frames_dev computes, per frame, the byte position at which each 4x4 block is
 * entered (d_offsets[f*nblk + k]) and how many blocks are entered before the reference raises
 * `escape` (d_nentered[f]) -- by speculative per-piece walks that are PROVEN per frame to be the serial parse, and by the
 * map / stitch / emit kernels for the frames that cannot be proven (AGMV_HIP_PARSE=robust in the
 * environment runs the latter alone, =serial a one-lane walk: debugging aids, same outputs).
 * agmv_hip_decode_frames_dev turns that into pixels:
 * d_pix_out + f*w*h.  d_prev_frame / d_prev_iframe (w*h pixels, may be NULL = zeroed, the state
 * of a fresh decoder) are img_data / iframe->img_data before the first frame of the batch;
 * blocks the bitstream does not reach keep the previous frame's pixels (:229-232). */
int agmv_hip_parse_frames_dev(agmv_hip_ctx* ctx, const uint8_t* d_bits, size_t bits_stride,
                              const uint32_t* d_bpos, uint32_t n_frames, uint32_t w, uint32_t h,
                              uint32_t* d_offsets, uint32_t* d_nentered, void* stream);
int agmv_hip_decode_frames_dev(agmv_hip_ctx* ctx, const uint8_t* d_bits, size_t bits_stride,
                               const uint32_t* d_bpos, const uint32_t* d_offsets,
                               const uint32_t* d_nentered, uint32_t n_frames, uint32_t w,
                               uint32_t h, uint32_t first_frame_count, uint32_t* d_pix_out,
                               const uint32_t* d_prev_frame, const uint32_t* d_prev_iframe,
                               void* stream);
/* How many frames of the last agmv_hip_parse_frames_dev call (of the last range, for agmv_hip_parse_decode_frames_dev; of
   the whole call, whatever its ranges, for agmv_hip_decode_bitstreams_dev) the speculative parser could not prove and left to the robust kernels (0 for streams the encoder emits unless a
   long run of FILL blocks carries a flag-valued index; damaged streams typically land here).  A statistic: the
   outputs are the same either way.  Synchronises the stream; negative on error. */
int agmv_hip_parse_fallback_frames(agmv_hip_ctx* ctx, void* stream);
/* Both steps as ONE call.  Same inputs, same outputs (d_offsets / d_nentered are written as by
   agmv_hip_parse_frames_dev), same pixels.  With AGMV_DEC_SLICES=n in the environment the batch is cut into n ranges of
   GOPs, the parser runs on a stream the context owns and the reconstruction of a range waits only for the parse of that
   range (measured: no gain on MI355X, the default is one range).  Everything is ordered after the work already on
   `stream`, and `stream` is complete only when the whole call is. */
int agmv_hip_parse_decode_frames_dev(agmv_hip_ctx* ctx, const uint8_t* d_bits, size_t bits_stride,
                                     const uint32_t* d_bpos, uint32_t n_frames, uint32_t w, uint32_t h,
                                     uint32_t first_frame_count, uint32_t* d_offsets, uint32_t* d_nentered,
                                     uint32_t* d_pix_out, const uint32_t* d_prev_frame,
                                     const uint32_t* d_prev_iframe, void* stream);
/* The same result without offsets[]: the parser's block-entry bitmaps (one bit per byte of stream) go straight to the
   reconstruction kernel, which ranks its own blocks in them; frames the speculative parser cannot prove get their bits from
   the robust kernels.  This is the form the sequence drivers and bench.py use: it saves the 4 bytes per block that
   agmv_hip_parse_frames_dev writes and agmv_hip_decode_frames_dev reads back (reference: the block loop of
   AGMV_DecodeFrameChunk, src/agmv_decode.c:224-407, has no such table either -- it walks).  d_nentered may be NULL.
   Any number of frames.  A long batch is cut at GOP boundaries into ranges that run one after the other on `stream`, each
   one parser -> reconstruction -> repair from the pixels the range before it left: a range is as many whole GOPs as decode
   to at most 512 frames' worth of 1920x1080 pixels (4.2 GB: 512 frames of 1080p, 1152 of 720p, 13824 of 320x240), and never
   more than 65532 frames.  That keeps the streams the parser has just read in the memory-side cache for the reconstruction
   that follows (MI355X: 256 MiB) and the parser's work areas one range long.  A batch no longer than a range runs as one.
   AGMV_DEC_RANGE_FRAMES=n in the environment (read per call; a test and tuning aid) forces ranges of n frames, rounded up to
   whole GOPs; 0 cuts at 65532 frames only.  The outputs, agmv_hip_decode_prior_dependent and
   agmv_hip_parse_fallback_frames answer for the whole call whatever the ranges. */
int agmv_hip_decode_bitstreams_dev(agmv_hip_ctx* ctx, const uint8_t* d_bits, size_t bits_stride,
                                   const uint32_t* d_bpos, uint32_t n_frames, uint32_t w, uint32_t h,
                                   uint32_t first_frame_count, uint32_t* d_nentered, uint32_t* d_pix_out,
                                   const uint32_t* d_prev_frame, const uint32_t* d_prev_iframe, void* stream);
/* After agmv_hip_decode_frames_dev / agmv_hip_parse_decode_frames_dev / agmv_hip_decode_bitstreams_dev: 1 when a pixel of that batch derives from d_prev_frame / d_prev_iframe (a block the
   bitstream did not rewrite before it was read: stale tail after `escape`, COPY in the first GOP, a FILL / NORMAL block cut
   off by bpos -- reference src/agmv_decode.c:229-232, :268-271, :277-285, :310-314), 0 when the batch is a function of its
   own bitstreams alone, negative on error.  Exact: tracked per pixel over the whole batch (a batch that starts inside a GOP
   also depends through a COPY in its first I-frame, which reads d_prev_iframe), so 1 means some output pixel changes with
   the prior state.  What a GOP-sharded decode needs to know before it trusts a range decoded from the fresh state.  Never 1 for a
   stream the encoder emits that starts at a GOP boundary, with one exception: at width 4 (one block per row) a FILL as the
   last block of the first frame stores the block's own pixel (3,0) of d_prev_frame (the reference's x-1 wraps, :264-266).
   A decode_bitstreams call cut into ranges reports its dependence on the caller's state, i.e. that of its first range:
   later ranges continue from the output of the range before them (the first range always holds the batch's first
   I-frame, the last frame that can read d_prev_iframe).  Synchronises the stream. */
int agmv_hip_decode_prior_dependent(agmv_hip_ctx* ctx, uint32_t w, uint32_t h, void* stream);
/* host-memory convenience: parse on the GPU, reconstruct, copy back (synchronous) */
int agmv_hip_decode_frames(agmv_hip_ctx* ctx, const uint8_t* h_bits, size_t bits_stride,
                           const uint32_t* h_bpos, uint32_t n_frames, uint32_t w, uint32_t h,
                           uint32_t first_frame_count, uint32_t* h_pix_out,
                           const uint32_t* h_prev_frame, const uint32_t* h_prev_iframe);

/* -- exchange step of the GOP-sharded encoder (the reference is single-process: its "gather" is the frame
 * loop of AGMV_EncodeAGMV appending chunk after chunk, src/agmv_encode.c:3610-3612) --------------------------------
 * A rank's bitstreams travel as ONE contiguous message: the used bytes of every slab row back to back.
 * agmv_hip_pack_frames_dev:   d_slab [n_frames][stride] + d_sizes[n_frames] (as agmv_hip_encode_frames_dev leaves them)
 *                             -> d_msg (sum of the sizes bytes; the caller sizes it, e.g. from the sizes it exchanges first)
 *                             and d_offsets[n_frames + 1] (u64: frame f starts at d_offsets[f]; [n_frames] = the total).
 * agmv_hip_unpack_frames_dev: the inverse on the receiving rank: d_msg + d_sizes -> rows of a slab (stride a multiple of 4;
 *                             bytes of a row behind its size are left as they are); d_offsets is scratch of n_frames + 1 u64.
 * Both are asynchronous on `stream`; what moves the message between the ranks (RCCL send/recv, hipMemcpyPeer, a host
 * socket) is the caller's business. */
int agmv_hip_pack_frames_dev(agmv_hip_ctx* ctx, const uint8_t* d_slab, size_t stride, const uint32_t* d_sizes,
                             uint32_t n_frames, uint8_t* d_msg, unsigned long long* d_offsets, void* stream);
int agmv_hip_unpack_frames_dev(agmv_hip_ctx* ctx, const uint8_t* d_msg, const uint32_t* d_sizes, uint32_t n_frames,
                               uint8_t* d_slab, size_t stride, unsigned long long* d_offsets, void* stream);

/* -- LZSS stage of the encoder (AGMV_LZSS + the csize handling of AGMV_EncodeFrame, reference src/agmv_encode.c:106-177,
 * :567-585, :622-624; AGMV_FlushWriteBits src/agmv_utils.c:106-112) ------------------------------------------------
 * agmv_hip_lzss_max_csize: bytes a payload row must hold for a pre-LZ bitstream of n bytes (ceil(9n/8) all-literal, plus
 *                          one byte for the float rounding of csize).
 * agmv_hip_lzss_frames_dev: row f = d_bits + f*bits_stride, d_sizes[f] bytes (as agmv_hip_encode_frames_dev leaves them);
 *                          d_out + f*out_stride receives exactly the csize payload bytes the reference's file holds for that
 *                          frame (the partial last byte when the float csize counts it, its unused high bits 0; bytes of
 *                          the row behind csize are left as they are), d_csize[f] its csize field.  Sizes may differ and
 *                          be 0; each must be < 2^24 and out_stride >= agmv_hip_lzss_max_csize of it.  Bit-exact with the
 *                          reference (longest match <= 15 in the 65535-byte window, earliest start among equals).
 *                          Asynchronous on `stream` except that it synchronises the stream once, before its kernels, to
 *                          read d_sizes (they decide how the batch is cut into chunks).  Calls on one context share its LZ
 *                          work areas: they must not overlap.  The payload rows of a batch travel to the host as one
 *                          message through agmv_hip_pack_frames_dev with d_csize as the sizes.
 * agmv_hip_lzss_frames:     the same from/to host memory (synchronous). */
size_t agmv_hip_lzss_max_csize(size_t n);
int agmv_hip_lzss_frames_dev(agmv_hip_ctx* ctx, const uint8_t* d_bits, size_t bits_stride, const uint32_t* d_sizes,
                             uint32_t n_frames, uint8_t* d_out, size_t out_stride, uint32_t* d_csize, void* stream);
int agmv_hip_lzss_frames(agmv_hip_ctx* ctx, const uint8_t* h_bits, size_t bits_stride, const uint32_t* h_sizes,
                         uint32_t n_frames, uint8_t* h_out, size_t out_stride, uint32_t* h_csize);

/* -- LZ77 stage of the encoder (AGMV_LZ77, reference src/agmv_encode.c:179-238; its csize :236; the byte behind the stream
 * that a match running to the end emits, :222, read from the reference's one persistent bitstream buffer) ---------------
 * agmv_hip_lz77_max_csize: bytes a payload row must hold for a pre-LZ bitstream of n bytes: 4 * n, every byte a token.
 * agmv_hip_lz77_peek_dev:  the persistent buffer over the n_frames rows, in frame order (reference :222 with the buffer
 *                          AGMV_EncodeFrame fills, src/agmv_encode.c:561-566): d_peek[f] = size_f < persist_len ?
 *                          buffer[size_f] : 0, then buffer[0, min(size_f, persist_len)) = row f.  d_persist (persist_len
 *                          bytes) is updated in place and carries over to the next batch.  Asynchronous on `stream`.
 * agmv_hip_lz77_frames_dev: rows and sizes as for agmv_hip_lzss_frames_dev.  d_out + f*out_stride receives the 4-byte
 *                          tokens {dist lo, dist hi, len, next} of the reference's greedy parse (longest match <= 255 in
 *                          the 65535-byte window, earliest start among equals, one equal byte is a match), d_csize[f] =
 *                          4 * tokens (reference :236).  The token of a match that ends exactly at size_f takes `next`
 *                          from d_peek[f] (NULL = zeros); a row is never read past its size.  Sizes may differ and be 0;
 *                          each must be < 2^24 and out_stride >= agmv_hip_lz77_max_csize of it, else an error return.
 *                          Bytes of a row behind csize are left as they are.  Asynchronous on `stream` except that it
 *                          synchronises the stream once, before its kernels, to read d_sizes.  Calls on one context share
 *                          its LZ77 work areas: they must not overlap.
 *                          Memory: the work areas hold 5 bytes per input byte of a chunk of frames (a chunk is at most
 *                          2^26 bytes of input: 320 MiB), grown on demand and kept by the context.
 * agmv_hip_lz77_frames:    peek + compress from/to host memory (synchronous).  h_persist (persist_len bytes) is the buffer
 *                          before the call and receives it after; NULL = zeroed and not returned.
 * agmv_hip_lz77_reparsed_segments: segments of the last agmv_hip_lz77_frames_dev call whose speculative parse did not
 *                          start on the true token chain and were parsed again from their true entry.  A statistic, like
 *                          agmv_hip_parse_fallback_frames: the outputs are the same either way.  Synchronises the stream. */
size_t agmv_hip_lz77_max_csize(size_t n);
int agmv_hip_lz77_peek_dev(agmv_hip_ctx* ctx, const uint8_t* d_bits, size_t bits_stride, const uint32_t* d_sizes,
                           uint32_t n_frames, uint8_t* d_persist, size_t persist_len, uint8_t* d_peek, void* stream);
int agmv_hip_lz77_frames_dev(agmv_hip_ctx* ctx, const uint8_t* d_bits, size_t bits_stride, const uint32_t* d_sizes,
                             uint32_t n_frames, const uint8_t* d_peek, uint8_t* d_out, size_t out_stride, uint32_t* d_csize,
                             void* stream);
int agmv_hip_lz77_frames(agmv_hip_ctx* ctx, const uint8_t* h_bits, size_t bits_stride, const uint32_t* h_sizes,
                         uint32_t n_frames, uint8_t* h_persist, size_t persist_len, uint8_t* h_out, size_t out_stride,
                         uint32_t* h_csize);
int agmv_hip_lz77_reparsed_segments(agmv_hip_ctx* ctx, void* stream);

/* -- LZ stage of the decoder (the LZSS / LZ77 decompression of AGMV_DecodeFrameChunk with its bit reader, reference
 * src/agmv_decode.c:160-222, src/agmv_utils.c:32-57; the persistent buffer agmv->bitstream->data it decompresses into) --
 * agmv_hip_lz_decode_frames_dev: version 1 or 2 is LZSS, any other value LZ77.  Frame f's payload starts at
 *                          d_src + d_off[f]; d_avail[f] bytes of it exist (reads past them return 0 and are not counted;
 *                          nothing past min(avail, csize + 3) is read), d_usize[f] / d_csize[f] are the chunk header's
 *                          fields.  Rows may overlap (a reader runs on into the guard and the next chunk header).  Row f of
 *                          d_bits (stride bits_stride >= cap) receives data[0, bpos) as agmv_lz_decode_mem writes it into a
 *                          buffer of cap bytes (lim = cap - 16), d_bpos[f] bpos and d_used[f] the payload bytes the reader
 *                          fetched, capped at avail (they decide where the next chunk is found).  Nothing else is written.
 *                          Asynchronous on `stream` except that it synchronises the stream once, before its kernels, to read
 *                          avail / usize / csize (they decide how the batch is cut into chunks); nothing else waits for
 *                          the device (the per-call tables go up from pinned staging).  cap < 2^31.
 * agmv_hip_lz_decode_frames_sized_dev: the same with h_avail / h_usize / h_csize in host memory (read before the call
 *                          returns): no stream synchronisation at all.  What a driver that has parsed the chunk headers
 *                          itself uses.
 * agmv_hip_lz_decode_commit_dev: the host driver's loop over the reference's ONE persistent buffer (d_persist, cap bytes) for
 *                          the first n_frames rows, in frame order: row f's bytes [bpos, bpos + 16), clipped to bits_stride
 *                          and to cap, become the buffer's, then the buffer's [0, min(bpos, cap)) become row f's.  The rows
 *                          are then what agmv_hip_decode_bitstreams_dev reads with d_bpos.  A separate call because only the
 *                          frames before a batch cut may reach the buffer.  Asynchronous on `stream`.
 * agmv_hip_lz_decode_fallback_frames: frames of the last agmv_hip_lz_decode_frames_dev call that the position-parallel path
 *                          left to the serial kernel (a match with offset > pos followed by further tokens, or LZ77 output
 *                          past usize + 256: damaged or crafted streams).  A statistic: the outputs are the same either way.
 *                          Synchronises the stream.
 * agmv_hip_lz_decode_frames: both from/to host memory, synchronous: h_src (src_len bytes), h_off[f] + min(avail, csize + 3)
 *                          <= src_len; rows h_bits [n_frames][bits_stride] are updated in place (bytes behind bpos + 16 keep
 *                          their content); h_persist (cap bytes, may be NULL = zeroed and not returned) is the buffer
 *                          before the call and receives it after.
 * Calls on one context share its LZ-decode work areas: they must not overlap. */
int agmv_hip_lz_decode_frames_dev(agmv_hip_ctx* ctx, int version, const uint8_t* d_src, const unsigned long long* d_off,
                                  const uint32_t* d_avail, const uint32_t* d_usize, const uint32_t* d_csize, uint32_t n_frames,
                                  uint8_t* d_bits, size_t bits_stride, size_t cap, uint32_t* d_bpos, uint32_t* d_used,
                                  void* stream);
int agmv_hip_lz_decode_frames_sized_dev(agmv_hip_ctx* ctx, int version, const uint8_t* d_src, const unsigned long long* d_off,
                                        const uint32_t* h_avail, const uint32_t* h_usize, const uint32_t* h_csize,
                                        uint32_t n_frames, uint8_t* d_bits, size_t bits_stride, size_t cap, uint32_t* d_bpos,
                                        uint32_t* d_used, void* stream);
int agmv_hip_lz_decode_commit_dev(agmv_hip_ctx* ctx, uint8_t* d_bits, size_t bits_stride, const uint32_t* d_bpos,
                                  uint32_t n_frames, uint8_t* d_persist, size_t cap, void* stream);
int agmv_hip_lz_decode_fallback_frames(agmv_hip_ctx* ctx, void* stream);
int agmv_hip_lz_decode_frames(agmv_hip_ctx* ctx, int version, const uint8_t* h_src, size_t src_len,
                              const unsigned long long* h_off, const uint32_t* h_avail, const uint32_t* h_usize,
                              const uint32_t* h_csize, uint32_t n_frames, uint8_t* h_bits, size_t bits_stride, size_t cap,
                              uint32_t* h_bpos, uint32_t* h_used, uint8_t* h_persist);

/* -- helpers on the caller side of the path -------------------------------------------------*/
/* canonical synthetic clip agmv_synth_v1: frames t0..t0+n-1 into d_pix */
int agmv_hip_synth_dev(agmv_hip_ctx* ctx, uint32_t* d_pix, uint32_t w, uint32_t h, uint32_t t0,
                       uint32_t n_frames, uint64_t seed, void* stream);
/* PDIFS midpoint frame, AGMV_InterpFrame (reference src/agmv_utils.c:949-969) */
int agmv_hip_interp_dev(agmv_hip_ctx* ctx, uint32_t* d_out, const uint32_t* d_f1,
                        const uint32_t* d_f2, size_t n_pixels, void* stream);
/* pass-1 colour histogram of the palette build: hist[AGMV_QuantizeColor(px, quality)] += 1
   (reference src/agmv_encode.c:2390-2394, src/agmv_utils.c:695-742); hist has 2^19 bins */
int agmv_hip_histogram_dev(agmv_hip_ctx* ctx, const uint32_t* d_pix, size_t n_pixels, int quality,
                           uint32_t* d_hist, void* stream);
/* the integer behind AGMV_CompareFrameSimilarity (reference src/agmv_utils.c:920-947) for every adjacent pair of a clip
   d_pix[n_frames][n_pixels]: d_counts[f], f = 0 .. n_frames - 2, = number of positions p with grey(frame f, p) ==
   grey(frame f + 1, p), grey = (R + G + B) / 3 in integers (bits >= 24 ignored).  d_counts is overwritten; any n_pixels >= 1.
   Each frame is read once.  The ratio count / (f32)n_pixels and its comparison with the leniency stay with the caller. */
int agmv_hip_similarity_dev(agmv_hip_ctx* ctx, const uint32_t* d_pix, uint32_t n_frames, size_t n_pixels,
                            uint32_t* d_counts, void* stream);
/* d_dst[f][k] = d_index[k] == 0xFFFFFFFF ? 0 : d_src[f][d_index[k]] for f < n_frames, k < n_out; source frames are
   src_frame_pixels apart, an index >= src_frame_pixels reads as 0xFFFFFFFF.  The GBA / NDS nearest scale of the sequence
   encoder, with the table built on the host. */
int agmv_hip_gather_dev(agmv_hip_ctx* ctx, const uint32_t* d_src, size_t src_frame_pixels, uint32_t n_frames,
                        const uint32_t* d_index, size_t n_out, uint32_t* d_dst, void* stream);

/* -- clips in the caller's pixel layout ---------------------------------------------------------
 * `fmt` is an AGMV_PIXFMT of include/agmv.h, by value: 1 XRGB32 (the 4-byte 0x00RRGGBB of every other entry point), 2 RGB24
 * [h][w][3] bytes R,G,B, 3 BGR24 [h][w][3] bytes B,G,R, 4 RGBA32 [h][w][4] bytes R,G,B,A (A ignored on input, 0xFF on output),
 * 5 RGB8P [3][h][w] bytes, plane R, G, B.  Frames lie back to back; the byte formats need no alignment (a clip whose frames
 * start on 16-byte boundaries is read and written with 16-byte accesses, any other byte by byte).  With XRGB32 each function
 * is the one it generalises, or a device-to-device copy.  An unknown format is an error return.
 * agmv_hip_pixfmt_frame_bytes:   bytes of a frame of n_pixels (4n, 3n, 3n, 4n, 3n); 0 for an unknown format.  Host only: needs no
 *                                context and no GPU.
 * agmv_hip_pixels_to_xrgb_dev:   d_dst[f][k] = pixel k of frame f as 0x00RRGGBB, k < n_pixels <= frame_pixels.  Source frames
 *                                are agmv_hip_pixfmt_frame_bytes(fmt, frame_pixels) bytes apart, planes frame_pixels bytes,
 *                                destination rows n_pixels words.  (The plain frame of the sequence encoder's device source,
 *                                which was a copy: agmv_hip_memcpy_async.)
 * agmv_hip_pixels_from_xrgb_dev: the inverse for whole frames of n_pixels (bits >= 24 of the source are ignored); no byte
 *                                outside the n_frames destination frames is written.  (The decoder's device sink.)
 * agmv_hip_gather_fmt_dev:       agmv_hip_gather_dev reading a source in fmt: only the pixels the table names are touched.
 * agmv_hip_histogram_fmt_dev:    agmv_hip_histogram_dev over the first n_pixels of each of n_frames frames read in fmt
 *                                (d_hist is added to).
 * agmv_hip_similarity_fmt_dev:   agmv_hip_similarity_dev on a clip in fmt (frames n_pixels apart): the same counts, each frame
 *                                read once, d_counts overwritten. */
size_t agmv_hip_pixfmt_frame_bytes(int fmt, size_t n_pixels);
int agmv_hip_pixels_to_xrgb_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, size_t frame_pixels, uint32_t n_frames, size_t n_pixels,
                                uint32_t* d_dst, void* stream);
int agmv_hip_pixels_from_xrgb_dev(agmv_hip_ctx* ctx, int fmt, const uint32_t* d_src, uint32_t n_frames, size_t n_pixels, void* d_dst,
                                  void* stream);
int agmv_hip_gather_fmt_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, size_t src_frame_pixels, uint32_t n_frames,
                            const uint32_t* d_index, size_t n_out, uint32_t* d_dst, void* stream);
int agmv_hip_histogram_fmt_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, size_t frame_pixels, uint32_t n_frames, size_t n_pixels,
                               int quality, uint32_t* d_hist, void* stream);
int agmv_hip_similarity_fmt_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t n_frames, size_t n_pixels, uint32_t* d_counts,
                                void* stream);

/* -- clips in 8-bit YUV 4:2:0 --------------------------------------------------------------------
 * `fmt` is AGMV_PIXFMT_NV12 (16) or AGMV_PIXFMT_I420 (17) of include/agmv.h, which defines the layouts and the arithmetic,
 * OR-ed with AGMV_YUV_BT709 (0x100) and / or AGMV_YUV_FULL_RANGE (0x200).  The chroma of a pixel depends on its x and y, so
 * these take the frame's w and h where the functions above take a pixel count.  Frames lie back to back, no alignment is needed
 * (w a multiple of 16 and a clip on a 16-byte boundary are read and written in patches of 16 x 2 pixels with 16-byte accesses,
 * anything else byte by byte).  Any other format or flag is an error return.
 * agmv_hip_yuv_frame_bytes:    w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2); 0 for anything that is not one of the two formats.
 *                              Host only: needs no context and no GPU.
 * agmv_hip_yuv_to_xrgb_dev:    d_dst[f][k] = pixel k (raster order) of frame f as 0x00RRGGBB, k < n_pixels <= w * h;
 *                              destination rows n_pixels words.
 * agmv_hip_yuv_from_xrgb_dev:  whole frames of w * h packed pixels (bits >= 24 ignored) written as YUV; no byte outside the
 *                              n_frames destination frames is written.  (The decoder's device sink.)
 * agmv_hip_yuv_gather_dev:     agmv_hip_gather_dev reading a YUV source: d_index holds y * w + x (agmv_source_index); only the
 *                              pixels the table names, and their chroma, are read.
 * agmv_hip_yuv_histogram_dev:  agmv_hip_histogram_dev over the first n_pixels of each of n_frames frames (d_hist is added to).
 * agmv_hip_yuv_similarity_dev: agmv_hip_similarity_dev on the clip: the same counts, each frame read once, d_counts
 *                              overwritten. */
size_t agmv_hip_yuv_frame_bytes(int fmt, uint32_t w, uint32_t h);
int agmv_hip_yuv_to_xrgb_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames, size_t n_pixels,
                             uint32_t* d_dst, void* stream);
int agmv_hip_yuv_from_xrgb_dev(agmv_hip_ctx* ctx, int fmt, const uint32_t* d_src, uint32_t w, uint32_t h, uint32_t n_frames, void* d_dst,
                               void* stream);
int agmv_hip_yuv_gather_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames,
                            const uint32_t* d_index, size_t n_out, uint32_t* d_dst, void* stream);
int agmv_hip_yuv_histogram_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames, size_t n_pixels,
                               int quality, uint32_t* d_hist, void* stream);
int agmv_hip_yuv_similarity_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t w, uint32_t h, uint32_t n_frames,
                                uint32_t* d_counts, void* stream);

/* -- a clip scaled down with the exact box filter ----------------------------------------------------
 * AGMV_SCALE_AREA of include/agmv.h, which holds the definition: every channel of a target pixel is the mean of the source
 * pixels under it, weighted by the overlap, in integers and rounded half up.  `fmt` is any of the seven layouts above (1 .. 5,
 * or 16 / 17 OR-ed with the YUV flags); the channels are averaged in RGB after the layout's reading rule.  The n_frames source
 * frames of src_w x src_h lie back to back at the layout's frame stride (agmv_hip_pixfmt_frame_bytes / agmv_hip_yuv_frame_bytes)
 * and need no alignment beyond the layout's own (frames on 16-byte boundaries are read with 16-byte loads; YUV also needs
 * src_w % 16 == 0 for that).  d_dst[f][Y][X], dst_w * dst_h words per frame, receives 0x00RRGGBB; nothing else is written.
 * One kernel, asynchronous on `stream`; each source frame is read once (the rows that lie under two target rows twice), no
 * temporary is allocated, the result does not depend on the launch.  Any n_frames.  Returns non-zero and launches nothing for
 * an unknown format, a zero size, dst_w > src_w, dst_h > src_h or src_w * src_h > 2^24 (the bound of the 32-bit sums). */
int agmv_hip_scale_area_dev(agmv_hip_ctx* ctx, int fmt, const void* d_src, uint32_t src_w, uint32_t src_h, uint32_t n_frames,
                            uint32_t dst_w, uint32_t dst_h, uint32_t* d_dst, void* stream);

/* -- a decoded clip written at a target size -------------------------------------------------------
 * AGMV_SCALE_NEAREST (1) and AGMV_SCALE_BILINEAR (3) of include/agmv.h, which holds both definitions, as the decoder's sink:
 * d_src holds n_frames packed XRGB32 frames of src_w x src_h (bits >= 24 ignored, 4-byte aligned); frame k of the scaled clip lands
 * k * (frame bytes of `fmt` at dst_w x dst_h) bytes into d_dst, written in `fmt` by that layout's writing rule -- any of the seven
 * layouts (1 .. 5, or 16 / 17 OR-ed with the YUV flags; NV12 / I420 take luma per target pixel and chroma from the 2 x 2 block of
 * target pixels that exist).  Any non-zero sizes of at most 2^28 pixels, in either direction.  One launch, asynchronous on
 * `stream`: no allocation, no host synchronisation, nothing of the context is used but its device, and no XRGB32 copy of the
 * scaled clip exists.  Where dst_w % 16 == 0 and every target frame (and plane) starts on a 16-byte boundary (YUV: and dst_h is
 * even) the pixels leave in 16-byte stores; any other target is written pixel by pixel, to the same bytes.  Nothing outside the n_frames target frames is
 * written.  n_frames == 0 is success and launches nothing.  Returns non-zero with a message and launches nothing for a NULL
 * pointer, an unknown format or filter, AGMV_SCALE_AREA (2: that filter is agmv_hip_scale_area_dev's), a zero size or a size
 * above 2^28 pixels. */
int agmv_hip_scale_frames_async(agmv_hip_ctx* ctx, int filter, const uint32_t* d_src, uint32_t src_w, uint32_t src_h,
                                uint32_t n_frames, int fmt, uint32_t dst_w, uint32_t dst_h, void* d_dst, void* stream);

/* -- normalised float tensor clips ---------------------------------------------------------------
 * AGMV_TENSORFMT of include/agmv.h ("normalised float tensors"), which holds the definitions: `type` is 1 F32, 2 F16 (IEEE
 * binary16) or 3 BF16, by value; a tensor clip is n frames of [3][h][w] elements, planes R, G, B, aligned to its element.
 * agmv_hip_tensor_frame_bytes:  3 * (4, 2, 2) * n_pixels; 0 for an unknown type.  Host only: needs no context and no GPU.
 * agmv_hip_tensor_table:        the writing rule as a table: table[256 * c + v] = the bit pattern, in `type`, of the float32
 *                               nearest to the double ((double)v / 255.0 - (double)mean[c]) / (double)std[c], rounded to
 *                               nearest-even into F16 / BF16 (overflow is an infinity) by integer code.  768 elements of the
 *                               type in host memory.  Host only.  Returns non-zero for an unknown type, a NULL pointer or a
 *                               normalisation outside the bounds of include/agmv.h (NaN and infinities are outside).
 * agmv_hip_tensor_from_xrgb_async (the decoder's sink): d_src holds n_frames packed XRGB32 frames of src_w x src_h (bits >= 24
 *   ignored, 4-byte aligned); target frame k, 3 * dst_w * dst_h elements, receives out[c][Y][X] = table[256 * c + channel c of
 *   D(X, Y)], where D is the source (`filter` 0: the sizes are equal) or the clip agmv_hip_scale_frames_async defines for `filter`
 *   1 (nearest) or 3 (bilinear); 2 is refused: the box filter is agmv_hip_scale_area_dev's.  d_table is agmv_hip_tensor_table's
 *   768 elements in device memory; the kernel keeps them in LDS and only looks them up, so the elements are the table's bit
 *   patterns whatever they are.  One launch, asynchronous on `stream`: no allocation, no host synchronisation, nothing of the
 *   context is used but its device, no XRGB32 copy of the scaled clip exists.  Where dst_w % 16 == 0 and every plane starts on
 *   a 16-byte boundary a lane forms 16 target pixels of a row and stores them per plane with 16-byte stores; any other target
 *   is written element by element, to the same bytes.  Nothing outside the n_frames target frames is written.
 * agmv_hip_tensor_to_xrgb_async (the encoder's source): d_src holds n_frames tensor frames of frame_pixels pixels; d_dst
 *   receives frame_pixels words 0x00RRGGBB per frame by the reading rule of include/agmv.h: an element x, converted exactly to
 *   float32, gives t = fl32(fl32(x * a[c]) + b[c]) -- two separately rounded operations, never fused -- and the byte 0 for a
 *   NaN, else (int)rintf(fminf(fmaxf(t, 0), 255)), rounding half to even.  `ab` is host memory, a[3] then b[3], read before
 *   the call returns.  One launch, asynchronous on `stream`, 16-byte loads and stores where every plane and every target
 *   frame starts on a 16-byte boundary, element by element otherwise, with the same result.
 * The two asynchronous calls: n_frames == 0 is success and launches nothing; a NULL pointer, an unknown type or filter, a zero
 * or oversize shape (more than 2^28 pixels) or a pointer that is not aligned to its element returns non-zero with a message and
 * launches nothing. */
size_t agmv_hip_tensor_frame_bytes(int type, size_t n_pixels);
int agmv_hip_tensor_table(int type, const float* mean /* [3] */, const float* std /* [3] */, void* table /* host, 768 elements */);
int agmv_hip_tensor_from_xrgb_async(agmv_hip_ctx* ctx, int type, const uint32_t* d_src, uint32_t src_w, uint32_t src_h,
                                    uint32_t n_frames, int filter, uint32_t dst_w, uint32_t dst_h, const void* d_table, void* d_dst,
                                    void* stream);
int agmv_hip_tensor_to_xrgb_async(agmv_hip_ctx* ctx, int type, const void* d_src, size_t frame_pixels, uint32_t n_frames,
                                  const float* ab /* host: a[3] then b[3] */, uint32_t* d_dst, void* stream);

/* -- the palette refined by weighted k-means ------------------------------------------------------
 * The refinement of include/agmv.h ("palette refinement"), which holds the definition: Lloyd's algorithm over the points of a
 * histogram, in exact integers.
 *   d_hist      2^19 bins as the agmv_hip_histogram*_dev functions fill them; not modified.  Only the bins of the quality's codes
 *               are read (2^19 HIGH, 2^17 MID, 2^16 LOW).
 *   d_pal       k colours 0x00RRGGBB, in and out; the first n_free move, the others are pinned.  Bits >= 24 are ignored, and
 *               cleared in a centroid that moves.
 *   iterations  rounds at most (<= 4096); 0 only measures.
 *   d_rounds    one word: the rounds that changed at least one centroid.
 *   d_sse       two words: the distortion of the centroids given and of the centroids returned.
 * 1 <= k <= 512, n_free <= k, quality 1 .. 3: anything else returns non-zero with a message, touches no memory and launches
 * nothing.  Asynchronous on `stream`: 2 * (iterations + 1) small launches and no host synchronisation; after the round that
 * changes nothing a device flag makes the remaining launches return at once.  The sums of a pass live in a work area of the
 * context (16 KB): calls on one context must not overlap.  Exact and repeatable: the same outputs from run to run. */
int agmv_hip_palette_refine_dev(agmv_hip_ctx* ctx, const uint32_t* d_hist, int quality, uint32_t* d_pal, uint32_t k, uint32_t n_free,
                                uint32_t iterations, uint32_t* d_rounds, uint64_t* d_sse, void* stream);

/* -- audio tracks -----------------------------------------------------------------------------------
 * The audio codec of include/agmv.h ("audio tracks"), which holds the definitions: a 16-bit track stores one code byte per
 * sample (compand), an 8-bit track its bytes.  `pcmfmt` is an AGMV_PCMFMT, by value:
 *   1 S16   [samples_per_channel][channels] 16-bit words, the track's own bit patterns; 2-byte aligned
 *   2 U8    [samples_per_channel][channels] bytes; both directions are a copy
 *   3 F32P  [channels][samples_per_channel] float, 1 .. 8 channels; 4-byte aligned.  In: clamp to [-1, 1], x 32767, round half to
 *           even, NaN = 0, the int16's bit pattern.  Out: the int16 / 32768.
 * d_codes holds samples_per_channel * channels bytes in track order (interleaved), 1-byte aligned.
 * agmv_hip_audio_compand_async: d_pcm -> d_codes.   agmv_hip_audio_expand_async: d_codes -> d_pcm.
 * Asynchronous on `stream`: one launch (U8: one device-to-device copy), no allocation, no host synchronisation, nothing of the
 * context is used but its device.  Nothing outside the samples_per_channel * channels elements of the destination is written.
 * The body runs on 16-byte loads and stores where the two pointers can be brought to 16-byte boundaries together (for F32P
 * also samples_per_channel % 4 == 0, so that every plane can); otherwise sample by sample, with the same result.
 * Returns non-zero with a message and launches nothing for a NULL pointer, an unknown format, zero channels, more than 8 planar
 * channels or a PCM pointer that is not aligned to its sample.  samples_per_channel == 0 is success and launches nothing. */
int agmv_hip_audio_compand_async(agmv_hip_ctx* ctx, int pcmfmt, const void* d_pcm, uint32_t channels, uint64_t samples_per_channel,
                                 uint8_t* d_codes, void* stream);
int agmv_hip_audio_expand_async(agmv_hip_ctx* ctx, int pcmfmt, const uint8_t* d_codes, uint32_t channels, uint64_t samples_per_channel,
                                void* d_pcm, void* stream);

/* -- a decoded clip measured against its reference ---------------------------------------------------
 * AGMV_FRAME_QUALITY of include/agmv.h ("measuring a decoded clip"), which holds the definition: per frame and channel the exact
 * squared error, the squared error of the 4x4 block sums, the largest error and the sum of the integer SSIM (Q20) of the 8x8
 * windows at stride 4.  d_test holds n_frames packed frames of w x h (bits >= 24 ignored, 4-byte aligned), d_ref the same frames
 * in the layout `ref_fmt`: any of the seven above (1 .. 5, or 16 / 17 OR-ed with the YUV flags), at that layout's frame stride and
 * alignment; a YUV reference is compared as the clip agmv_hip_yuv_to_xrgb_dev makes of it.  w and h are multiples of 4, w * h
 * <= 2^28.  d_quality (8-byte aligned) receives n_frames entries of 96 bytes: 12 64-bit words sse[3], block_sse[3], max_err[3],
 * ssim[3] (signed), channel 0 = R.  The call clears them itself on `stream`: what they held before does not matter.
 * Asynchronous on `stream`: one memset and one launch, no allocation, no host synchronisation, nothing of the context is used
 * but its device.  Each clip is read once (the one block row and column two tiles share, twice), the test clip and a reference
 * whose frames start on 16-byte boundaries with 16-byte loads; no converted copy of the reference exists.  Exact and repeatable:
 * integer sums, the same words from run to run.  Any n_frames; n_frames == 0 is success and touches nothing.  Returns non-zero
 * with a message and launches nothing for an unknown format, a zero size, a size that is no multiple of 4 or a NULL pointer. */
int agmv_hip_measure_frames_async(agmv_hip_ctx* ctx, const uint32_t* d_test, int ref_fmt, const void* d_ref,
                                  uint32_t w, uint32_t h, uint32_t n_frames, void* d_quality /* n_frames * 96 bytes */, void* stream);

/* optional timing: when enabled the library records HIP events on the caller's stream around its three kernel
   groups; agmv_hip_last_kernel_ms(which) returns the last launch's duration in ms (0 = k_encode, 1 = the parser
   kernels, 2 = k_decode + k_fixup, 3 = the whole of agmv_hip_parse_decode_frames_dev / agmv_hip_decode_bitstreams_dev), or a negative value if
   unavailable.  An agmv_hip_decode_bitstreams_dev call cut into ranges runs groups 1 and 2 once per range: 1 and 2 are then the
   sums over the ranges of that call (disjoint intervals inside 3) */
int   agmv_hip_enable_timing(agmv_hip_ctx* ctx, int on);
float agmv_hip_last_kernel_ms(agmv_hip_ctx* ctx, int which);

/* check for an asynchronous device-side failure (look-back timeout) after synchronising */
int agmv_hip_check(agmv_hip_ctx* ctx, void* stream);

/* streams, pinned host staging and asynchronous copies for C hosts that do not link the HIP runtime themselves (the
   pipelined sequence drivers: H2D || kernels || D2H || host LZ).  The *_on / *_async forms act on the context's device;
   kind: 0 = host to device, 1 = device to host, 2 = device to device.  Host memory of asynchronous copies must come from
   agmv_hip_host_alloc. */
void* agmv_hip_stream_create(agmv_hip_ctx* ctx);
void  agmv_hip_stream_destroy(agmv_hip_ctx* ctx, void* stream);
int   agmv_hip_stream_sync(agmv_hip_ctx* ctx, void* stream);
/* events order work across streams without a host synchronisation: agmv_hip_stream_wait_event makes later work on `stream`
   wait for the work before agmv_hip_event_record on the other stream (the sequence decoder hands its LZ stage's rows over so) */
void* agmv_hip_event_create(agmv_hip_ctx* ctx);
void  agmv_hip_event_destroy(agmv_hip_ctx* ctx, void* ev);
int   agmv_hip_event_record(agmv_hip_ctx* ctx, void* ev, void* stream);
int   agmv_hip_stream_wait_event(agmv_hip_ctx* ctx, void* stream, void* ev);
void* agmv_hip_host_alloc(size_t bytes);
void  agmv_hip_host_free(void* h);
void* agmv_hip_malloc_on(agmv_hip_ctx* ctx, size_t bytes);
void  agmv_hip_free_on(agmv_hip_ctx* ctx, void* d);
int   agmv_hip_memcpy_async(agmv_hip_ctx* ctx, void* dst, const void* src, size_t n, int kind, void* stream);
int   agmv_hip_memset_async(agmv_hip_ctx* ctx, void* d, int v, size_t n, void* stream);
int   agmv_hip_ctx_device(agmv_hip_ctx* ctx);

/* raw device memory for C hosts that do not link the HIP runtime themselves (current device) */
void* agmv_hip_malloc(size_t bytes);
void  agmv_hip_free(void* d);
int   agmv_hip_memcpy_h2d(void* d, const void* h, size_t bytes);
int   agmv_hip_memcpy_d2h(void* h, const void* d, size_t bytes);
int   agmv_hip_memset(void* d, int value, size_t bytes);
int   agmv_hip_sync(void);

#ifdef __cplusplus
}
#endif
#endif
