/*
 * dirt_hip.h -- C ABI of libdirt_hip.so, the MI355X (gfx950) replacement for the two TensorFlow
 * custom ops of pmh47/dirt.  Plain C, raw device pointers and sizes; no torch / TF / HIP types.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository root).  The reference binds its ops through the TF op registry
 * (dirt/rasterise_ops.py:5-10: tf.load_op_library('librasterise.so')); a maintainer binds this
 * library with ctypes -- see INTEGRATION.md for the stub.
 *
 * Conventions shared by every call
 *   - all tensors are dense, row-major, float32 except `faces` (int32); device pointers, 16-byte
 *     aligned (torch / hipMalloc allocations are);
 *   - background / pixels / grad_* images are [B,H,W,C], top row first (README.md:183);
 *     vertices [B,V,4] are OpenGL clip-space (x,y,z,w); vertex_colors [B,V,C]; faces [B,F,3];
 *   - `workspace` is caller-owned device scratch of at least dirt_workspace_bytes(...) bytes,
 *     16-byte aligned; the library keeps no DEVICE state between calls.  Calls on different workspaces are independent
 *     (any threads, any streams).  ONE workspace is a single-stream object: the calls that share it -- a forward with
 *     DIRT_FLAG_KEEP_STATE and the backward calls with DIRT_FLAG_REUSE_STATE that consume it -- must be enqueued on one
 *     stream (or be ordered by the caller's own events): nothing in the library serialises two streams on one workspace;
 *   - the one piece of HOST state: per workspace address, which gradient buffers the last forward left cleared (see
 *     DIRT_FLAG_OUTPUTS_CLEARED / DIRT_FLAG_DENSE_FROM_STATE).  It is consulted at ENQUEUE time and knows pointers, not
 *     contents -- so the "skip the clearing launch" paths additionally require that (i) forward and backward are captured
 *     TOGETHER when a HIP graph is recorded (a backward captured alone replays without its forward's clear and would
 *     accumulate), (ii) the cleared tensors stay allocated between the two calls (a caching allocator handing the same
 *     addresses to other tensors in between is indistinguishable), and (iii) nothing writes to them in between.  The
 *     Python wrapper keeps the tensors on the state object, which guarantees (ii) and (iii); a caller that cannot, omits
 *     the flags and pays one clearing launch.  Any call that rebuilds a workspace (a forward, a stateless backward,
 *     dirt_rasterise_visibility) forgets what was cleared in it;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); work is enqueued
 *     asynchronously on it and the call returns without synchronising;
 *   - the current HIP device must be the one that owns the pointers;
 *   - return value 0 = success, <0 = DIRT_E_* below; dirt_last_error() describes the last
 *     failure on the calling thread.  The library never aborts the process.
 */
#ifndef DIRT_HIP_H
#define DIRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIRT_ABI_VERSION 4

/* error codes */
#define DIRT_OK 0
#define DIRT_E_INVALID_ARGUMENT (-1) /* bad sizes / null pointers: the OP_REQUIRES checks of
                                        csrc/rasterise_egl.cpp:301-316, csrc/rasterise_grad_egl.cpp:349-377
                                        and the CHECKs of csrc/hwc.h:27-28 */
#define DIRT_E_TOO_MANY_VERTICES (-2) /* V > 2^24: csrc/rasterise_grad_egl.cpp:399-405 */
#define DIRT_E_WORKSPACE (-3)         /* workspace NULL / too small / misaligned */
#define DIRT_E_HIP (-4)               /* a HIP runtime call failed (the reference LOG(FATAL)s) */

/* flags (bitwise or) */
#define DIRT_FLAG_Q1_INTENDED 1u /* backward: for 1-channel groups take the Scharr L1 over the one
                                    real channel instead of reproducing the reference's out-of-range
                                    channel reads (csrc/rasterise_grad_egl.cu:119-123,185; SURVEY.md
                                    App. A.3 quirk Q1).  Default (0) reproduces the reference. */

#define DIRT_FLAG_KEEP_STATE 2u  /* forward: also leave, in `workspace`, the state the backward pass needs
                                    (per-face set-up records and the per-pixel front-most face). */
#define DIRT_FLAG_REUSE_STATE 4u /* backward: `workspace` is the very buffer a forward call with
                                    DIRT_FLAG_KEEP_STATE filled for the same vertices, faces and sizes, and
                                    nothing has written to it since: skip triangle set-up and the visibility
                                    render.  The reference re-renders in RasteriseGrad and notes the
                                    alternative itself (csrc/rasterise_grad_egl.cpp:446-447: "It may or may
                                    not more efficient to render these in the forward pass and return them
                                    in separate outputs").  The state is caller-owned memory; the library
                                    stays stateless.  Results are identical with or without the flag. */
#define DIRT_FLAG_DENSE_FROM_STATE 8u /* backward, with DIRT_FLAG_REUSE_STATE and dense caller tensors for grad_vertices /
                                    grad_vertex_colors: sum the vertex gradients in the accumulators the forward pass
                                    cleared inside the state (one interleaved row per vertex: what the float atomics are
                                    fastest on) and copy them out into the caller's dense [B,V,4] / [B,V,C] tensors with one
                                    more launch -- what csrc/rasterise_grad_egl.cpp:381-391 allocates as the op's outputs.
                                    Re-entrant since ABI 3: the library knows (host-side, per workspace address) whether the
                                    accumulators are still as the forward left them and clears them itself when they are
                                    not, so a second backward call over one forward returns that call's gradients, not the
                                    sum of both.  Results agree to summation order. */
#define DIRT_FLAG_OUTPUTS_CLEARED 0x10u /* backward, with DIRT_FLAG_REUSE_STATE: grad_vertices / grad_vertex_colors are the
                                    very tensors dirt_rasterise_forward_train was given with this workspace, and nothing
                                    has written to them since: skip the launch that clears them (the reference's
                                    cudaMemsetAsync, csrc/rasterise_grad_egl.cu:244-250, happened inside the forward's
                                    launch).  Checked against the library's host-side record of that forward: if the
                                    record does not name these pointers, or a backward call has consumed it already, the
                                    outputs are cleared as without the flag -- never added onto. */

#define DIRT_FLAG_TILES_LARGE 0x200u /* pin the forward / visibility kernels' tile shape instead of letting the library
                                       choose it from the frame size and the face density: 32x32 pixel tiles ... */
#define DIRT_FLAG_TILES_SMALL 0x400u /* ... or 16x16.  Results do not depend on the shape (pixels and visibility bit for
                                       bit); for tests.  (The gradient kernel's shapes: DIRT_FLAG_GRAD_*.)  BOTH bits:
                                       32x32 tiles rendered by EIGHT half-size waves each, the shape the library takes by
                                       itself for launches of at most 2048 such tiles (DIRT_FLAG_TILES_LARGE alone pins four
                                       waves per tile); where that shape does not exist -- meshes of more than 16 384 faces,
                                       channel counts other than 1, 3, 4, the visibility pass -- the pair means 32x32. */
#define DIRT_FLAG_GRAD_ROWS 0x1000u  /* pin the gradient kernel's face-loop shape instead of letting the library choose by
                                        frame size: every 8x8 block of a wave walks its own faces ... */
#define DIRT_FLAG_GRAD_PAIRS 0x2000u /* ... or pairs of blocks share a face (fewer float atomics).  Results agree to
                                        summation order (how the parity tests cover both) */
#define DIRT_FLAG_GRAD_SMALL 0x4000u /* ... or the small-frame gradient kernel: one pixel per lane on 16x16 tiles
                                        (channel counts 1, 3, 4; chosen by the library when tiles x scenes of the call --
                                        32x32 tiles -- are at most 256 and the mesh has at least 96 faces per tile, counted
                                        over ALL faces of a scene, culled and off-screen ones included).  Same results to
                                        summation order */
#define DIRT_FLAG_GRAD_PX2 0x8000u   /* ... or the two-pixels-per-lane gradient kernel on 32x16 tiles (channel counts 1, 3, 4:
                                        twice the waves at half the instruction chain each; chosen by the library for frames
                                        of more than 256 and fewer than 1024 32x32 tiles -- 3 channels: of more than 256 --
                                        where it measured faster).  Same results to summation order */
#define DIRT_FLAG_GRAD_PX4 0x10000u  /* ... or the four-pixels-per-lane kernel (rows or pairs by the library's own rule) where
                                        the library would choose the two-pixels-per-lane one */
#define DIRT_FLAG_GRAD_STREAM 0x20000u /* reserved: accepted and ignored.  It pinned an experimental streaming gradient
                                        kernel that was never the library's own choice (it measured slower,
                                        profiles/EXPERIMENTS.md round 6) and has been removed; a call that sets it gets the
                                        library's own kernel choice, the same results to summation order */
#define DIRT_FLAG_SHARED_FACES 0x800u /* `faces` is one [F,3] topology shared by all B scenes instead of [B,F,3] (the
                                        TODO of csrc/rasterise_egl.cpp:314).  Same flag on the
                                        forward, visibility and backward calls of one scene batch. */
#define DIRT_FLAG_PROFILE 0x100u /* record a HIP-event pair around every kernel this call launches (on the
                                    call's stream); read the totals with dirt_profile_read.  Replaces the
                                    reference's compile-time TIME_SECTIONS wall-clock prints
                                    (csrc/rasterise_egl.cpp:398-405, csrc/rasterise_grad_egl.cpp:479-483). */

/* Limits of this implementation (the reference's limit is the GL max texture size of its atlas). */
#define DIRT_MAX_DIM 16384

/* Returns DIRT_ABI_VERSION of the loaded library. */
int dirt_abi_version(void);

/* Thread-local description of the last error returned on this thread ("" if none). */
const char *dirt_last_error(void);

/*
 * Scratch bytes needed by dirt_rasterise_forward / dirt_rasterise_backward for these sizes
 * (replaces the grow-only GL buffers / framebuffer atlas the reference caches per thread,
 * csrc/rasterise_egl.cpp:325-346, csrc/rasterise_grad_egl.cpp:407-425).  Returns 0 on invalid sizes.
 */
size_t dirt_workspace_bytes(int B, int V, int F, int H, int W, int C);

/*
 * Forward.  Replaces the `Rasterise` op: REGISTER_OP csrc/rasterise_egl.cpp:32-51 and
 * RasteriseOpGpu::Compute csrc/rasterise_egl.cpp:276-407, as called from
 * dirt/rasterise_ops.py:81-85,98-105.  Unlike the reference op, C may be any value >= 1: the
 * result equals the reference's channel-grouped evaluation (dirt/rasterise_ops.py:86-108).
 *   in : background [B,H,W,C], vertices [B,V,4], vertex_colors [B,V,C], faces [B,F,3]
 *   out: pixels [B,H,W,C]
 * B, V or F may be 0 (pixels = background when there is nothing to draw).
 */
int dirt_rasterise_forward(const float *background, const float *vertices, const float *vertex_colors,
                           const int32_t *faces, float *pixels, int B, int V, int F, int H, int W, int C,
                           void *workspace, size_t workspace_bytes, unsigned flags, void *stream);

/*
 * Forward of a training step: dirt_rasterise_forward with DIRT_FLAG_KEEP_STATE that, in the same launch, also clears the
 * DENSE gradient tensors the backward call will be given -- the RasteriseGrad op's outputs grad_vertices [B,V,4] and
 * grad_vertex_colors [B,V,C] (csrc/rasterise_grad_egl.cpp:381-391), which the reference clears with cudaMemsetAsync at the
 * start of its gradient op (csrc/rasterise_grad_egl.cu:244-250).  A following dirt_rasterise_backward with
 * DIRT_FLAG_REUSE_STATE | DIRT_FLAG_OUTPUTS_CLEARED on the same workspace and the same two tensors then is ONE launch that
 * adds straight into the op's contract outputs: no clearing launch, no copy out of the state.  (The state's own
 * interleaved accumulators are NOT cleared by this call.)
 */
int dirt_rasterise_forward_train(const float *background, const float *vertices, const float *vertex_colors,
                                 const int32_t *faces, float *pixels, float *grad_vertices, float *grad_vertex_colors,
                                 int B, int V, int F, int H, int W, int C, void *workspace, size_t workspace_bytes,
                                 unsigned flags, void *stream);

/*
 * Backward.  Replaces the `RasteriseGrad` op: REGISTER_OP csrc/rasterise_grad_egl.cpp:33-53,
 * Compute csrc/rasterise_grad_egl.cpp:324-485 and launch_grad_assembly / assemble_grads
 * csrc/rasterise_grad_egl.cu:93-278, as called from dirt/rasterise_ops.py:113-118,154-160; for C
 * not in {1,3} it reproduces _rasterise_grad_multichannel (dirt/rasterise_ops.py:132-177):
 * channel groups of 3 then 1s, grad_vertices summed over groups, the others concatenated.
 *   in : vertices [B,V,4], faces [B,F,3], pixels [B,H,W,C] (the forward output), grad_pixels [B,H,W,C]
 *   out: grad_background [B,H,W,C], grad_vertices [B,V,4], grad_vertex_colors [B,V,C],
 *        debug_thingy [B,H,W,3] or NULL (the reference's 4th, diagnostic output, of the first
 *        channel group; csrc/rasterise_grad_egl.cu:150-151,172)
 * All outputs are fully written (zero where the reference's memsets leave zero,
 * csrc/rasterise_grad_egl.cu:244-250).  Float atomics make grad_vertices / grad_vertex_colors
 * order-dependent in the last bits, as in the reference.
 */
int dirt_rasterise_backward(const float *vertices, const int32_t *faces, const float *pixels,
                            const float *grad_pixels, float *grad_background, float *grad_vertices,
                            float *grad_vertex_colors, float *debug_thingy, int B, int V, int F, int H, int W,
                            int C, void *workspace, size_t workspace_bytes, unsigned flags, void *stream);

/*
 * Visibility only (no reference counterpart as an op; it is the render pass of
 * csrc/rasterise_grad_egl.cpp:432-456 exposed for tests and for the deferred-shading row):
 *   out: face_id [B,H,W] int32, index of the front-most face or -1.
 */
int dirt_rasterise_visibility(const float *vertices, const int32_t *faces, int32_t *face_id, int B, int V,
                              int F, int H, int W, void *workspace, size_t workspace_bytes, unsigned flags,
                              void *stream);

/*
 * With DIRT_FLAG_KEEP_STATE the forward pass also clears the gradient accumulators inside the workspace.  This
 * returns their addresses and ROW STRIDES (in floats): a backward call with DIRT_FLAG_REUSE_STATE whose grad_vertices /
 * grad_vertex_colors ARE these pointers accumulates straight into them and needs no clearing launch (the reference
 * clears its outputs with four cudaMemsetAsync, csrc/rasterise_grad_egl.cu:244-250).  Any other output pointers work
 * too; they are dense ([B,V,4] and [B,V,C]) and are cleared first.
 *   The two accumulators are INTERLEAVED: one row of S = 4 + C (rounded up to a multiple of 4) floats per vertex,
 * {x, y, z, w, c0 .. cC-1}, so both strides are S and *grad_vertex_colors == *grad_vertices + 4: a face adds all of a
 * vertex's values to one row, which is what the memory system's float atomics are priced by (tools/atomic_bench.hip).
 * View them as strided tensors ([B,V,4] with strides (S V, S, 1) ...).  The layout depends on C: use the state's
 * accumulators only with the channel count of the forward call that cleared them.
 */
int dirt_state_grad_buffers(void *workspace, size_t workspace_bytes, int B, int V, int F, int H, int W, int C,
                            float **grad_vertices, float **grad_vertex_colors, int *grad_vertices_row_stride,
                            int *grad_vertex_colors_row_stride);

/*
 * Texture look-up of a deferred shader, fused.  Replaces the TensorFlow composition
 * `sample_texture(texture, uvs_to_pixel_indices(uvs, shape, mode), filter)` of the reference's samples/textured.py:16-61
 * as used by its shader_fn (samples/textured.py:116-141): (u, v) with (0, 0) at the TOP-LEFT of the image -> repeat
 * (uvs % 1) or clamp -> scaled by the texture size -> bilinear blend of the four neighbours (fraction of the index, no
 * half-texel shift) or nearest.  Float32, the reference's operation order; where its gather would read row Ht / column Wt
 * the last texel is used.
 *   texture [Ht,Wt,Ct]; uvs: n pairs (u, v) `uv_stride` >= 2 floats apart -- read in place from a G-buffer [H,W,C] with
 *   uv_stride = C and the pointer at the u channel; out [n,Ct].
 * Backward: grad_out [n,Ct] -> grad_texture [Ht,Wt,Ct] (cleared by the call -- by a kernel on `stream`, so the call can be
 * captured in a graph -- then accumulated with float atomics) and grad_uvs (n pairs `grad_uv_stride` >= 2 apart, only those
 * two floats of each pair written; may be NULL, and grad_uv_stride is then ignored).  Float32 denormals are kept, in the
 * look-up and in both gradients.  n == 0 is not an error: nothing is read, every pointer may be NULL, and a grad_texture
 * that is given is still cleared.  Arguments are checked before any device work; a pixel grid with more than 2^31 - 1 rows,
 * columns or tiles is refused with DIRT_E_HIP after the clear.
 * dirt_texture_last_error(): thread-local description of the last failure of these calls (and of the trilinear ones below).
 */
#define DIRT_TEX_CLAMP 1u   /* mode 'clamp' instead of 'repeat' (samples/textured.py:21-24) */
#define DIRT_TEX_NEAREST 2u /* mode 'nearest' instead of 'bilinear' (samples/textured.py:31-33) */
int dirt_texture_sample_forward(const float *texture, const float *uvs, float *out, long long n, int Ht, int Wt, int Ct,
                                int uv_stride, unsigned flags, void *stream);
int dirt_texture_sample_backward(const float *texture, const float *uvs, const float *grad_out, float *grad_texture,
                                 float *grad_uvs, long long n, int Ht, int Wt, int Ct, int uv_stride, int grad_uv_stride,
                                 unsigned flags, void *stream);
/* The same gradient for look-ups that form an IMAGE -- rows x cols pixels, row-major, n = rows * cols pairs (a G-buffer slice
 * [H, W, 2]; batches stack their rows): the kernel then works on 16 x 16-pixel tiles, sums a tile's contributions in an LDS copy
 * of the texture patch they fall into and sends every texel of the patch to memory once -- instead of 4 Ct float atomics
 * per pixel (what `gather_nd`'s gradient in the reference and dirt_texture_sample_backward's flat runs of 256 amount to where
 * neighbouring pixels share texels).  Same results to summation order. */
int dirt_texture_sample_backward_image(const float *texture, const float *uvs, const float *grad_out, float *grad_texture,
                                       float *grad_uvs, long long rows, long long cols, int Ht, int Wt, int Ct, int uv_stride,
                                       int grad_uv_stride, unsigned flags, void *stream);
const char *dirt_texture_last_error(void);
/* A TEXTURE PER SCENE (extends samples/textured.py:16-61, whose shader_fn has one texture for the whole batch): `scenes`
 * look-ups of the two calls above in one launch each.  textures [scenes,Ht,Wt,Ct]; scene b's n (rows x cols) look-ups read
 * textures[b]: its pairs start b * n * uv_stride floats after scene 0's (a slice of a contiguous G-buffer [scenes,H,W,C] is
 * read in place with uv_stride = C), its out / grad_out b * n * Ct, its grad_uvs b * n * grad_uv_stride, its grad_textures
 * b * Ht * Wt * Ct.  rows and cols are PER SCENE (a flat list: rows = 1): a 16 x 16 tile, or a 256 x 1 run, of the backward
 * holds look-ups of one scene only.  grad_textures is cleared by the call (a kernel on `stream`) and fully written.  The
 * checks of the single-texture calls, then: scenes >= 0, scenes x every per-scene extent fits 63 bits, scenes <= 65535 (one
 * launch addresses no more; refused, not truncated), and a pixel grid with more than 2^31 - 1 rows, columns or tiles -- all
 * DIRT_E_INVALID_ARGUMENT before any device work.  scenes == 0 launches nothing. */
int dirt_texture_sample_batch_forward(const float *textures, const float *uvs, float *out, long long scenes, long long n, int Ht,
                                      int Wt, int Ct, int uv_stride, unsigned flags, void *stream);
int dirt_texture_sample_batch_backward_image(const float *textures, const float *uvs, const float *grad_out, float *grad_textures,
                                             float *grad_uvs, long long scenes, long long rows, long long cols, int Ht, int Wt,
                                             int Ct, int uv_stride, int grad_uv_stride, unsigned flags, void *stream);

/*
 * Trilinear (mipmapped) texture look-up.  Extends the bilinear look-up above (samples/textured.py:16-61) with a mip
 * pyramid and a level of detail (LOD) from the screen-space footprint of (u, v); specification in
 * dirt_amd/csrc/dirt_texture_mip.hip and DESIGN.md §7.  The pyramid is one packed buffer: level k [max(Ht >> k, 1),
 * max(Wt >> k, 1), Ct] after level k - 1, level 0 a copy of the texture.  All calls return 0 or DIRT_E_*; failures are
 * described by dirt_texture_last_error().  The library keeps no device state: pyramids and scratch belong to the caller.
 *
 * dirt_texture_mip_levels: the level count of an Ht x Wt texture (levels halve while each dimension is even or 1, up to
 * `max_level`, < 0: no limit; samples/textured.py:16-61 has one level) as the return value (>= 1), and the packed
 * pyramid's size in floats in *pyramid_floats (may be NULL).
 */
int dirt_texture_mip_levels(int Ht, int Wt, int Ct, int max_level, long long *pyramid_floats);
/* The pyramid of `texture` [Ht,Wt,Ct] (the texture of samples/textured.py:16-61) into `pyramid` (pyramid_floats floats):
 * 2 x 2 (or 2 x 1) means in float32; one launch for levels 0-5, one more for any above. */
int dirt_texture_mip_build(const float *texture, float *pyramid, int Ht, int Wt, int Ct, int levels, void *stream);
/* The gradient of dirt_texture_mip_build (samples/textured.py:16-61's texture gradient through the pyramid):
 * grad_pyramid (packed) -> grad_texture [Ht,Wt,Ct], fully written, in one launch. */
int dirt_texture_mip_collapse(const float *grad_pyramid, float *grad_texture, int Ht, int Wt, int Ct, int levels, void *stream);
/* The trilinear look-up (extends samples/textured.py:16-61): rows x cols look-ups, row-major, stacked images of
 * `image_rows` rows each (a flat list: rows = image_rows = 1); (u, v) pairs `uv_stride` floats apart, read in place.
 * `lod` (rows x cols floats) gives lambda = lod + lod_bias; NULL takes lambda from the footprint of neighbouring look-ups
 * of the same image, skipping pixels whose `mask` (rows x cols, `mask_stride` floats apart; NULL: all valid) is 0.
 * flags: DIRT_TEX_CLAMP. */
int dirt_texture_sample_mip_forward(const float *pyramid, const float *uvs, const float *lod, const float *mask, float *out,
                                    long long rows, long long cols, int image_rows, int Ht, int Wt, int Ct, int levels,
                                    int uv_stride, int mask_stride, float lod_bias, unsigned flags, void *stream);
/* Its gradient (extends samples/textured.py:16-61's): grad_out [rows*cols,Ct] -> grad_texture [Ht,Wt,Ct] (fully written),
 * grad_uvs (pairs `grad_uv_stride` apart; may be NULL) and grad_lod (rows*cols; may be NULL, needs `lod`).
 * `grad_pyramid` is caller-owned scratch of pyramid_floats floats (cleared by the call); lambda is held constant. */
int dirt_texture_sample_mip_backward(const float *pyramid, const float *uvs, const float *lod, const float *mask,
                                     const float *grad_out, float *grad_pyramid, float *grad_texture, float *grad_uvs,
                                     float *grad_lod, long long rows, long long cols, int image_rows, int Ht, int Wt, int Ct,
                                     int levels, int uv_stride, int grad_uv_stride, int mask_stride, float lod_bias,
                                     unsigned flags, void *stream);
/* A TEXTURE PER SCENE for the four calls above (extends samples/textured.py:16-61 as dirt_texture_sample_batch_forward does;
 * the same layout rule and the same three extra checks).  pyramids / grad_pyramids [scenes, pyramid_floats]: scene b's packed
 * pyramid after scene b - 1's, each laid out as dirt_texture_mip_levels says.  The build is one launch for levels 0-5 of every
 * scene and one more, a workgroup per scene, for any above; the collapse is one launch. */
int dirt_texture_mip_build_batch(const float *textures, float *pyramids, long long scenes, int Ht, int Wt, int Ct, int levels,
                                 void *stream);
int dirt_texture_mip_collapse_batch(const float *grad_pyramids, float *grad_textures, long long scenes, int Ht, int Wt, int Ct,
                                    int levels, void *stream);
/* The trilinear look-up of `scenes` textures (extends samples/textured.py:16-61): rows x cols look-ups PER SCENE, stacked
 * images of `image_rows` rows each (image_rows divides rows; a flat list: rows = image_rows = 1); scene b's pairs, lod, mask,
 * out and gradients start b per-scene extents after scene 0's (lod and grad_lod b * rows * cols, mask b * rows * cols *
 * mask_stride).  The footprint never looks across images or scenes. */
int dirt_texture_sample_mip_batch_forward(const float *pyramids, const float *uvs, const float *lod, const float *mask, float *out,
                                          long long scenes, long long rows, long long cols, int image_rows, int Ht, int Wt, int Ct,
                                          int levels, int uv_stride, int mask_stride, float lod_bias, unsigned flags, void *stream);
/* Its gradient (extends samples/textured.py:16-61's): one clear of grad_pyramids (caller-owned scratch, [scenes,
 * pyramid_floats]), one launch over every scene's tiles, one collapse into grad_textures [scenes,Ht,Wt,Ct] (fully written). */
int dirt_texture_sample_mip_batch_backward(const float *pyramids, const float *uvs, const float *lod, const float *mask,
                                           const float *grad_out, float *grad_pyramids, float *grad_textures, float *grad_uvs,
                                           float *grad_lod, long long scenes, long long rows, long long cols, int image_rows, int Ht,
                                           int Wt, int Ct, int levels, int uv_stride, int grad_uv_stride, int mask_stride,
                                           float lod_bias, unsigned flags, void *stream);
/* CUBE-MAP look-up: a texture indexed by a direction (an environment map).  These two replace no reference interface -- the
 * reference's samples/textured.py:16-61 has flat textures only; specification in dirt_amd/csrc/dirt_texture_cube.hip and
 * DESIGN.md §7.  `pyramid` [6, floats]: the packed pyramid of each `size` x `size` x `channels` face, faces in the order +X, -X,
 * +Y, -Y, +Z, -Z, as dirt_texture_mip_build_batch makes it of the cube [6, size, size, channels] with scenes = 6 and `floats` as
 * dirt_texture_mip_levels(size, size, channels, ...) says; with levels = 1 it is the cube itself.  directions: n triples
 * (x, y, z) `dir_stride` >= 3 floats apart, read in place (4-byte alignment suffices), not normalised; one that is not finite
 * or all zero gives 0 in every channel and adds to no gradient.  lod [n]: the look-up is trilinear, lambda = lod + lod_bias;
 * NULL: level 0 only, bilinear, or its nearest texel with DIRT_TEX_NEAREST -- the only flag these calls take (a face clamps
 * to its edges: DIRT_TEX_CLAMP is refused, as is DIRT_TEX_NEAREST with lod).  out [n, channels].
 * Backward: the n = rows x cols look-ups as a pixel grid (a flat list: rows = 1), tiled as dirt_texture_sample_backward_image
 * tiles it.  grad_out [n, channels] -> grad_pyramid [6, floats] (cleared by the call, by a kernel on `stream`, also when
 * n == 0; the gradient of every level -- dirt_texture_mip_collapse_batch with scenes = 6 turns it into the cube's),
 * grad_directions (triples `grad_dir_stride` >= 3 apart, only the three floats of a row are written; may be NULL) and grad_lod
 * (n; may be NULL, needs `lod`).  Both return 0 or DIRT_E_*, described by dirt_texture_last_error(); refused before any device
 * work: the flags above, sizes < 1, strides < 3, levels outside 1..dirt_texture_mip_levels(size, size, ...), NULL required
 * pointers, a pixel grid that overflows or has more than 2^31 - 1 tiles, grad_lod without lod. */
int dirt_texture_cube_forward(const float *pyramid, const float *directions, const float *lod, float *out, long long n, int size,
                              int channels, int levels, int dir_stride, float lod_bias, unsigned flags, void *stream);
int dirt_texture_cube_backward(const float *pyramid, const float *directions, const float *lod, const float *grad_out,
                               float *grad_pyramid, float *grad_directions, float *grad_lod, long long rows, long long cols,
                               int size, int channels, int levels, int dir_stride, int grad_dir_stride, float lod_bias,
                               unsigned flags, void *stream);
/* ENVIRONMENT PREFILTER: one level of a cube map convolved with a lobe on the sphere, and the transpose (the gradient).  These
 * two replace no reference interface; specification in dirt_amd/csrc/dirt_envmap.hip and DESIGN.md §7.  src, dst, grad_dst and
 * grad_src point at the level [size, size, channels] (dense) inside face 0; the six faces are `face_stride` floats apart, so a
 * level of a packed pyramid [6, floats] (face_stride = floats) is read and written where it lies, and a cube [6, size, size,
 * channels] has face_stride = size * size * channels.  kind: DIRT_ENVMAP_GGX, a GGX lobe of alpha = roughness^2 in (0, 1],
 * cut off at 1/256 of its peak while 16 alpha^2 < 1; DIRT_ENVMAP_LAMBERT, the clamped cosine (alpha is ignored).  Every output
 * texel is the weighted mean of the source texels of all six faces, the weights the lobe times the texels' solid angles.
 * norm [6, size, size]: the sum of an output texel's weights, in the kernel's own scale, written by the forward and read by the
 * backward only.  grad_src is fully written (no clear).  No atomics: the same bits on every run.  Both return 0 or DIRT_E_*,
 * described by dirt_texture_last_error(); refused before any device work: sizes or channels < 1, a size above 16384,
 * face_stride < size * size * channels, an unknown kind, alpha outside (0, 1] for DIRT_ENVMAP_GGX, NULL pointers, an output
 * that is the input. */
#define DIRT_ENVMAP_GGX 0u
#define DIRT_ENVMAP_LAMBERT 1u
int dirt_envmap_filter_forward(const float *src, float *dst, float *norm, int size, int channels, long long face_stride, float alpha,
                               unsigned kind, void *stream);
int dirt_envmap_filter_backward(const float *grad_dst, const float *norm, float *grad_src, int size, int channels,
                                long long face_stride, float alpha, unsigned kind, void *stream);

/*
 * G-buffer lighting of a deferred shader, fused.  Replaces the torch composition of the reference's shader
 * (samples/deferred.py:59-98): ambient + the reflectance models of dirt/lighting.py:175-344 per pixel, composited over a
 * background colour through the mask channel and clamped; specification in dirt_amd/csrc/dirt_shade.hip and DESIGN.md §7b.
 *   gbuffer [scenes, pixels, Cg], read in place (4-byte alignment suffices); off_colors / off_normals / off_positions: the
 *   first of three channels of each attribute inside a pixel, off_mask: the mask channel; off_positions / off_mask may be
 *   -1 (absent: no light may then need positions; every pixel covered).  Attributes may not overlap.
 *   params [param_scenes, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights], param_scenes = 1 (one block for every
 *   scene) or scenes: ambient[3], background[3], camera position[3], then per light {direction or position[3], colour[3],
 *   shininess, 0}.  light_kinds: two bits per light (DIRT_SHADE_DIFFUSE_DIRECTIONAL ...), light 0 lowest; double_sided:
 *   one bit per light.  flags: DIRT_SHADE_CLAMP (clamp to [clamp_lo, clamp_hi]), DIRT_SHADE_HAS_CAMERA (the block's
 *   camera position is meaningful: a specular light requires it).
 *   out [scenes, pixels, 3].
 * Backward: grad_out [scenes, pixels, 3] -> grad_gbuffer [scenes, pixels, Cg], fully written (zeros in the channels no
 * attribute uses), and grad_params [param_scenes, ...] shaped like params; either may be NULL and is then not computed.
 * grad_params needs `scratch`, caller-owned, of dirt_shade_scratch_bytes(scenes, pixels, lights) bytes (0: invalid
 * sizes): one row of partial sums per workgroup, added by a second launch in a fixed order -- no atomics, the same bits
 * on every run.  Zero scenes or pixels: success, nothing is launched or written.  Failures: dirt_last_error().
 */
#define DIRT_SHADE_MAX_LIGHTS 8
#define DIRT_SHADE_MAX_CHANNELS 1024
#define DIRT_SHADE_PARAM_HEAD 9
#define DIRT_SHADE_PARAM_LIGHT 8
#define DIRT_SHADE_DIFFUSE_DIRECTIONAL 0  /* dirt/lighting.py:175-218 */
#define DIRT_SHADE_SPECULAR_DIRECTIONAL 1 /* dirt/lighting.py:221-283 */
#define DIRT_SHADE_DIFFUSE_POINT 2        /* dirt/lighting.py:286-344 */
#define DIRT_SHADE_CLAMP 1u
#define DIRT_SHADE_HAS_CAMERA 2u
size_t dirt_shade_scratch_bytes(long long scenes, long long pixels, int lights);
int dirt_shade_forward(const float *gbuffer, const float *params, float *out, long long scenes, long long pixels, int Cg,
                       int off_colors, int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                       unsigned light_kinds, unsigned double_sided, float clamp_lo, float clamp_hi, unsigned flags,
                       void *stream);
int dirt_shade_backward(const float *gbuffer, const float *params, const float *grad_out, float *grad_gbuffer,
                        float *grad_params, void *scratch, size_t scratch_bytes, long long scenes, long long pixels, int Cg,
                        int off_colors, int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                        unsigned light_kinds, unsigned double_sided, float clamp_lo, float clamp_hi, unsigned flags,
                        void *stream);
/*
 * The same lighting with the colours in an image of their own, so that any colour source composes with it (a texture
 * look-up's output, a network's): colors [scenes, pixels, color_stride], the first three floats of a pixel its colour,
 * color_stride >= 3 (3: dense; 4: the first or the last three channels of an RGBA image; Cg: three channels of the
 * G-buffer itself), read in place, 4-byte alignment suffices.  The G-buffer then has no colour channels: there is no
 * off_colors, Cg may be as small as 3, and normals / positions / mask may sit anywhere, channel 0 included.  Everything
 * else is as above -- the same kernels with the colour's load and the store of its gradient redirected.
 * Backward: grad_colors [scenes, pixels, 3], dense; grad_gbuffer (fully written: no channel is a colour's), grad_colors
 * and grad_params may each be NULL and are then not computed -- all three NULL: success, nothing is launched.  Only
 * grad_params needs `scratch` (dirt_shade_scratch_bytes, as above).  NULL colors and color_stride < 3 are refused.
 */
int dirt_shade_albedo_forward(const float *gbuffer, const float *colors, const float *params, float *out, long long scenes,
                              long long pixels, int Cg, int color_stride, int off_normals, int off_positions, int off_mask,
                              int param_scenes, int lights, unsigned light_kinds, unsigned double_sided, float clamp_lo,
                              float clamp_hi, unsigned flags, void *stream);
int dirt_shade_albedo_backward(const float *gbuffer, const float *colors, const float *params, const float *grad_out,
                               float *grad_gbuffer, float *grad_colors, float *grad_params, void *scratch, size_t scratch_bytes,
                               long long scenes, long long pixels, int Cg, int color_stride, int off_normals, int off_positions,
                               int off_mask, int param_scenes, int lights, unsigned light_kinds, unsigned double_sided,
                               float clamp_lo, float clamp_hi, unsigned flags, void *stream);
/*
 * Second-order spherical-harmonic lighting of a G-buffer, fused (the reference has no such model; the specification is
 * DESIGN.md §7b and dirt_amd/lighting.py::spherical_harmonics).  Per pixel, with colour c, normal n, mask m:
 *     nh = n, or n / max(|n|, 1e-12) with DIRT_SHADE_SH_NORMALIZE;   E_j = sum_k scale_band(k) L[k, j] Y_k(nh)
 *     out_j = clamp(c_j E_j m + background_j (1 - m), clamp_lo, clamp_hi)
 * with the nine real basis functions in the order (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2) .. (2,2); scale0 / scale1 /
 * scale2 multiply bands 0 / 1 / 2 ((pi, 2 pi / 3, pi / 4): radiance coefficients to Lambertian irradiance).
 *   gbuffer [scenes, pixels, Cg], read in place.  colors NULL: the colour is the three channels at off_colors; otherwise
 *   colors [scenes, pixels, color_stride >= 3] as dirt_shade_albedo_forward takes it, and off_colors is not read.
 *   off_normals: three channels; off_mask: one, or -1 (every pixel covered).  Attributes may not overlap.
 *   params [param_scenes, DIRT_SHADE_SH_PARAMS], param_scenes = 1 or scenes: L[k, j] at 3 k + j, then background[3].
 *   flags: DIRT_SHADE_CLAMP, DIRT_SHADE_SH_NORMALIZE; any other bit is refused.   out [scenes, pixels, 3].
 * Backward: grad_gbuffer [scenes, pixels, Cg], fully written; grad_colors [scenes, pixels, 3], dense, only with colors;
 * grad_params like params.  Each may be NULL and is then not computed -- all three NULL: success, nothing is launched.
 * grad_params needs `scratch` of dirt_shade_sh_scratch_bytes(scenes, pixels) bytes (0: invalid sizes): one row of partial
 * sums per workgroup, added by a second launch in a fixed order -- no atomics, the same bits on every run.  Zero scenes
 * or pixels: success, nothing is launched or written.  Failures: dirt_last_error().
 */
#define DIRT_SHADE_SH_PARAMS 30
#define DIRT_SHADE_SH_NORMALIZE 4u
size_t dirt_shade_sh_scratch_bytes(long long scenes, long long pixels);
int dirt_shade_sh_forward(const float *gbuffer, const float *colors, const float *params, float *out, long long scenes,
                          long long pixels, int Cg, int color_stride, int off_colors, int off_normals, int off_mask,
                          int param_scenes, float scale0, float scale1, float scale2, float clamp_lo, float clamp_hi,
                          unsigned flags, void *stream);
int dirt_shade_sh_backward(const float *gbuffer, const float *colors, const float *params, const float *grad_out,
                           float *grad_gbuffer, float *grad_colors, float *grad_params, void *scratch, size_t scratch_bytes,
                           long long scenes, long long pixels, int Cg, int color_stride, int off_colors, int off_normals,
                           int off_mask, int param_scenes, float scale0, float scale1, float scale2, float clamp_lo,
                           float clamp_hi, unsigned flags, void *stream);
/*
 * Cook-Torrance (metallic-roughness) lighting of a G-buffer, fused (the reference has no such model; the specification is
 * DESIGN.md §7b and dirt_amd/lighting.py::cook_torrance).  Per pixel, with albedo c, normal n, position p, roughness r,
 * metalness mu, mask m, and every normalisation x / max(|x|, 1e-12):
 *     N = normalize(n)   v = normalize(camera - p)   rho = clamp(r, min_roughness, 1)   a2 = (rho^2)^2   k = (rho + 1)^2 / 8
 *     F0_j = dielectric_f0 (1 - mu) + c_j mu         nv = max(N . v, 0)
 *     per light:  l = normalize(-vector) (directional) | normalize(vector - p) (point);  h = normalize(l + v)
 *                 nl = max(N . l, 0)  nh = max(N . h, 0)  vh = max(v . h, 0)
 *                 D = a2 / (pi den^2), den = |N x h|^2 + a2 nh^2;   Vis = 0.25 / ((nl (1 - k) + k) (nv (1 - k) + k))
 *                 F_j = F0_j + (1 - F0_j) (1 - vh)^5;   kd_j = (1 - F_j)(1 - mu);   L_j = (kd_j c_j / pi + D Vis F_j) colour_j nl
 *     out_j = clamp((ambient_j c_j + sum L_j) m + background_j (1 - m), clamp_lo, clamp_hi)
 *   gbuffer [scenes, pixels, Cg], read in place.  colors NULL: the colour is the three channels at off_colors; otherwise
 *   colors [scenes, pixels, color_stride >= 3] and off_colors is not read.  material NULL: roughness and metalness are the two
 *   channels at off_material; otherwise material [scenes, pixels, material_stride >= 2] and off_material is not read.
 *   off_normals, off_positions: three channels each; off_mask: one, or -1 (every pixel covered).  Attributes may not overlap.
 *   params [param_scenes, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights], param_scenes = 1 or scenes: ambient[3],
 *   background[3], camera[3], then per light {vector[3], colour[3], 0, 0}.  lights: 0..DIRT_SHADE_PBR_MAX_LIGHTS; light_kinds:
 *   bit i set = light i is a point light (bits beyond `lights` are refused).  min_roughness in (0, 1], dielectric_f0 in [0, 1].
 *   flags: DIRT_SHADE_CLAMP; any other bit is refused.   out [scenes, pixels, 3].
 * Backward: grad_gbuffer [scenes, pixels, Cg], fully written; grad_colors [scenes, pixels, 3] and grad_material
 * [scenes, pixels, 2], dense, only with colors / material; grad_params like params.  Each may be NULL and is then not
 * computed -- all four NULL: success, nothing is launched.  grad_params needs `scratch` of
 * dirt_shade_pbr_scratch_bytes(scenes, pixels, lights) bytes (0: invalid sizes): one row of partial sums per workgroup, added
 * by a second launch in a fixed order -- no atomics, the same bits on every run.  Zero scenes or pixels: success, nothing is
 * launched or written.  Failures: dirt_last_error().
 */
#define DIRT_SHADE_PBR_MAX_LIGHTS 4
size_t dirt_shade_pbr_scratch_bytes(long long scenes, long long pixels, int lights);
int dirt_shade_pbr_forward(const float *gbuffer, const float *colors, const float *material, const float *params, float *out,
                           long long scenes, long long pixels, int Cg, int color_stride, int material_stride, int off_colors,
                           int off_material, int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                           unsigned light_kinds, float min_roughness, float dielectric_f0, float clamp_lo, float clamp_hi,
                           unsigned flags, void *stream);
int dirt_shade_pbr_backward(const float *gbuffer, const float *colors, const float *material, const float *params,
                            const float *grad_out, float *grad_gbuffer, float *grad_colors, float *grad_material,
                            float *grad_params, void *scratch, size_t scratch_bytes, long long scenes, long long pixels, int Cg,
                            int color_stride, int material_stride, int off_colors, int off_material, int off_normals,
                            int off_positions, int off_mask, int param_scenes, int lights, unsigned light_kinds,
                            float min_roughness, float dielectric_f0, float clamp_lo, float clamp_hi, unsigned flags, void *stream);
/*
 * The same with a visibility: one factor s_i per light and pixel (the output of dirt_shadow_forward) scales the light's weight,
 *     L_i,j = (kd_j c_j / pi + D Vis F_j) ((colour_i,j nl) s_i)
 * a plain float32 multiplication: s is not clamped, the ambient term is not shadowed, and s = 1 everywhere gives the bits of
 * dirt_shade_pbr_forward / _backward.  visibility: a pixel's `lights` factors are consecutive floats, visibility_stride >=
 * lights floats from pixel to pixel ([scenes, pixels, visibility_stride], read in place); lights: 1..DIRT_SHADE_PBR_MAX_LIGHTS
 * (0 is refused: there is nothing to scale).  Backward: grad_visibility [scenes, pixels, lights], dense, or NULL; the other
 * outputs and the scratch (dirt_shade_pbr_scratch_bytes) as dirt_shade_pbr_backward's -- all five NULL: success, nothing is
 * launched.  No atomics, the same bits on every run.
 */
int dirt_shade_pbr_visibility_forward(const float *gbuffer, const float *colors, const float *material, const float *visibility,
                                      const float *params, float *out, long long scenes, long long pixels, int Cg,
                                      int color_stride, int material_stride, int visibility_stride, int off_colors,
                                      int off_material, int off_normals, int off_positions, int off_mask, int param_scenes,
                                      int lights, unsigned light_kinds, float min_roughness, float dielectric_f0, float clamp_lo,
                                      float clamp_hi, unsigned flags, void *stream);
int dirt_shade_pbr_visibility_backward(const float *gbuffer, const float *colors, const float *material, const float *visibility,
                                       const float *params, const float *grad_out, float *grad_gbuffer, float *grad_colors,
                                       float *grad_material, float *grad_visibility, float *grad_params, void *scratch,
                                       size_t scratch_bytes, long long scenes, long long pixels, int Cg, int color_stride,
                                       int material_stride, int visibility_stride, int off_colors, int off_material,
                                       int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                                       unsigned light_kinds, float min_roughness, float dielectric_f0, float clamp_lo,
                                       float clamp_hi, unsigned flags, void *stream);

/*
 * Split-sum image-based lighting of a G-buffer, fused (the specification is DESIGN.md §7b and
 * dirt_amd/lighting.py::image_based_lighting).  Per pixel, with the attributes, N, v, rho and F0_j of dirt_shade_pbr_forward:
 *     nv_raw = N . v   nv = max(nv_raw, 0)   R = 2 nv_raw N - v
 *     (A, B) = bilinear look-up of table [S, S, 2] at column clamp(nv S - 0.5, 0, S - 1), row clamp(rho S - 0.5, 0, S - 1)
 *     S_j = F0_j A + B
 *     spec_j = the trilinear look-up of dirt_texture_cube_forward in `pyramid` at R, lod = rho (levels - 1)
 *     E_j    = its bilinear look-up in `irradiance` at n (not normalised: an all-zero normal gives 0)
 *     out_j = clamp(intensity_j ((1 - S_j)(1 - mu) c_j E_j + S_j spec_j) m + background_j (1 - m), clamp_lo, clamp_hi)
 *   gbuffer [scenes, rows * cols, Cg], colors, material, the channel offsets, min_roughness, dielectric_f0, the clamp and flags:
 *   as dirt_shade_pbr_forward.  rows x cols: a scene's pixel grid (a flat list: rows = 1); the backward scatters into the
 *   cubes on its 16 x 16 tiles.  params [param_scenes, DIRT_SHADE_PARAM_HEAD]: intensity[3], background[3], camera[3].
 *   pyramid [6, floats]: a packed pyramid per face of `levels` levels (1 .. the level count of `size`) and 3 channels, level 0
 *   of size `size`, laid out as dirt_texture_mip_build_batch makes it; irradiance [6, irradiance_size, irradiance_size, 3];
 *   table [table_size, table_size, 2], table_size in 2..DIRT_SHADE_IBL_MAX_TABLE.  One set serves every scene.
 * Backward: grad_gbuffer, grad_colors, grad_material, grad_params as dirt_shade_pbr_backward's; grad_pyramid like pyramid and
 * grad_irradiance like irradiance, cleared and then added into by the kernels of dirt_texture_cube_backward (float atomics
 * where a tile straddles faces: not the same bits on every run; everything else is).  Each may be NULL and is then not
 * computed -- all six NULL: success, nothing is launched.  grad_params, grad_pyramid and grad_irradiance need `scratch` of
 * dirt_shade_ibl_scratch_bytes(scenes, rows, cols) bytes (0: invalid sizes).  No gradient goes to the table.  Zero scenes or
 * pixels: success, the cubes' gradients are cleared.  Failures: dirt_last_error().
 */
#define DIRT_SHADE_IBL_MAX_TABLE 128
size_t dirt_shade_ibl_scratch_bytes(long long scenes, long long rows, long long cols);
int dirt_shade_ibl_forward(const float *gbuffer, const float *colors, const float *material, const float *params,
                           const float *pyramid, const float *irradiance, const float *table, float *out, long long scenes,
                           long long rows, long long cols, int Cg, int color_stride, int material_stride, int off_colors,
                           int off_material, int off_normals, int off_positions, int off_mask, int param_scenes, int size,
                           int levels, int irradiance_size, int table_size, float min_roughness, float dielectric_f0,
                           float clamp_lo, float clamp_hi, unsigned flags, void *stream);
int dirt_shade_ibl_backward(const float *gbuffer, const float *colors, const float *material, const float *params,
                            const float *pyramid, const float *irradiance, const float *table, const float *grad_out,
                            float *grad_gbuffer, float *grad_colors, float *grad_material, float *grad_params, float *grad_pyramid,
                            float *grad_irradiance, void *scratch, size_t scratch_bytes, long long scenes, long long rows,
                            long long cols, int Cg, int color_stride, int material_stride, int off_colors, int off_material,
                            int off_normals, int off_positions, int off_mask, int param_scenes, int size, int levels,
                            int irradiance_size, int table_size, float min_roughness, float dielectric_f0, float clamp_lo,
                            float clamp_hi, unsigned flags, void *stream);

/*
 * The vertex stage in front of the rasteriser, fused.  Replaces the torch composition of the reference's samples
 * (samples/deferred.py:40-51): world4 = v4 @ model, clip = world4 @ view_projection (row vectors), and the vertex normals
 * of dirt/lighting.py:21-28,31-89 (`vertex_normals`) or, with DIRT_GEOM_PRE_SPLIT, of dirt/lighting.py:97-129
 * (`vertex_normals_pre_split`), taken from the first three components of world4; specification in
 * dirt_amd/csrc/dirt_geometry.hip and DESIGN.md §7c.
 *   vertices [B, V, components], components = 3 (w = 1 is appended) or 4, 4-byte alignment suffices.
 *   faces [F, 3]: one topology for every scene.  offsets [V + 1], entries [3 F]: its inverted index -- the entries of
 *   vertex v are entries[offsets[v] .. offsets[v + 1]), each 3 * face + corner, ordered by face, then corner (a face that
 *   names a vertex twice has two entries; a vertex no face names has none).  The kernels trust the three arrays: every
 *   index must lie inside [0, V) / [0, 3 F) (dirt_amd.geometry.MeshTopology builds and checks them).
 *   model, view_projection [scenes, 4, 4] row-major with scenes = 1 (shared) or B; scenes = 0 and NULL: absent (model:
 *   the identity; view_projection: there is no clip output).
 *   clip [B, V, 4], world [B, V, 4], normals [B, V, 3]: each may be NULL and is then neither computed nor written.
 *   flags: DIRT_GEOM_PRE_SPLIT; DIRT_GEOM_LONG_LIST(n): lists of more than n entries are summed by a whole wave
 *   instead of one lane (0: DIRT_GEOM_LONG_LIST_DEFAULT).
 * One launch, no atomics.  B or V equal to 0: success, nothing is launched; F = 0 is a mesh without faces (zero normals).
 * Backward (the gradient of the above, dirt/lighting.py:21-28,31-89,97-129 and samples/deferred.py:40-51 under torch's
 * autograd: the norm of a zero vector has gradient 0): grad_clip / grad_world / grad_normals, each may be NULL (zero),
 * -> grad_vertices [B, V, components], grad_model and grad_view_projection (shaped like the matrices); each may be NULL
 * and is then not computed; those given are fully written.  `scratch` is caller-owned, of
 * dirt_geometry_scratch_bytes(B, V, F) bytes (0: invalid sizes): d loss / d (un-normalised normal sum) per vertex and
 * one row of partial matrix sums per workgroup, added by a last launch in a fixed order.  At most 2 launches, + 1 when
 * a matrix gradient is wanted; no atomics, the same bits on every run.  Failures: dirt_last_error().
 */
#define DIRT_GEOM_PRE_SPLIT 1u              /* dirt/lighting.py:97-129 instead of dirt/lighting.py:31-89 */
#define DIRT_GEOM_LONG_LIST_SHIFT 8
#define DIRT_GEOM_LONG_LIST_MASK 0xffff00u
#define DIRT_GEOM_LONG_LIST(n) (((unsigned)(n) << DIRT_GEOM_LONG_LIST_SHIFT) & DIRT_GEOM_LONG_LIST_MASK)
#define DIRT_GEOM_LONG_LIST_DEFAULT 64
#define DIRT_GEOM_MAX_VERTICES (1 << 28)
#define DIRT_GEOM_MAX_FACES (1 << 29)
size_t dirt_geometry_scratch_bytes(long long B, long long V, long long F);
int dirt_geometry_forward(const float *vertices, int components, const int32_t *faces, const int32_t *offsets,
                          const int32_t *entries, const float *model, int model_scenes, const float *view_projection,
                          int view_projection_scenes, float *clip, float *world, float *normals, long long B, long long V,
                          long long F, unsigned flags, void *stream);
int dirt_geometry_backward(const float *vertices, int components, const int32_t *faces, const int32_t *offsets,
                           const int32_t *entries, const float *model, int model_scenes, const float *view_projection,
                           int view_projection_scenes, const float *grad_clip, const float *grad_world,
                           const float *grad_normals, float *grad_vertices, float *grad_model, float *grad_view_projection,
                           void *scratch, size_t scratch_bytes, long long B, long long V, long long F, unsigned flags,
                           void *stream);

/*
 * Linear-blend skinning in front of the vertex stage, fused.  Extends what the reference's samples do with one matrix
 * for the whole mesh (samples/deferred.py:40-41: one `model` transform per scene) to a per-vertex blend of bone
 * matrices; specification in dirt_amd/csrc/dirt_skin.hip and DESIGN.md §7d.  Per scene, row vectors:
 *     M[v] = sum over k in slot order of bone_weights[v, k] * transforms[bone_indices[v, k]],   posed[v] = (v4 @ M[v])[:3]
 *   vertices [vertex_scenes, V, components], components = 3 (w = 1 is appended) or 4, 4-byte alignment suffices;
 *   vertex_scenes = 1 (one rest mesh for every scene) or B.
 *   bone_indices int32 [V, K], bone_weights [V, K], 1 <= K <= DIRT_SKIN_MAX_INFLUENCES: one table for every scene.  Weights
 *   are taken as given (nothing is renormalised; a zero weight is padding; a vertex may name a bone in two slots).
 *   transforms [transform_scenes, J, 4, 4] row-major (translation in row 3), transform_scenes = 1 or B, J <=
 *   DIRT_SKIN_MAX_BONES.  Column 3 is never read.  Up to DIRT_SKIN_LDS_BONES bones a workgroup stages the scene's 4x3
 *   blocks in LDS (12 KB); with more they are read through the caches.
 *   posed [B, V, 3]; NULL: nothing is computed.
 * One launch, no atomics.  B or V equal to 0: success, nothing is launched.  flags: none defined, must be 0.
 * Backward: grad_posed [B, V, 3] -> grad_vertices (shaped like vertices), grad_transforms (shaped like transforms, column
 * 3 written as zero, a bone no vertex names all zero) and grad_weights [V, K]; each may be NULL and is then not computed;
 * those given are fully written, an operand shared by the scenes receiving the sum over the scenes.  grad_transforms
 * needs the inverted index of bone_indices (dirt_amd.skinning.SkinWeights builds it):
 *   entries [V K]: the positions v * K + k, ordered by bone, then position;
 *   chunk_table [chunks, 3]: (bone, begin, end) -- every bone's run of `entries` cut into pieces of a fixed number of
 *   entries, none spanning two bones, ordered by bone, then begin; chunks <= DIRT_SKIN_MAX_CHUNKS;
 *   chunk_offsets [J + 1]: the chunks of bone j are chunk_offsets[j] .. chunk_offsets[j + 1]);
 * and `scratch`, caller-owned, of dirt_skin_scratch_bytes(B, chunks) = 4 * 12 * B * chunks bytes (0: invalid sizes): one
 * row of partial sums per (scene, chunk), added by a second launch in a fixed order.  The kernels trust the index arrays:
 * every bone index must lie inside [0, J), every entry inside [0, V K).  At most 4 launches; no atomics, the same bits on
 * every run.  Failures: dirt_last_error().
 */
#define DIRT_SKIN_MAX_INFLUENCES 8
#define DIRT_SKIN_MAX_BONES 65536
#define DIRT_SKIN_LDS_BONES 256
#define DIRT_SKIN_MAX_VERTICES (1 << 28)
#define DIRT_SKIN_MAX_ENTRIES (1 << 30) /* V K: the positions v * K + k and the kernels' entry counters are int32 */
#define DIRT_SKIN_MAX_CHUNKS 0x7fffffff
size_t dirt_skin_scratch_bytes(long long B, long long chunks);
int dirt_skin_forward(const float *vertices, int components, int vertex_scenes, const int32_t *bone_indices,
                      const float *bone_weights, const float *transforms, int transform_scenes, float *posed, long long B,
                      long long V, int K, int J, unsigned flags, void *stream);
int dirt_skin_backward(const float *vertices, int components, int vertex_scenes, const int32_t *bone_indices,
                       const float *bone_weights, const float *transforms, int transform_scenes, const int32_t *entries,
                       const int32_t *chunk_table, const int32_t *chunk_offsets, const float *grad_posed,
                       float *grad_vertices, float *grad_transforms, float *grad_weights, void *scratch,
                       size_t scratch_bytes, long long B, long long V, int K, int J, long long chunks, unsigned flags,
                       void *stream);

/*
 * Forward kinematics in front of the skinning stage, fused.  Extends the one matrices.rodrigues / compose per mesh of the
 * reference's samples (samples/deferred.py:40-41; dirt/matrices.py:15-61,183-207) to a skeleton: a forest of J <=
 * DIRT_KINEMATICS_MAX_JOINTS joints whose parents come before their children; specification in
 * dirt_amd/csrc/dirt_kinematics.hip and DESIGN.md §7e.  Per scene, float32, row vectors:
 *     R[j] = rodrigues(rotations[j]) (3 x 3, dirt/matrices.py:15-61 operation for operation),  tl[j] = p[j] - p[j] @ R[j]
 *     root: S3[j] = R[j], t[j] = tl[j];   else: S3[j] = R[j] @ S3[parent],  t[j] = tl[j] @ S3[parent] + t[parent]
 *     transforms[j] = [[S3[j], 0], [t[j], 1]],   posed_joints[j] = p[j] @ S3[j] + t[j]
 *   rotations [rotation_scenes, J, 3] angle-axis vectors, joints [joint_scenes, J, 3] rest-pose positions p; each scene count
 *   is 1 (shared by the scenes) or B; 4-byte alignment suffices.
 *   parents int32 [J] (-1: a root), and the index dirt_amd.kinematics.Skeleton builds from it: order [J], the joints by
 *   depth, then index; level_offsets [levels + 1], the joints of depth d being order[level_offsets[d] ..
 *   level_offsets[d + 1]); 1 <= levels <= J.  The kernels trust the index arrays.
 *   transforms [B, J, 4, 4] (what dirt_skin_forward takes; column 3 written as (0, 0, 0, 1)), posed_joints [B, J, 3]: each
 *   may be NULL and is then not written.
 * One launch of a workgroup per scene, no atomics.  B or J equal to 0: success, nothing is launched.  flags: none defined,
 * must be 0.
 * Backward: grad_transforms [B, J, 4, 4] (column 3 is ignored) and grad_posed_joints [B, J, 3], each may be NULL (zero), ->
 * grad_rotations and grad_joints (shaped like the operands); each may be NULL and is then not computed; those given are
 * fully written, an operand shared by the scenes receiving the sum over the scenes.  Needs, beside the above, the inverted
 * index of parents: child_entries, the non-root joints ordered by parent, then index, and child_offsets [J + 1] (the
 * children of j are child_entries[child_offsets[j] .. child_offsets[j + 1])).  `scratch`, caller-owned, of
 * dirt_kinematics_scratch_bytes(B, J) = 4 * 6 * B * J bytes (0: invalid sizes), is needed -- and checked -- only where a
 * wanted gradient belongs to an operand shared by B > 1 scenes: one row per (scene, joint), added by a second launch in a
 * fixed order.  1 launch, + 1 for a shared operand; no atomics, the same bits on every run.  Failures: dirt_last_error().
 */
#define DIRT_KINEMATICS_MAX_JOINTS 256 /* the skinning stage's DIRT_SKIN_LDS_BONES: a scene's joints live in 12 KB of LDS */
size_t dirt_kinematics_scratch_bytes(long long B, long long J);
int dirt_kinematics_forward(const float *rotations, int rotation_scenes, const float *joints, int joint_scenes,
                            const int32_t *parents, const int32_t *order, const int32_t *level_offsets, int levels,
                            float *transforms, float *posed_joints, long long B, int J, unsigned flags, void *stream);
int dirt_kinematics_backward(const float *rotations, int rotation_scenes, const float *joints, int joint_scenes,
                             const int32_t *parents, const int32_t *order, const int32_t *level_offsets, int levels,
                             const int32_t *child_entries, const int32_t *child_offsets, const float *grad_transforms,
                             const float *grad_posed_joints, float *grad_rotations, float *grad_joints, void *scratch,
                             size_t scratch_bytes, long long B, int J, unsigned flags, void *stream);

/*
 * Blend shapes in front of the kinematics and skinning stages, fused.  Extends the one fixed mesh per scene of the
 * reference's samples (samples/deferred.py:40-41 moves it with one matrix) to the rest mesh of a body, hand or face model:
 * template + sum of coefficient x direction, and the joints regressed from it; specification in
 * dirt_amd/csrc/dirt_blend.hip and DESIGN.md §7f.  Per scene, float32:
 *     vertices[v] = template[v] + sum over k < K of c[k] * directions[k, v]
 *     joints[j]   = sum over the non-zeros (j, v) of the regressor of w[j, v] * template[v]
 *                 + sum over k < Ks of c[k] * joint_directions[k, j]
 *   template_vertices [template_scenes, V, 3], coefficients [coefficient_scenes, K]: each scene count is 1 (shared by the
 *   scenes) or B; 4-byte alignment suffices.  V <= DIRT_BLEND_MAX_VERTICES, 0 <= K <= DIRT_BLEND_MAX_SHAPES.
 *   directions: the packed table [K, stride] dirt_amd.blendshapes.BlendShapes builds -- row k holds directions[k] as 3 V
 *   floats, then zeros up to `stride`, a multiple of 4 floats; the base 16-byte aligned (checked): every row starts 16-byte
 *   aligned and is read 16 bytes per lane.
 *   The regressor [J, V], J <= DIRT_BLEND_MAX_JOINTS, as its non-zeros ordered by joint, then vertex (CSR): row_offsets
 *   [J + 1], row_vertices and row_weights (the non-zeros of joint j are row_offsets[j] .. row_offsets[j + 1]); at most
 *   DIRT_BLEND_MAX_ENTRIES non-zeros.  joint_directions [Ks, J, 3] = regressor @ directions[k] for the first Ks <= K
 *   directions, the ones that move the joints (computed once, in float64, by the caller).  The kernels trust the index arrays.
 *   vertices [B, V, 3], joints [B, J, 3]: each may be NULL and is then not computed.
 * One launch, no atomics.  B or V equal to 0: success, nothing is launched; K = 0 copies the template.  flags: none
 * defined, must be 0.
 * Backward: grad_vertices [B, V, 3] and grad_joints [B, J, 3], each may be NULL (zero), -> grad_template and
 * grad_coefficients (shaped like the operands); each may be NULL and is then not computed; those given are fully written,
 * an operand shared by the scenes receiving the sum over the scenes.  The directions, the regressor and joint_directions
 * are constants: they receive no gradient.  grad_template gathers grad_joints over the regressor's inverted index (CSC):
 * column_offsets [V + 1], column_joints and column_weights, the non-zeros ordered by vertex, then joint.  grad_coefficients
 * needs `scratch`, caller-owned, of dirt_blend_scratch_bytes(B, V, K) = 4 * 32 * ceil(B / 4) * ceil(K / 8) * ceil(3 V / 1024)
 * bytes (0: invalid sizes): one row of partial sums per workgroup of the first launch, added by a second launch in a
 * fixed order.  At most 3 launches; no atomics, the same bits on every run.  Failures: dirt_last_error().
 */
#define DIRT_BLEND_MAX_SHAPES 4096
#define DIRT_BLEND_MAX_VERTICES (1 << 26)
#define DIRT_BLEND_MAX_JOINTS 256 /* DIRT_KINEMATICS_MAX_JOINTS: what the next stage takes */
#define DIRT_BLEND_MAX_ENTRIES (1 << 30) /* the regressor's non-zeros: their offsets are int32 */
size_t dirt_blend_scratch_bytes(long long B, long long V, long long K);
int dirt_blend_forward(const float *template_vertices, int template_scenes, const float *coefficients,
                       int coefficient_scenes, const float *directions, long long stride, const int32_t *row_offsets,
                       const int32_t *row_vertices, const float *row_weights, const float *joint_directions,
                       float *vertices, float *joints, long long B, long long V, int K, int Ks, int J, unsigned flags,
                       void *stream);
int dirt_blend_backward(int template_scenes, int coefficient_scenes, const float *directions, long long stride,
                        const int32_t *column_offsets, const int32_t *column_joints, const float *column_weights,
                        const float *joint_directions, const float *grad_vertices, const float *grad_joints,
                        float *grad_template, float *grad_coefficients, void *scratch, size_t scratch_bytes, long long B,
                        long long V, int K, int Ks, int J, unsigned flags, void *stream);

/*
 * Tangent-space normal mapping, fused; specification in dirt_amd/csrc/dirt_tangent.hip, dirt_amd/csrc/dirt_normal_map.hip
 * and DESIGN.md §7g (dirt_amd/lighting.py: `vertex_tangents`, `perturb_normals`).
 *
 * dirt_tangent_*: per-vertex tangent frames from the uv parametrisation, over the inverted index of the vertex stage.
 *   vertices [B, V, components] (components = 3 or 4; only x, y, z are read), normals [B, V, 3] (taken as given),
 *   uvs [V, 2] shared by the scenes, faces / offsets / entries as for dirt_geometry_forward (trusted likewise)
 *   -> tangents [B, V, 4]: the unit tangent and the handedness -1 / +1; a vertex whose tangent sum has no part orthogonal
 *   to its normal (no face, degenerate uv triangles only) gets (0, 0, 0, 1).  One launch.
 * Backward: grad_tangents [B, V, 4] (the handedness' component is not read) -> grad_vertices [B, V, components] (a fourth
 *   component gets zeros) and grad_normals [B, V, 3]; each may be NULL and is then not computed; those given are fully
 *   written.  grad_vertices needs `scratch` of dirt_tangent_scratch_bytes(B, V, F) bytes (0: invalid sizes): d loss /
 *   d (tangent sum) per vertex, which a second launch gathers over each vertex's faces.  No atomics, the same bits on
 *   every run.  B or V equal to 0: success, nothing is launched.
 *
 * dirt_normal_map_*: a G-buffer [scenes, pixels, Cg] (7 <= Cg <= DIRT_SHADE_MAX_CHANNELS) with three channels of normals at
 *   off_normals and four of tangent and handedness at off_tangents (no overlap), and a texel of three floats per pixel,
 *   map_stride >= 3 floats apart -> out [scenes, pixels, Cg]: the G-buffer with its normal channels replaced by the
 *   shading normal (a pixel with a zero normal, no tangent orthogonal to it or a zero decoded texel keeps its normal),
 *   every other channel copied.  flags: DIRT_NORMAL_MAP_ENCODED (the texel is decoded as 2 m - 1); the decoded x and y
 *   are multiplied by `strength`.  One launch.
 * Backward: grad_out [scenes, pixels, Cg] -> grad_gbuffer [scenes, pixels, Cg] (grad_out with the normal channels
 *   replaced by the normal's gradient and the tangent's and handedness' added to theirs) and grad_normal_map
 *   [scenes, pixels, 3] dense; each may be NULL and is then not computed.  One launch, no scratch, no atomics.
 *   scenes * pixels equal to 0: success, nothing is launched.
 * Failures: dirt_last_error().
 */
#define DIRT_NORMAL_MAP_ENCODED 1u
size_t dirt_tangent_scratch_bytes(long long B, long long V, long long F);
int dirt_tangent_forward(const float *vertices, int components, const float *normals, const float *uvs, const int32_t *faces,
                         const int32_t *offsets, const int32_t *entries, float *tangents, long long B, long long V,
                         long long F, void *stream);
int dirt_tangent_backward(const float *vertices, int components, const float *normals, const float *uvs, const int32_t *faces,
                          const int32_t *offsets, const int32_t *entries, const float *grad_tangents, float *grad_vertices,
                          float *grad_normals, void *scratch, size_t scratch_bytes, long long B, long long V, long long F,
                          void *stream);
int dirt_normal_map_forward(const float *gbuffer, const float *normal_map, float *out, long long scenes, long long pixels,
                            int Cg, int map_stride, int off_normals, int off_tangents, float strength, unsigned flags,
                            void *stream);
int dirt_normal_map_backward(const float *gbuffer, const float *normal_map, const float *grad_out, float *grad_gbuffer,
                             float *grad_normal_map, long long scenes, long long pixels, int Cg, int map_stride,
                             int off_normals, int off_tangents, float strength, unsigned flags, void *stream);

/*
 * The look-up of shadow maps from a G-buffer, fused; specification in dirt_amd/csrc/dirt_shadow.hip and DESIGN.md §7h
 * (dirt_amd/lighting.py::shadow_visibility).  Per pixel and light, with K = kernel and h = (K - 1) / 2:
 *     q = p + normal_offset n / max(|n|, 1e-12)      (x, y, z, w) = [q, 1] @ M (row vectors)      d = z
 *     col = (x / w + 1) Ws / 2 - 0.5      row = (1 - y / w) Hs / 2 - 0.5      (r0, fr), (c0, fc): floor - h and fraction
 *     v = (1 / K^2) sum_{a, b = 0..K} wr[a] wc[b] S(r0 + a, c0 + b),   wr[0] = 1 - fr, wr[K] = fr, 1 between; wc likewise
 *     S = s((Z[r, c] - d + bias) / softness + 1/2) inside the map, 1 outside;   s(t) = u u (3 - 2 u), u = clamp(t, 0, 1)
 *     out = 1 - m (1 - v);   v = 1 where not w > 0 or where the whole window lies off the map
 *   gbuffer [scenes, pixels, Cg] with three channels of world positions at off_positions, three of normals at off_normals
 *   (-1: none; needed when normal_offset != 0, not read otherwise) and the mask at off_mask (-1: every pixel is covered);
 *   maps [map_scenes, lights, Hs, Ws] and matrices [matrix_scenes, lights, 4, 4] with map_scenes and matrix_scenes each 1
 *   (one set serves every scene) or `scenes`; lights: 1..DIRT_SHADOW_MAX_LIGHTS; kernel: 1, 3 or 5; softness > 0
 *   -> out [scenes, pixels, lights].  One launch.
 * Backward: rows x cols is a scene's pixel grid (a flat list: rows = 1); grad_out [scenes, rows * cols, lights] ->
 *   grad_gbuffer [scenes, rows * cols, Cg] (every row written whole, exact zeros in the channels no attribute uses),
 *   grad_maps like maps (cleared, then added into with float atomics: one per touched texel of a 16 x 16 tile whose window
 *   box fits the LDS patch, one per tap otherwise and for a flat list; not the same bits on every run) and grad_matrices
 *   like matrices (per-workgroup sums in `scratch` of dirt_shadow_scratch_bytes(scenes, rows, cols, lights) bytes -- 0:
 *   invalid sizes --, added in a fixed order: the same bits on every run, as grad_gbuffer).  Each may be NULL and is then
 *   not computed -- all three NULL: success, nothing is launched.  Zero scenes or pixels: success, grad_maps and
 *   grad_matrices are cleared.
 * Refused before any device work, with a sentence in dirt_last_error(): negative sizes, more than 65535 scenes or 2^40
 *   pixels, a channel count outside 1..DIRT_SHADE_MAX_CHANNELS, a light count outside 1..DIRT_SHADOW_MAX_LIGHTS, a map
 *   that is empty or has more than 2^31 - 1 texels, map_scenes or matrix_scenes that is neither 1 nor scenes, a kernel
 *   other than 1, 3, 5, a softness that is not a finite number > 0 or whose float32 reciprocal is not finite (below
 *   2.94e-39: the kernels multiply by it), a bias or normal_offset that is not finite, a
 *   normal_offset without normals, attributes that do not fit or overlap, a NULL operand, a pixel grid the backward's
 *   tiles cannot index, a scratch that is missing, too small or misaligned.
 */
#define DIRT_SHADOW_MAX_LIGHTS 4
size_t dirt_shadow_scratch_bytes(long long scenes, long long rows, long long cols, int lights);
int dirt_shadow_forward(const float *gbuffer, const float *maps, const float *matrices, float *out, long long scenes,
                        long long pixels, int Cg, int off_positions, int off_normals, int off_mask, int lights, int Hs, int Ws,
                        int map_scenes, int matrix_scenes, int kernel, float bias, float softness, float normal_offset,
                        void *stream);
int dirt_shadow_backward(const float *gbuffer, const float *maps, const float *matrices, const float *grad_out,
                         float *grad_gbuffer, float *grad_maps, float *grad_matrices, void *scratch, size_t scratch_bytes,
                         long long scenes, long long rows, long long cols, int Cg, int off_positions, int off_normals,
                         int off_mask, int lights, int Hs, int Ws, int map_scenes, int matrix_scenes, int kernel, float bias,
                         float softness, float normal_offset, void *stream);

/*
 * The environment seen behind the mesh, fused; specification in dirt_amd/csrc/dirt_background.hip and DESIGN.md §7i
 * (dirt_amd/lighting.py::environment_background).  Per pixel (r, c) of a rows x cols image, with M = the scene's matrix
 * (clip -> world, row vectors), I its intensity and m its mask (0 without one):
 *     nx = 2 (c + 0.5) / cols - 1      ny = 1 - 2 (r + 0.5) / rows      h(z) = [nx, ny, z, 1] @ M
 *     d = h(0).xyz / h(0).w - h(-1).xyz / h(-1).w          out_j = (1 - m) I_j E_j(d)
 * E: the look-up of dirt_texture_cube_forward at d -- `filter` DIRT_BACKGROUND_NEAREST, _BILINEAR or _TRILINEAR, the last at
 * the level of detail lod + lod_bias or, with DIRT_BACKGROUND_FOOTPRINT in `flags`, at log2 of the pixel's analytic footprint
 * in texels + lod_bias (lod is not read).  A pixel whose d is not valid (h.w = 0, anything non-finite) or whose 1 - m is 0
 * gives 0, reads no texel and adds to no gradient but grad_mask.
 *   environment [6, floats]: a packed pyramid per face of `levels` levels of a size x size x 3 cube, as
 *   dirt_texture_mip_build_batch lays the six faces out (levels = 1: the cube [6, size, size, 3] itself; anything but
 *   _TRILINEAR takes 1 only); matrices [matrix_scenes, 4, 4], intensity [intensity_scenes, 3]; mask: NULL, or a scene's
 *   rows * cols values mask_stride >= 1 floats apart, scene after scene (mask_scenes = scenes) or one for all (1);
 *   out [scenes, rows, cols, 3].  Each ..._scenes is 1 (shared by the scenes) or scenes.
 * Backward: grad_out like out; grad_environment like environment (cleared, then added into with float atomics by the
 *   kernels of dirt_texture_cube_backward: not the same bits on every run), grad_matrices like matrices and grad_intensity
 *   like intensity (per-workgroup sums in `scratch` of dirt_background_scratch_bytes(scenes, rows, cols) bytes -- 0:
 *   invalid sizes --, added in a fixed order, over the scenes in scene order where shared: the same bits on every run),
 *   grad_mask [scenes, rows * cols], dense, one value per scene and pixel whatever mask_scenes (needs mask).  Each may be
 *   NULL and is then not computed -- all four NULL: success, nothing is launched; the scratch is needed unless grad_mask
 *   alone is asked for.  Zero scenes or pixels: success, the first three are cleared.
 * Refused before any device work, with a sentence in dirt_last_error(): a scene count outside 0..65535, a pixel grid that
 *   is negative, has more than 2^31 - 1 rows or columns or 2^40 pixels, an unknown filter or flag, the footprint without
 *   _TRILINEAR, a size outside 1..32768, levels the size does not have or more than 1 without _TRILINEAR, a ..._scenes that
 *   is neither 1 nor scenes, mask_stride < 1, a lod or lod_bias that is not finite, a NULL operand, grad_mask without
 *   mask, a scratch that is missing, too small or misaligned.
 */
#define DIRT_BACKGROUND_NEAREST 0
#define DIRT_BACKGROUND_BILINEAR 1
#define DIRT_BACKGROUND_TRILINEAR 2
#define DIRT_BACKGROUND_FOOTPRINT 1u
size_t dirt_background_scratch_bytes(long long scenes, long long rows, long long cols);
int dirt_background_forward(const float *environment, const float *matrices, const float *intensity, const float *mask,
                            float *out, long long scenes, long long rows, long long cols, int size, int levels,
                            int matrix_scenes, int intensity_scenes, int mask_scenes, int mask_stride, int filter, float lod,
                            float lod_bias, unsigned flags, void *stream);
int dirt_background_backward(const float *environment, const float *matrices, const float *intensity, const float *mask,
                             const float *grad_out, float *grad_environment, float *grad_matrices, float *grad_intensity,
                             float *grad_mask, void *scratch, size_t scratch_bytes, long long scenes, long long rows,
                             long long cols, int size, int levels, int matrix_scenes, int intensity_scenes, int mask_scenes,
                             int mask_stride, int filter, float lod, float lod_bias, unsigned flags, void *stream);

/*
 * The last stage of the renderer, fused: supersample resolve, exposure, tone curve, sRGB encode and clamp; specification in
 * dirt_amd/csrc/dirt_resolve.hip and DESIGN.md §7j (dirt_amd/lighting.py::resolve_image).  Per pixel (r, c) and channel ch of
 * a rows x cols output, with S = factor, e the scene's exposure and w its white point, in float32 and in this order:
 *     acc = 0;  for i in 0..S-1, for j in 0..S-1:  acc += image[S r + i, S c + j, ch] (+ add[...]);   L = acc * float(1 / S^2)
 *     E = e[ch] L;   t = E (DIRT_RESOLVE_LINEAR), or with x = max(E, 0):  x (1 + x / (w w)) / (1 + x)  (_REINHARD),
 *     x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14)  (_ACES);   y = t (DIRT_RESOLVE_ENCODE_LINEAR) or, with u = max(t, 0),
 *     12.92 u where u <= 0.0031308, else 1.055 powf(u, 1 / 2.4) - 0.055  (_ENCODE_SRGB);   out = clamp(y, clamp_lo, clamp_hi)
 *     with DIRT_RESOLVE_CLAMP in `flags`.  A NaN stays NaN.
 *   image, add (NULL: none): a scene's S rows x S cols samples of `channels` floats, image_stride / add_stride >= channels
 *   floats apart, scene after scene (image_scenes = scenes) or one image for all (1); exposure [exposure_scenes, channels];
 *   white [white_scenes] with _REINHARD and only with it, else NULL; out and linear (NULL: not written; L, what the backward
 *   pass reads) [scenes, rows, cols, channels].  Each ..._scenes is 1 (shared by the scenes) or scenes.
 * Backward: grad_out like out; grad_image and grad_add [scenes, S rows, S cols, channels], dense, one value per scene and
 *   sample whatever image_scenes; grad_exposure like exposure and grad_white like white (per-workgroup sums in `scratch` of
 *   dirt_resolve_scratch_bytes(scenes, rows, cols, channels, factor) bytes -- 0: invalid sizes --, added in a fixed order, over
 *   the scenes in scene order where shared: the same bits on every run).  Each may be NULL and is then not computed -- all
 *   four NULL: success, nothing is launched; the scratch is needed for grad_exposure and grad_white.  Zero scenes or pixels:
 *   success, the last two are cleared.
 * Refused before any device work, with a sentence in dirt_last_error(): a scene count outside 0..65535, channels outside
 *   1..DIRT_RESOLVE_MAX_CHANNELS, a factor outside 1..DIRT_RESOLVE_MAX_FACTOR, an image that is negative, has more than
 *   (2^31 - 1) / DIRT_RESOLVE_MAX_FACTOR rows or columns or 2^36 pixels, an unknown curve, encoding or flag, clamp_lo >
 *   clamp_hi, a ..._scenes that is neither 1 nor scenes, white without _REINHARD or _REINHARD without white, a stride below
 *   channels, a NULL operand, grad_white without white, a scratch that is missing, too small or misaligned.
 */
#define DIRT_RESOLVE_MAX_FACTOR 4
#define DIRT_RESOLVE_MAX_CHANNELS 4
#define DIRT_RESOLVE_LINEAR 0
#define DIRT_RESOLVE_REINHARD 1
#define DIRT_RESOLVE_ACES 2
#define DIRT_RESOLVE_ENCODE_LINEAR 0
#define DIRT_RESOLVE_ENCODE_SRGB 1
#define DIRT_RESOLVE_CLAMP 1u
size_t dirt_resolve_scratch_bytes(long long scenes, long long rows, long long cols, int channels, int factor);
int dirt_resolve_forward(const float *image, const float *add, const float *exposure, const float *white, float *out,
                         float *linear, long long scenes, long long rows, long long cols, int channels, int factor,
                         int image_stride, int add_stride, int image_scenes, int add_scenes, int exposure_scenes,
                         int white_scenes, int curve, int encode, float clamp_lo, float clamp_hi, unsigned flags, void *stream);
int dirt_resolve_backward(const float *linear, const float *exposure, const float *white, const float *grad_out,
                          float *grad_image, float *grad_add, float *grad_exposure, float *grad_white, void *scratch,
                          size_t scratch_bytes, long long scenes, long long rows, long long cols, int channels, int factor,
                          int exposure_scenes, int white_scenes, int curve, int encode, float clamp_lo, float clamp_hi,
                          unsigned flags, void *stream);

/*
 * Lat-long (equirectangular) environment maps, fused: a panorama resampled into a cube and a cube into a panorama, both
 * supersampled and under a rotation; specification in dirt_amd/csrc/dirt_panorama.hip and DESIGN.md §7k
 * (dirt_amd/texture.py::panorama_to_cube_dense, cube_to_panorama_dense).  The panorama [rows, cols, channels] has row 0 at
 * +Y, its middle column looks along -Z and its columns grow towards +X; its columns wrap, its rows clamp, the look-up is
 * bilinear.  The cube is [6, size, size, channels], faces in OpenGL order, each face clamped to its own edges.  rotation
 * [3, 3], row vectors: its rows are the images of the panorama's axes in the cube's frame.
 *   dirt_panorama_to_cube_forward: cube texel (f, r, c) = the mean of the samples x samples look-ups of the panorama at
 *   e @ rotation^T, e the direction through the sub-sample's place on the face.
 *   dirt_cube_to_panorama_forward: panorama pixel (i, j) = the mean of the samples x samples look-ups of the cube (as
 *   dirt_texture_cube_forward's, bilinear) at d @ rotation, d the direction of the sub-sample's (theta, phi).
 *   A direction that is not finite or all zero after the rotation adds 0.  The samples are added in row-major order, then
 *   multiplied by float(1 / samples^2).
 * Backward: grad_cube / grad_panorama (the incoming one) like the forward's output.  The gradient of the sampled operand
 *   (grad_panorama of dirt_panorama_to_cube_backward, grad_cube of dirt_cube_to_panorama_backward) is cleared, then added into
 *   with float atomics (the latter by the kernels of dirt_texture_cube_backward): not the same bits on every run.
 *   grad_rotation [3, 3]: per-workgroup sums in `scratch`, added in a fixed order: the same bits on every run.  Either may be
 *   NULL and is then not computed -- both NULL: success, nothing is launched.  scratch: dirt_panorama_scratch_bytes(rows, cols,
 *   size, channels, samples, to_cube) bytes (0: invalid sizes), to_cube = 1 for dirt_panorama_to_cube_backward, which needs it
 *   for grad_rotation only, 0 for dirt_cube_to_panorama_backward, which always needs it.
 * Refused before any device work, with a sentence in dirt_texture_last_error(): rows, cols, size or channels below 1, samples
 *   outside 1..DIRT_PANORAMA_MAX_SAMPLES, a size above 32768, a panorama of more than 2^20 rows or columns, more than 65536
 *   channels, a grid of samples of more than 2^31 - 1 tiles (dirt_cube_to_panorama_*), a NULL operand, a scratch that is
 *   missing, too small or misaligned.
 */
#define DIRT_PANORAMA_MAX_SAMPLES 4
size_t dirt_panorama_scratch_bytes(long long rows, long long cols, int size, int channels, int samples, int to_cube);
int dirt_panorama_to_cube_forward(const float *panorama, const float *rotation, float *cube, long long rows, long long cols,
                                  int size, int channels, int samples, void *stream);
int dirt_panorama_to_cube_backward(const float *panorama, const float *rotation, const float *grad_cube, float *grad_panorama,
                                   float *grad_rotation, void *scratch, size_t scratch_bytes, long long rows, long long cols,
                                   int size, int channels, int samples, void *stream);
int dirt_cube_to_panorama_forward(const float *cube, const float *rotation, float *panorama, long long rows, long long cols,
                                  int size, int channels, int samples, void *stream);
int dirt_cube_to_panorama_backward(const float *cube, const float *rotation, const float *grad_panorama, float *grad_cube,
                                   float *grad_rotation, void *scratch, size_t scratch_bytes, long long rows, long long cols,
                                   int size, int channels, int samples, void *stream);

/*
 * Per-kernel timing (host-side state only).  Slots are the library's kernels; dirt_profile_count()
 * returns how many there are, dirt_profile_name(i) their names.  dirt_profile_read waits for the
 * recorded events of calls made with DIRT_FLAG_PROFILE on this thread, adds them to the running
 * totals and returns total milliseconds and launch count of slot i; dirt_profile_reset clears the
 * totals.  Returns 0 or DIRT_E_*.
 */
int dirt_profile_count(void);
const char *dirt_profile_name(int slot);
int dirt_profile_read(int slot, double *total_ms, long long *launches);
int dirt_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* DIRT_HIP_H */
