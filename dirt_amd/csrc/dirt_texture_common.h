// dirt_texture_common.h -- what the texture kernels share (dirt_texture.hip: nearest / bilinear; dirt_texture_mip.hip: trilinear over a
// mip pyramid; dirt_texture_cube.hip: the three by direction into a cube map).  Per look-up: (u, v) -> fractional (row, column) index of the reference's samples/textured.py:16-26, the four bilinear taps of
// :36-60, the channel-vector loads / stores, the blend.  The pieces of the backward tile scheme.  The rule of a batched launch (a texture per scene).
// Host: the pixel grid, a launch for one texture or a batch (Scenes), the scene count of a batch, the clear of a buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include "dirt_stage.h"

namespace dirt {

// tf.clip_by_value(x, 0, 1) = minimum(maximum(x, 0), 1), which keeps a NaN (fminf / fmaxf would return the bound instead)
__device__ __forceinline__ float clip01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// samples/textured.py:16-26: (u, v) -> fractional (row, column) index
__device__ __forceinline__ void uv_to_index(float u, float v, int Ht, int Wt, bool clamp_mode, float& row, float& col, float& drow_dv,
                                            float& dcol_du)
{
    if (clamp_mode) {
        row = clip01(v) * (float)Ht;
        col = clip01(u) * (float)Wt;
        drow_dv = (v >= 0.f && v <= 1.f) ? (float)Ht : 0.f;   // the gradient of clip_by_value
        dcol_du = (u >= 0.f && u <= 1.f) ? (float)Wt : 0.f;
    } else {
        row = (v - floorf(v)) * (float)Ht;                    // uvs % 1. (floor-mod)
        col = (u - floorf(u)) * (float)Wt;
        drow_dv = (float)Ht; dcol_du = (float)Wt;
    }
}

// One texel / output pixel of CT channels as a register array, with the widest access its size and alignment allow
// (CT = 4: 16 bytes; 3: 12; 1: 4; 0: any count `ct`, channel by channel).
template <int CT>
__device__ __forceinline__ void load_ch(const float* __restrict__ p, int ct, float (&v)[CT ? CT : 1], int ch0 = 0)
{
    if constexpr (CT == 4) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else if constexpr (CT == 3) load3(p, v);
    else v[0] = p[ch0];
}
template <int CT>
__device__ __forceinline__ void store_ch(float* __restrict__ p, const float (&v)[CT ? CT : 1], int ch0 = 0)
{
    if constexpr (CT == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else if constexpr (CT == 3) store3(p, v);
    else p[ch0] = v[0];
}

// A float index -> texel index in [0, n - 1] as min(max((int)x, 0), n - 1), with a NaN index (a NaN coordinate) taking 0:
// converting a NaN to int is undefined in C++, so the rule is written out here instead of being left to the compiler
__device__ __forceinline__ int texel_index(float x, int n) { return x >= 1.f ? min((int)fminf(x, (float)n), n - 1) : 0; }

// The four texels of a bilinear look-up (samples/textured.py:36-60) and their weights
struct Taps {
    int r0, r1, c0, c1;
    float fr, fc, wr0, wc0;
};
__device__ __forceinline__ Taps bilinear_taps(float row, float col, int Ht, int Wt)
{
    Taps t;
    const float fr0 = floorf(row), fc0 = floorf(col);
    t.fr = row - fr0; t.fc = col - fc0;   // frac_indices[..., :1] (row), [..., 1:] (column)
    t.r0 = texel_index(fr0, Ht); t.r1 = min(t.r0 + 1, Ht - 1);
    t.c0 = texel_index(fc0, Wt); t.c1 = min(t.c0 + 1, Wt - 1);
    t.wc0 = 1.f - t.fc; t.wr0 = 1.f - t.fr;
    return t;
}

// The bilinear blend of four texels' values at the taps `k` (samples/textured.py:50-60), in the reference's order of operations.  (The
// four loads stay with the forward kernels: sampling through one function cost texture_forward_kernel<3> and <4> 2 us, 7 %.)
__device__ __forceinline__ float bilinear_blend(float tl, float tr, float bl, float br, const Taps& k)
{
    const float ta = (tl * k.wc0) * k.wr0, tb = (tr * k.fc) * k.wr0, tc = (bl * k.wc0) * k.fr, td = (br * k.fc) * k.fr;
    return ((ta + tb) + tc) + td;
}

// ---- what the trilinear look-ups share (dirt_texture_mip.hip; dirt_texture_cube.hip: a pyramid per cube face) ----
// the size of a dimension n0 at level k of a mip pyramid
__host__ __device__ __forceinline__ int mip_dim(int n0, int k) { const int d = n0 >> k; return d > 1 ? d : 1; }

// clamp to [0, L - 1] (NaN -> 0), split into level and fraction (spec 4 of dirt_texture_mip.hip)
__device__ __forceinline__ void mip_split(float lam, int L, int& l, float& f)
{
    const float top = (float)(L - 1);
    const float c = lam > 0.f ? (lam < top ? lam : top) : 0.f;
    const float fl = floorf(c);
    l = (int)fl; f = c - fl;
}

// the bilinear sample of one level [*, Wk, Ct]
template <int CT>
__device__ __forceinline__ void mip_sample(const float* __restrict__ lvl, int Wk, const Taps& k, int Ct, int ch, float (&o)[CT ? CT : 1])
{
    constexpr int NV = CT ? CT : 1;
    float a[NV], b[NV], c[NV], d[NV];
    load_ch<CT>(lvl + ((size_t)k.r0 * Wk + k.c0) * Ct, Ct, a, ch); load_ch<CT>(lvl + ((size_t)k.r0 * Wk + k.c1) * Ct, Ct, b, ch);
    load_ch<CT>(lvl + ((size_t)k.r1 * Wk + k.c0) * Ct, Ct, c, ch); load_ch<CT>(lvl + ((size_t)k.r1 * Wk + k.c1) * Ct, Ct, d, ch);
#pragma unroll
    for (int j = 0; j < NV; ++j) o[j] = bilinear_blend(a[j], b[j], c[j], d[j], k);
}

// ---- backward: a workgroup takes a tw x th tile of the pixel grid (16 x 16 of an image `cols` wide; 256 x 1 of a flat list).  The
// texels a tile's look-ups touch are a compact patch of the texture wherever (u, v) is smooth (a G-buffer: a rendered surface): the
// four products of every pixel are summed in an LDS copy of that patch (ds_add_f32) and each texel of the patch goes to memory ONCE,
// as one float atomic per channel, consecutive lanes on consecutive floats.  Scattering 4 Ct atomics per pixel straight at the texture,
// as the reference's gather_nd gradient does, is 64 same-address atomics per texel and channel at 16 pixels per texel, serialised by
// the memory system (2.8 ms for a 2048 x 2048 frame); tiles whose patch does not fit (a (u, v) seam, `repeat` wrapping) still do.
constexpr int TEX_PATCH = 1600;   // texels of a tile's patch (trilinear: of its two levels' patches) held in LDS (x Ct floats: 19 KB at 3 channels)

// lane `tid` of tile blockIdx.x -> the index i of its pixel in the rows x cols grid (of integer type I); false, and i = 0, outside it
template <class I> __device__ __forceinline__ bool tile_pixel(int tid, int tw, int th, int tiles_x, I rows, I cols, long long& i)
{
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const I px = (I)tile_x * tw + tid % tw, py = (I)tile_y * th + tid / tw;
    i = px < cols && py < rows ? (long long)py * cols + px : 0;
    return px < cols && py < rows;
}

// the bounding box (rmin, rmax, cmin, cmax) of tap sets, in LDS: empty, and grown by one set
__device__ __forceinline__ void box_clear(int* box) { box[0] = 0x7fffffff; box[1] = -1; box[2] = 0x7fffffff; box[3] = -1; }
__device__ __forceinline__ void box_add(int* box, const Taps k) { atomicMin(&box[0], k.r0); atomicMax(&box[1], k.r1); atomicMin(&box[2], k.c0); atomicMax(&box[3], k.c1); }

// grad_out of a pixel from channel c0 on, as registers: CT = 1, 3, 4: all CT channels; any count: four, zero from the nc-th on
template <int CT> __device__ __forceinline__ void load_grad_out(const float* __restrict__ gout, int Ct, int c0, int nc, float (&g)[CT ? CT : 4])
{
    if constexpr (CT != 0) load_ch<CT>(gout, Ct, g);
    else { for (int j = 0; j < 4; ++j) g[j] = j < nc ? gout[c0 + j] : 0.f; }
}

// The four texels of a tap set as offsets: of channel c0 in a level W texels wide; in the LDS patch (lct floats a texel) of the box at (rmin, cmin), bw wide
template <class T> struct Four { T tl, tr, bl, br; };
__device__ __forceinline__ Four<size_t> tap_offsets(const Taps k, int W, int Ct, int c0)
{
    return {((size_t)k.r0 * W + k.c0) * Ct + c0, ((size_t)k.r0 * W + k.c1) * Ct + c0, ((size_t)k.r1 * W + k.c0) * Ct + c0, ((size_t)k.r1 * W + k.c1) * Ct + c0};
}
__device__ __forceinline__ Four<int> patch_offsets(const Taps k, int rmin, int cmin, int bw, int lct)
{
    return {((k.r0 - rmin) * bw + (k.c0 - cmin)) * lct, ((k.r0 - rmin) * bw + (k.c1 - cmin)) * lct, ((k.r1 - rmin) * bw + (k.c0 - cmin)) * lct, ((k.r1 - rmin) * bw + (k.c1 - cmin)) * lct};
}

// g * d sample / d fr and g * d sample / d fc of one channel with the texels `t`
__device__ __forceinline__ void tap_gradients(float g, const Four<float>& t, const Taps k, float& e_fr, float& e_fc)
{
    e_fr = g * ((t.bl - t.tl) * k.wc0 + (t.br - t.tr) * k.fc);
    e_fc = g * ((t.tr - t.tl) * k.wr0 + (t.br - t.bl) * k.fr);
}

// g times a tap set's four weights, added to channel j at its four offsets of `dst`: the LDS patch, or the gradient in memory
template <class T> __device__ __forceinline__ void add_taps(float* dst, const Four<T>& o, int j, float g, const Four<float>& w)
{
    atomicAdd(&dst[o.tl + j], g * w.tl); atomicAdd(&dst[o.tr + j], g * w.tr); atomicAdd(&dst[o.bl + j], g * w.bl); atomicAdd(&dst[o.br + j], g * w.br);
}

__device__ __forceinline__ void clear_patch(float* s_acc, int n, int tid) { for (int e = tid; e < n; e += 256) s_acc[e] = 0.f; }

// Texel t of the patch of the box with top-left (rmin, cmin) and width bw -> its offset in a level W texels wide.  The flush loop
// stays in each kernel: handed this mapping as a function, the trilinear kernel (one of two boxes) kept its boxes in 4 KB of LDS.
__device__ __forceinline__ size_t box_texel(int t, int rmin, int cmin, int bw, int W, int Ct)
{
    const int pr = t / bw, pc = t - pr * bw;
    return ((size_t)(rmin + pr) * W + (cmin + pc)) * Ct;
}

// ---- host: the pixel grid.  rows x cols must not overflow; its tiles of 256 pixels are 16 x 16 of an image, 256 x 1 of a flat list (rows == 1)
inline int check_pixel_grid(const char* who, long long rows, long long cols)
{
    if (rows < 0 || cols < 0 || (rows > 0 && cols > 0x7fffffffffffffffll / rows)) TEX_FAIL("%s: bad pixel grid (rows=%lld cols=%lld)", who, rows, cols);
    return DIRT_OK;
}
struct TileGrid { int tw, th; long long tiles_x, tiles; };
inline TileGrid tile_grid(long long rows, long long cols)
{
    const int tw = rows > 1 ? 16 : 256, th = rows > 1 ? 16 : 1;
    return {tw, th, (cols + tw - 1) / tw, ((cols + tw - 1) / tw) * ((rows + th - 1) / th)};
}

// ---- batched launches (a texture per scene).  Scene b's texture, pyramid, coordinates, outputs and gradients start b per-scene extents
// after scene 0's, the scene is gridDim.y, and blockIdx.x / gridDim.x mean what they mean in a single-texture launch: a tile or a
// grid-stride loop never sees look-ups of two scenes.  A kernel's BATCH instantiation moves its base pointers to its scene's data once
// (workgroup-uniform, in size_t), before the per-look-up code, which is the single-texture kernel's; a pointer that is missing stays so.
// Host: an entry point and its batched form are one function that takes a `Scenes`; it checks the count of a batch with check_scenes and
// launches through dispatch_scenes on scene_grid, so each kernel's two instantiations share one launch statement.
constexpr long long TEX_MAX_SCENES = 65535;   // gridDim.y
template <class T> __device__ __forceinline__ void scene_shift(T*& p, size_t floats) { if (p) p += floats; }

// host: what a call works on -- one texture (`count` 1), or a batch of `count` of them (the caller's number, for check_scenes to judge)
struct Scenes { bool batch; long long count; bool none() const { return batch && count == 0; } };   // none(): a batch of zero scenes
constexpr Scenes ONE_TEXTURE{false, 1};
inline dim3 scene_grid(unsigned blocks, Scenes s) { return s.batch ? dim3(blocks, (unsigned)s.count) : dim3(blocks); }
// f(std::false_type) for a single texture, f(std::true_type) for a batch: a kernel's BATCH argument, as dispatch_channels hands over CT
template <class F> inline void dispatch_scenes(Scenes s, F&& f) { if (!s.batch) f(std::false_type{}); else f(std::true_type{}); }

// the scene count of a batched entry point and its per-scene extents in floats, each a count x a stride (both >= 0)
struct SceneExtent { long long count, stride; };
inline int check_scenes(const char* who, long long scenes, std::initializer_list<SceneExtent> extents)
{
    if (scenes < 0) TEX_FAIL("%s: bad scene count (scenes=%lld)", who, scenes);
    for (const SceneExtent& e : extents) {
        long long t;
        if (__builtin_mul_overflow(e.count, e.stride, &t) || __builtin_mul_overflow(t, scenes, &t))
            TEX_FAIL("%s: %lld scenes of %lld x %lld floats overflow", who, scenes, e.count, e.stride);
    }
    if (scenes > TEX_MAX_SCENES) TEX_FAIL("%s: %lld scenes, one launch addresses at most %lld", who, scenes, TEX_MAX_SCENES);
    return DIRT_OK;
}

// ---- p[0 .. n) = 0 on `stream`: how the backward entry points clear the buffer their kernels add into.  A kernel of the
// library's own, NOT hipMemsetAsync: captured in a graph (hipGraph, torch.cuda.graph), the runtime's memset node cleared the
// buffer on the first replay only -- from the second replay on, one float in four came back holding the float count
// (tests/test_texture_edges.py::test_a_captured_lookup_and_backward_replay_on_new_textures).  The floats before the first
// 16-byte boundary (`head`, < 4) and after the last one are stored one by one, the rest as float4.
static __global__ __launch_bounds__(256) void clear_floats_kernel(float* __restrict__ p, long long n, int head)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x, lanes = (long long)gridDim.x * 256;
    const long long quads = (n - head) / 4, tail = head + quads * 4;
    float4* __restrict__ q = reinterpret_cast<float4*>(p + head);
    for (long long i = lane; i < quads; i += lanes) q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < head) p[lane] = 0.f;
    if (lane < n - tail) p[tail + lane] = 0.f;
}

inline hipError_t clear_floats(float* p, long long n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const long long to_boundary = (4 - (long long)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3;
    const int head = (int)(to_boundary < n ? to_boundary : n);
    const long long quads = (n - head) / 4;
    hipLaunchKernelGGL(clear_floats_kernel, dim3(capped_blocks(quads > 0 ? quads : 1)), dim3(256), 0, stream, p, n, head);
    return hipGetLastError();
}

}  // namespace dirt
