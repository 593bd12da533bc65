// dirt_texture.hip -- texture look-up of a deferred shader as one kernel (and its gradient).
//
// Replaces the TensorFlow composition of the reference's samples/textured.py:16-61 -- `uvs_to_pixel_indices` (flip to
// (row, column), repeat / clamp, scale by the texture size) followed by `sample_texture` (floor, fraction, a 4 x gather_nd,
// bilinear blend; or nearest) -- which materialises the index tensor, the four gathered neighbour tensors and five
// products per pixel.  Here one thread reads a (u, v) pair straight out of the G-buffer (any element stride), gathers the
// four texels and writes the blended colour; the backward kernel scatters dL/dtexture with float atomics and writes
// dL/duv.  The arithmetic is the reference's, operation for operation in float32 (so the result equals the composed
// torch / TF expression bit for bit); where the reference's gather would read row Ht or column Wt -- an index inside the
// last texel -- the last texel is used.
// A texture per scene (dirt_texture_sample_batch_*): the same two kernels, instantiated with BATCH, take the scene from
// gridDim.y and move their base pointers to that scene's data before the per-look-up code (dirt_texture_common.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_texture_common.h"

namespace dirt {

struct TexParams {
    const float* texture;   // [Ht, Wt, Ct]
    const float* uvs;       // n pairs (u, v), `uv_stride` floats apart; (0, 0) is the TOP-LEFT of the image
    long long n;
    int Ht, Wt, Ct, uv_stride, guv_stride;
    unsigned flags;
    float* out;             // [n, Ct]
    const float* grad_out;  // [n, Ct]
    float* grad_texture;    // [Ht, Wt, Ct], accumulated into (cleared by the caller)
    float* grad_uvs;        // n pairs, `guv_stride` floats apart; or nullptr
};

// BATCH: `p` describes scene 0 of a batch and blockIdx.y is the scene (dirt_texture_common.h): its texture, look-ups, outputs and gradients
__device__ __forceinline__ void tex_scene(TexParams& p)
{
    const size_t b = blockIdx.y, texels = (size_t)p.Ht * p.Wt * p.Ct, n = (size_t)p.n;
    scene_shift(p.texture, b * texels); scene_shift(p.uvs, b * n * p.uv_stride); scene_shift(p.out, b * n * p.Ct);
    scene_shift(p.grad_out, b * n * p.Ct); scene_shift(p.grad_texture, b * texels); scene_shift(p.grad_uvs, b * n * p.guv_stride);
}

// ---- forward: one thread per pixel, CT channels per access ----
template <int CT, bool BATCH = false>
__global__ __launch_bounds__(256) void texture_forward_kernel(TexParams p)
{
    if constexpr (BATCH) tex_scene(p);
    const bool clamp_mode = (p.flags & DIRT_TEX_CLAMP) != 0, nearest = (p.flags & DIRT_TEX_NEAREST) != 0;
    const int Ct = CT ? CT : p.Ct;
    constexpr int NV = CT ? CT : 1;
    const bool uv_pairs = (p.uv_stride & 1) == 0 && (reinterpret_cast<uintptr_t>(p.uvs) & 7u) == 0;   // (u, v) as one 8-byte load
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (long long)gridDim.x * blockDim.x) {
        float u, v;
        if (uv_pairs) { const float2 q = *reinterpret_cast<const float2*>(p.uvs + i * p.uv_stride); u = q.x; v = q.y; }
        else { u = p.uvs[i * p.uv_stride]; v = p.uvs[i * p.uv_stride + 1]; }
        float row, col, drow_dv, dcol_du;
        uv_to_index(u, v, p.Ht, p.Wt, clamp_mode, row, col, drow_dv, dcol_du);
        float* __restrict__ out = p.out + i * Ct;
        if (nearest) {   // samples/textured.py:31-33: the indices truncated
            const int r = texel_index(row, p.Ht), c = texel_index(col, p.Wt);
            const float* __restrict__ t = p.texture + ((size_t)r * p.Wt + c) * Ct;
            for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) { float q[NV]; load_ch<CT>(t, Ct, q, ch); store_ch<CT>(out, q, ch); }
            continue;
        }
        const Taps k = bilinear_taps(row, col, p.Ht, p.Wt);
        const float* __restrict__ tl = p.texture + ((size_t)k.r0 * p.Wt + k.c0) * Ct, * __restrict__ tr = p.texture + ((size_t)k.r0 * p.Wt + k.c1) * Ct;
        const float* __restrict__ bl = p.texture + ((size_t)k.r1 * p.Wt + k.c0) * Ct, * __restrict__ br = p.texture + ((size_t)k.r1 * p.Wt + k.c1) * Ct;
        for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) {
            float a[NV], b[NV], c[NV], d[NV], o[NV];
            load_ch<CT>(tl, Ct, a, ch); load_ch<CT>(tr, Ct, b, ch); load_ch<CT>(bl, Ct, c, ch); load_ch<CT>(br, Ct, d, ch);
#pragma unroll
            for (int j = 0; j < NV; ++j) o[j] = bilinear_blend(a[j], b[j], c[j], d[j], k);
            store_ch<CT>(out, o, ch);
        }
    }
}

// ---- backward: the tile scheme of dirt_texture_common.h with one patch, the bounding box of the tile's taps
template <int CT, bool BATCH = false>
__global__ __launch_bounds__(256) void texture_backward_kernel(TexParams p, int rows, int cols, int tw, int th, int tiles_x)
{
    if constexpr (BATCH) tex_scene(p);
    constexpr int LCT = CT ? CT : 4;                 // channels per LDS patch pass (any count: passes of 4)
    __shared__ float s_acc[TEX_PATCH * LCT];
    __shared__ int s_box[4];                         // rmin, rmax, cmin, cmax of the tile's taps
    const bool clamp_mode = (p.flags & DIRT_TEX_CLAMP) != 0, nearest = (p.flags & DIRT_TEX_NEAREST) != 0;
    const int Ct = CT ? CT : p.Ct;
    const int tid = threadIdx.x;
    long long i;
    const bool active = tile_pixel(tid, tw, th, tiles_x, rows, cols, i);
    if (tid == 0) box_clear(s_box);
    float u = 0.f, v = 0.f;
    if (active) { u = p.uvs[i * p.uv_stride]; v = p.uvs[i * p.uv_stride + 1]; }
    float row, col, drow_dv, dcol_du;
    uv_to_index(u, v, p.Ht, p.Wt, clamp_mode, row, col, drow_dv, dcol_du);
    Taps k = bilinear_taps(row, col, p.Ht, p.Wt);
    if (nearest) {   // one tap, weight 1 (samples/textured.py:31-33: the indices truncated)
        k.r0 = k.r1 = texel_index(row, p.Ht); k.c0 = k.c1 = texel_index(col, p.Wt);
        k.fr = 0.f; k.fc = 0.f; k.wr0 = 1.f; k.wc0 = 1.f;
    }
    __syncthreads();
    if (active) box_add(s_box, k);
    __syncthreads();
    const int rmin = s_box[0], cmin = s_box[2];
    const int bh = s_box[1] - rmin + 1, bw = s_box[3] - cmin + 1;
    const bool patch = bh > 0 && bw > 0 && (long long)bh * bw <= TEX_PATCH;   // (workgroup-uniform)
    const Four<float> w = {k.wc0 * k.wr0, k.fc * k.wr0, k.wc0 * k.fr, k.fc * k.fr};
    float d_fr = 0.f, d_fc = 0.f;
    const float* __restrict__ gout = p.grad_out + i * Ct;
    for (int c0 = 0; c0 < Ct; c0 += LCT) {          // (CT = 1, 3, 4: one pass; any other count: passes of four channels)
        const int nc = CT ? CT : min(LCT, Ct - c0);
        if (patch) {
            clear_patch(s_acc, bh * bw * LCT, tid);
            __syncthreads();
        }
        if (active) {
            float g[LCT];
            load_grad_out<CT>(gout, Ct, c0, nc, g);
            // (tap_offsets written out: through the function, <4> came out with other registers and its autograd figure 0.1 % past the margin)
            const Four<size_t> o = {((size_t)k.r0 * p.Wt + k.c0) * Ct + c0, ((size_t)k.r0 * p.Wt + k.c1) * Ct + c0, ((size_t)k.r1 * p.Wt + k.c0) * Ct + c0, ((size_t)k.r1 * p.Wt + k.c1) * Ct + c0};
            const Four<int> l = patch_offsets(k, rmin, cmin, bw, LCT);
#pragma unroll
            for (int j = 0; j < LCT; ++j) {
                if (j >= nc) break;
                if (!nearest) {
                    float e_fr, e_fc;
                    tap_gradients(g[j], {p.texture[o.tl + j], p.texture[o.tr + j], p.texture[o.bl + j], p.texture[o.br + j]}, k, e_fr, e_fc);
                    d_fr += e_fr; d_fc += e_fc;
                }
                if (patch) {
                    if (nearest) { atomicAdd(&s_acc[l.tl + j], g[j]); continue; }
                    add_taps(s_acc, l, j, g[j], w);
                } else {
                    if (nearest) { atomicAdd(&p.grad_texture[o.tl + j], g[j]); continue; }
                    add_taps(p.grad_texture, o, j, g[j], w);
                }
            }
        }
        if (patch) {
            __syncthreads();
            // the patch to memory: entry e = (patch row, patch column, channel); consecutive lanes -> consecutive floats of a texture row
            for (int e = tid; e < bh * bw * LCT; e += 256) {
                const float val = s_acc[e];
                const int j = e % LCT, t = e / LCT;
                if (val != 0.f && j < nc) atomicAdd(&p.grad_texture[box_texel(t, rmin, cmin, bw, p.Wt, Ct) + c0 + j], val);
            }
            __syncthreads();
        }
    }
    if (active && p.grad_uvs) {   // floor() has zero gradient: d frac / d index = 1 (nearest: zero)
        p.grad_uvs[i * p.guv_stride] = nearest ? 0.f : d_fc * dcol_du;
        p.grad_uvs[i * p.guv_stride + 1] = nearest ? 0.f : d_fr * drow_dv;
    }
}

// (both launchers: a batch goes to the BATCH kernels with the scene in gridDim.y.  Four channels: every per-scene extent is a multiple of
// 16 bytes, so scene 0's alignment is every scene's.)
hipError_t launch_texture_forward(const TexParams& p, Scenes sc, hipStream_t stream)
{
    if (p.n == 0 || sc.none()) return hipSuccess;
    const bool a16 = (reinterpret_cast<uintptr_t>(p.texture) & 15u) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15u) == 0;
    dispatch_channels(p.Ct, a16, [&](auto ct) { dispatch_scenes(sc, [&](auto b) {
        hipLaunchKernelGGL((texture_forward_kernel<decltype(ct)::value, decltype(b)::value>), scene_grid(capped_blocks(p.n), sc), dim3(256), 0, stream, p);
    }); });
    return hipGetLastError();
}

// what a launch of the backward kernel can address: the tile index and the kernel's `rows` and `cols` are ints
inline bool tiles_fit(const TileGrid& t, long long rows, long long cols) { return t.tiles <= 0x7fffffffll && cols <= 0x7fffffffll && rows <= 0x7fffffffll; }

hipError_t launch_texture_backward(const TexParams& p, Scenes sc, long long rows, long long cols, hipStream_t stream)
{
    if (p.n == 0 || sc.none()) return hipSuccess;
    const TileGrid t = tile_grid(rows, cols);
    if (!tiles_fit(t, rows, cols)) return hipErrorInvalidValue;
    const bool a16 = (reinterpret_cast<uintptr_t>(p.grad_out) & 15u) == 0;
    dispatch_channels(p.Ct, a16, [&](auto ct) { dispatch_scenes(sc, [&](auto b) {
        hipLaunchKernelGGL((texture_backward_kernel<decltype(ct)::value, decltype(b)::value>), scene_grid((unsigned)t.tiles, sc), dim3(256), 0, stream, p, (int)rows,
                           (int)cols, t.tw, t.th, (int)t.tiles_x);
    }); });
    return hipGetLastError();
}

namespace {
thread_local char g_tex_error[256] = "";
}

// dirt_texture_last_error()'s text, for this file and dirt_texture_mip.hip
int set_texture_error(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    format_error(g_tex_error, sizeof(g_tex_error), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_texture_error;   // the error channel of this file's entry points

const char* dirt_texture_last_error(void) { return dirt::g_tex_error; }

static int tex_check(const char* who, const void* texture, const void* uvs, long long n, int Ht, int Wt, int Ct, int uv_stride)
{
    if (n < 0 || Ht <= 0 || Wt <= 0 || Ct <= 0 || uv_stride < 2)
        TEX_FAIL("%s: bad sizes (n=%lld Ht=%d Wt=%d Ct=%d uv_stride=%d)", who, n, Ht, Wt, Ct, uv_stride);
    if (n > 0 && (!texture || !uvs)) TEX_FAIL("%s: texture / uvs is NULL", who);
    return DIRT_OK;
}

// (every entry point below and its batched form are one function: a single texture, or `sc.count` of them, checked by check_scenes after
// the checks the two have in common, each scene's data a per-scene extent after the one before)

static int tex_forward(const char* who, dirt::Scenes sc, const float* texture, const float* uvs, float* out, long long n, int Ht, int Wt, int Ct,
                       int uv_stride, unsigned flags, void* stream)
{
    int rc = tex_check(who, texture, uvs, n, Ht, Wt, Ct, uv_stride);
    if (rc) return rc;
    if (n > 0 && !out) TEX_FAIL("%s: out is NULL", who);
    if (sc.batch && (rc = dirt::check_scenes(who, sc.count, {{(long long)Ht * Wt, Ct}, {n, uv_stride}, {n, Ct}}))) return rc;
    dirt::TexParams p{};
    p.texture = texture; p.uvs = uvs; p.n = n; p.Ht = Ht; p.Wt = Wt; p.Ct = Ct; p.uv_stride = uv_stride; p.flags = flags; p.out = out;
    return dirt::stage_hip(report, who, dirt::launch_texture_forward(p, sc, reinterpret_cast<hipStream_t>(stream)));
}

static int tex_backward(const char* who, dirt::Scenes sc, const float* texture, const float* uvs, const float* grad_out, float* grad_texture,
                        float* grad_uvs, long long rows, long long cols, int Ht, int Wt, int Ct, int uv_stride, int grad_uv_stride, unsigned flags,
                        void* stream)
{
    int rc = dirt::check_pixel_grid(who, rows, cols);
    if (!rc) rc = tex_check(who, texture, uvs, rows * cols, Ht, Wt, Ct, uv_stride);
    if (rc) return rc;
    const long long n = rows * cols;
    if (n > 0 && (!grad_out || !grad_texture)) TEX_FAIL("%s: grad_out / %s is NULL", who, sc.batch ? "grad_textures" : "grad_texture");
    if (grad_uvs && grad_uv_stride < 2) TEX_FAIL("%s: grad_uv_stride < 2", who);
    if (sc.batch && (rc = dirt::check_scenes(who, sc.count, {{(long long)Ht * Wt, Ct}, {n, uv_stride}, {n, Ct}, {n, grad_uvs ? grad_uv_stride : 0}}))) return rc;
    if (!grad_texture || sc.none()) return dirt::stage_ok(report);   // (n == 0 without a gradient buffer, or no scenes: nothing to clear, nothing to launch)
    // a pixel grid the kernel cannot address: a batch is refused here, before any device work; a single texture has its gradient cleared
    // and is then refused by the launcher (DIRT_E_HIP)
    if (sc.batch && !dirt::tiles_fit(dirt::tile_grid(rows, cols), rows, cols)) TEX_FAIL("%s: pixel grid too large (rows=%lld cols=%lld)", who, rows, cols);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = dirt::clear_floats(grad_texture, sc.count * ((long long)Ht * Wt * Ct), s);
    if (e == hipSuccess) {
        dirt::TexParams p{};
        p.texture = texture; p.uvs = uvs; p.n = n; p.Ht = Ht; p.Wt = Wt; p.Ct = Ct; p.uv_stride = uv_stride; p.guv_stride = grad_uv_stride;
        p.flags = flags; p.grad_out = grad_out; p.grad_texture = grad_texture; p.grad_uvs = grad_uvs;
        e = dirt::launch_texture_backward(p, sc, rows, cols, s);
    }
    return dirt::stage_hip(report, who, e);
}

int dirt_texture_sample_forward(const float* texture, const float* uvs, float* out, long long n, int Ht, int Wt, int Ct, int uv_stride,
                                unsigned flags, void* stream)
{
    return tex_forward("dirt_texture_sample_forward", dirt::ONE_TEXTURE, texture, uvs, out, n, Ht, Wt, Ct, uv_stride, flags, stream);
}

int dirt_texture_sample_backward_image(const float* texture, const float* uvs, const float* grad_out, float* grad_texture, float* grad_uvs,
                                       long long rows, long long cols, int Ht, int Wt, int Ct, int uv_stride, int grad_uv_stride, unsigned flags,
                                       void* stream)
{
    // (reports under the flat-list entry point's name, which forwards here)
    return tex_backward("dirt_texture_sample_backward", dirt::ONE_TEXTURE, texture, uvs, grad_out, grad_texture, grad_uvs, rows, cols, Ht, Wt, Ct, uv_stride,
                        grad_uv_stride, flags, stream);
}

int dirt_texture_sample_backward(const float* texture, const float* uvs, const float* grad_out, float* grad_texture, float* grad_uvs,
                                 long long n, int Ht, int Wt, int Ct, int uv_stride, int grad_uv_stride, unsigned flags, void* stream)
{
    // a flat list of n look-ups: one row of n pixels
    return dirt_texture_sample_backward_image(texture, uvs, grad_out, grad_texture, grad_uvs, 1, n, Ht, Wt, Ct, uv_stride, grad_uv_stride, flags, stream);
}

int dirt_texture_sample_batch_forward(const float* textures, const float* uvs, float* out, long long scenes, long long n, int Ht, int Wt, int Ct,
                                      int uv_stride, unsigned flags, void* stream)
{
    return tex_forward("dirt_texture_sample_batch_forward", {true, scenes}, textures, uvs, out, n, Ht, Wt, Ct, uv_stride, flags, stream);
}

int dirt_texture_sample_batch_backward_image(const float* textures, const float* uvs, const float* grad_out, float* grad_textures, float* grad_uvs,
                                             long long scenes, long long rows, long long cols, int Ht, int Wt, int Ct, int uv_stride,
                                             int grad_uv_stride, unsigned flags, void* stream)
{
    return tex_backward("dirt_texture_sample_batch_backward_image", {true, scenes}, textures, uvs, grad_out, grad_textures, grad_uvs, rows, cols, Ht, Wt,
                        Ct, uv_stride, grad_uv_stride, flags, stream);
}

}  // extern "C"
