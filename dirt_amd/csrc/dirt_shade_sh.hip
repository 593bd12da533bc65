// dirt_shade_sh.hip -- second-order spherical-harmonic lighting of a G-buffer, fused: one pass forward, one backward.
//
// The light model differentiable face and body fitting uses: 9 coefficients per colour channel, image = albedo * sum_k L_k Y_k(n).
// The specification (DESIGN.md §7b restates it; dirt_amd/lighting.py::spherical_harmonics is its readable form, which
// tests/shade_sh_reference.py composes in float64), per pixel with colour c, normal n, mask m (1 without a mask channel):
//
//     nh = n                          (DIRT_SHADE_SH_NORMALIZE: n / max(|n|, 1e-12), torch.nn.functional.normalize)
//     E_j = sum_k s_band(k) L[k, j] Y_k(nh)           out_j = clamp(c_j E_j m + background_j (1 - m), lo, hi)
//
//  with the real basis in the order (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2):
//     Y0 = C0       Y1 = C1 y    Y2 = C1 z             Y3 = C1 x
//     Y4 = C2 x y   Y5 = C2 y z  Y6 = C3 (3 z^2 - 1)   Y7 = C2 x z   Y8 = C4 (x^2 - y^2)
//  Gradients are torch autograd's for that composition: the clamp passes the gradient at both edges (0 at a NaN), the norm of a
//  zero vector has gradient 0, and max(|n|, 1e-12) passes the gradient to |n| from 1e-12 up.
//
// The parameter block is [scenes or 1, 30] floats: L[k, j] at 3 k + j, then the background.  The three band scales, the clamp
// and the flag are launch arguments.
//
// Kernels: the tiling, the clamp and the host checks of dirt_shade_common.h.  Forward one pixel per lane; the colours are
// three floats `cstride` apart, which is three channels of the G-buffer (cstride = Cg) as well as an image of their own, so
// the forward is one kernel.  Backward four
// passes of 256 pixels per workgroup inside one scene: the forward again, d gbuffer through an LDS tile so that every row
// leaves whole, the colours' gradient of the tensor path by one 12-byte store per lane, the 30 parameter sums in registers,
// then wave_sum -> fold_waves_to_row -> one row per workgroup in caller scratch -> shade_launch_reduce in a fixed order.
// No atomics.  `normalize` is a wave-uniform branch, not a template argument: it adds a handful of registers to kernels whose
// occupancy the 30 sums set (DESIGN.md §7b has the table).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"

namespace dirt {

constexpr int SH_BLOCK = 256;      // lanes of a workgroup, pixels of one of its passes
constexpr int SH_ITER = 4;         // passes of a backward workgroup
constexpr int SH_SPAN = SH_BLOCK * SH_ITER;   // pixels of a backward workgroup
constexpr int SH_TERMS = 9;        // basis functions
constexpr int SH_PARAMS = DIRT_SHADE_SH_PARAMS;
constexpr int SH_ROW = 9;          // floats of a pixel's row in the LDS tile: dc[3], dn[3], dm, 0, and one of padding (odd: no bank conflicts)
constexpr int SH_ZERO = 7;         // the row's zero

constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f, SH_C2 = 1.0925484305920792f;
constexpr float SH_C3 = 0.31539156525252005f, SH_C4 = 0.5462742152960396f;

struct ShadeShParams {
    const float* g;        // [scenes, pixels, Cg]
    const float* col;      // a pixel's colour: three floats, cstride apart (g + off_colors with cstride = Cg, or the colour tensor)
    const float* prm;      // [scenes or 1, 30]
    float* out;            // [scenes, pixels, 3]
    const float* gout;     // [scenes, pixels, 3]
    float* gg;             // [scenes, pixels, Cg] or nullptr
    float* gcol;           // [scenes, pixels, 3] or nullptr (tensor path)
    float* partial;        // [scenes, blocks, 30] or nullptr
    long long pixels;      // of one scene
    int Cg, cstride, oc, on, om, pstride;   // channel offsets (oc: -1 on the tensor path; om: -1 = absent); pstride: 0 = one block for every scene
    int clamp, normalize;
    float lo, hi, s0, s1, s2;
};

struct ShPixel {
    float c[3], n[3], m;
    float h[3];            // the normal the basis sees
    float len, inv;        // |n|, 1 / max(|n|, 1e-12) (normalize only)
    float Y[SH_TERMS];     // the basis, band scale included
    float E[3];
};

// the band scale of term k
__device__ __forceinline__ float sh_scale(const ShadeShParams& P, int k) { return k == 0 ? P.s0 : (k < 4 ? P.s1 : P.s2); }

// loads a pixel and evaluates its irradiance
__device__ __forceinline__ void sh_pixel(const ShadeShParams& P, const float* __restrict__ prm, long long pix, ShPixel& px)
{
    const float* __restrict__ row = P.g + pix * P.Cg;
    load3(P.col + pix * P.cstride, px.c);
    load3(row + P.on, px.n);
    px.m = P.om >= 0 ? row[P.om] : 1.f;
    px.len = 0.f; px.inv = 1.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) px.h[j] = px.n[j];
    if (P.normalize) {   // (uniform)
        px.len = sqrtf(dot3(px.n, px.n));
        px.inv = 1.f / (px.len < 1.e-12f ? 1.e-12f : px.len);
#pragma unroll
        for (int j = 0; j < 3; ++j) px.h[j] = px.n[j] * px.inv;
    }
    const float x = px.h[0], y = px.h[1], z = px.h[2];
    px.Y[0] = P.s0 * SH_C0;
    px.Y[1] = P.s1 * (SH_C1 * y);
    px.Y[2] = P.s1 * (SH_C1 * z);
    px.Y[3] = P.s1 * (SH_C1 * x);
    px.Y[4] = P.s2 * (SH_C2 * (x * y));
    px.Y[5] = P.s2 * (SH_C2 * (y * z));
    px.Y[6] = P.s2 * (SH_C3 * (3.f * (z * z) - 1.f));
    px.Y[7] = P.s2 * (SH_C2 * (x * z));
    px.Y[8] = P.s2 * (SH_C4 * (x * x - y * y));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float e = prm[j] * px.Y[0];
#pragma unroll
        for (int k = 1; k < SH_TERMS; ++k) e += prm[3 * k + j] * px.Y[k];
        px.E[j] = e;
    }
}

// ---- forward: one pixel per lane; the 30 parameters are wave-uniform (scalar loads)
__global__ __launch_bounds__(SH_BLOCK) void shade_sh_forward_kernel(ShadeShParams P)
{
    const long long i = (long long)blockIdx.x * SH_BLOCK + threadIdx.x;
    if (i >= P.pixels) return;
    const long long pix = (long long)blockIdx.y * P.pixels + i;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    ShPixel px;
    sh_pixel(P, prm, pix, px);
    const float om = 1.f - px.m;
    float o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = clamp_out(P, (px.c[j] * px.E[j]) * px.m + prm[27 + j] * om);
    store3(P.out + pix * 3, o);
}

// which value of a pixel's LDS row goes to channel `ch` of d gbuffer; on the tensor path no channel is a colour (oc is -1
// there, which the range test would take for channels 0 and 1)
template <bool TENSOR>
__device__ __forceinline__ int shade_sh_source(const ShadeShParams& P, int ch)
{
    if constexpr (!TENSOR)
        if ((unsigned)(ch - P.oc) < 3u) return ch - P.oc;
    if ((unsigned)(ch - P.on) < 3u) return 3 + ch - P.on;
    if (ch == P.om) return 6;
    return SH_ZERO;
}

// ---- backward.  PARAMS: the parameter block wants its gradient; GBUF: the G-buffer does; TENSOR: the colours are a tensor
// of their own, whose gradient leaves by one store per lane where P.gcol is there (the tile's dc[3] stay unused).
template <bool PARAMS, bool GBUF, bool TENSOR>
__global__ __launch_bounds__(SH_BLOCK) void shade_sh_backward_kernel(ShadeShParams P)
{
    constexpr int NP = SH_PARAMS;
    constexpr int NA = PARAMS ? NP : 1;
    __shared__ float s_g[GBUF ? SH_BLOCK * SH_ROW : 1];
    __shared__ unsigned char s_src[GBUF ? DIRT_SHADE_MAX_CHANNELS : 1];
    __shared__ float s_part[PARAMS ? 4 * NP : 1];
    const int tid = threadIdx.x;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
    const int Cg = P.Cg;
    const TileWalk walk = tile_walk<SH_BLOCK>(Cg, tid);
    if constexpr (GBUF) {
        for (int ch = tid; ch < Cg; ch += SH_BLOCK) s_src[ch] = (unsigned char)shade_sh_source<TENSOR>(P, ch);
        s_g[tid * SH_ROW + SH_ZERO] = 0.f;
    }
    for (int it = 0; it < SH_ITER; ++it) {
        const long long first = ((long long)blockIdx.x * SH_ITER + it) * SH_BLOCK;   // (uniform)
        if (first >= P.pixels) break;
        const int npx = (int)(P.pixels - first < SH_BLOCK ? P.pixels - first : SH_BLOCK);
        const long long pix = (long long)blockIdx.y * P.pixels + first + tid;
        if (tid < npx) {
            ShPixel px;
            sh_pixel(P, prm, pix, px);
            float go[3];
            load3(P.gout + pix * 3, go);
            const float om = 1.f - px.m;
            float w[3], gc[3], gm = 0.f, gmb = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float lit = px.c[j] * px.E[j];
                const float pre = lit * px.m + prm[27 + j] * om;
                const float gpre = clamp_gate(P, pre, go[j]);
                const float glit = gpre * px.m;
                gm += gpre * lit;
                gmb += gpre * prm[27 + j];
                gc[j] = glit * px.E[j];
                w[j] = glit * px.c[j];
                if constexpr (PARAMS) {
                    acc[27 + j] += gpre * om;
#pragma unroll
                    for (int k = 0; k < SH_TERMS; ++k) acc[3 * k + j] += w[j] * px.Y[k];
                }
            }
            gm -= gmb;   // d (background (1 - m)) / d m
            // A_k = s_k sum_j w_j L[k, j]: what arrives at Y_k; then d nh = sum_k A_k grad Y_k
            float A[SH_TERMS];
#pragma unroll
            for (int k = 1; k < SH_TERMS; ++k)
                A[k] = sh_scale(P, k) * ((w[0] * prm[3 * k] + w[1] * prm[3 * k + 1]) + w[2] * prm[3 * k + 2]);
            const float x = px.h[0], y = px.h[1], z = px.h[2];
            float gh[3];
            gh[0] = (SH_C1 * A[3] + SH_C2 * (y * A[4] + z * A[7])) + (2.f * SH_C4) * (x * A[8]);
            gh[1] = (SH_C1 * A[1] + SH_C2 * (x * A[4] + z * A[5])) - (2.f * SH_C4) * (y * A[8]);
            gh[2] = (SH_C1 * A[2] + SH_C2 * (y * A[5] + x * A[7])) + (6.f * SH_C3) * (z * A[6]);
            float gn[3] = {gh[0], gh[1], gh[2]};
            if (P.normalize) {   // (uniform)  nh = n / den, den = max(|n|, 1e-12)
                const float gden = -(dot3(gh, px.n) * px.inv) * px.inv;
                const float glen = px.len >= 1.e-12f ? gden : 0.f;            // max passes the gradient at its edge
                const float gl = px.len == 0.f ? 0.f : glen / px.len;         // d |n| / d n = n / |n|, 0 at a zero vector
#pragma unroll
                for (int j = 0; j < 3; ++j) gn[j] = gh[j] * px.inv + px.n[j] * gl;
            }
            if constexpr (TENSOR)
                if (P.gcol) store3(P.gcol + pix * 3, gc);
            if constexpr (GBUF) {
                float* __restrict__ r = s_g + tid * SH_ROW;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if constexpr (!TENSOR) r[j] = gc[j];
                    r[3 + j] = gn[j];
                }
                r[6] = gm;
            }
        }
        if constexpr (GBUF)
            tile_rows_out<SH_BLOCK, SH_ROW>(s_g, s_src, P.gg + ((long long)blockIdx.y * P.pixels + first) * Cg, npx, Cg, tid, walk);
    }
    if constexpr (PARAMS) {
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const float s = wave_sum(acc[k]);
            if (lane == 0) s_part[wave * NP + k] = s;
        }
        __syncthreads();
        if (tid < NP) fold_waves_to_row<NP>(s_part, P.partial, tid);
    }
}

template <bool TENSOR>
static void shade_sh_launch_backward(const ShadeShParams& P, bool params, bool gbuf, dim3 grid, hipStream_t s)
{
    if (params && gbuf) hipLaunchKernelGGL((shade_sh_backward_kernel<true, true, TENSOR>), grid, dim3(SH_BLOCK), 0, s, P);
    else if (params) hipLaunchKernelGGL((shade_sh_backward_kernel<true, false, TENSOR>), grid, dim3(SH_BLOCK), 0, s, P);
    else if (gbuf) hipLaunchKernelGGL((shade_sh_backward_kernel<false, true, TENSOR>), grid, dim3(SH_BLOCK), 0, s, P);
    else if constexpr (TENSOR) hipLaunchKernelGGL((shade_sh_backward_kernel<false, false, true>), grid, dim3(SH_BLOCK), 0, s, P);
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

// what this file's entry points refuse (the shared refusals: dirt_shade_common.h); `colors`: whether the colours are a tensor of their own
static int shade_sh_check(const char* who, bool colors, long long scenes, long long pixels, int Cg, int color_stride, int off_colors,
                          int off_normals, int off_mask, int param_scenes, float s0, float s1, float s2, float lo, float hi, unsigned flags,
                          dirt::ShadeShParams& P)
{
    if (int rc = dirt::shade_check_sizes(who, scenes, pixels, Cg)) return rc;
    if (colors && color_stride < 3) STAGE_FAIL("%s: color_stride=%d, a pixel's colour is 3 floats", who, color_stride);
    if (param_scenes != 1 && param_scenes != scenes) STAGE_FAIL("%s: param_scenes=%d is neither 1 nor scenes=%lld", who, param_scenes, scenes);
    if (flags & ~(DIRT_SHADE_CLAMP | DIRT_SHADE_SH_NORMALIZE)) STAGE_FAIL("%s: unknown flags 0x%x", who, flags);
    // with a colour tensor the G-buffer has no colour channels (off_colors is not read): three channels of normals are the smallest one
    const int off[3] = {off_colors, off_normals, off_mask}, width[3] = {3, 3, 1};
    const bool absent[3] = {colors, false, off_mask == -1};
    const char* const names[3] = {"colors", "normals", "mask"};
    if (int rc = dirt::shade_check_attributes(who, Cg, 3, off, width, absent, names)) return rc;
    if (int rc = dirt::shade_check_clamp(who, flags, lo, hi)) return rc;
    P.pixels = pixels; P.Cg = Cg; P.oc = colors ? -1 : off_colors; P.on = off_normals; P.om = off_mask;
    P.cstride = colors ? color_stride : Cg;
    P.pstride = dirt::shade_pstride(param_scenes, DIRT_SHADE_SH_PARAMS);
    P.clamp = (flags & DIRT_SHADE_CLAMP) ? 1 : 0; P.normalize = (flags & DIRT_SHADE_SH_NORMALIZE) ? 1 : 0;
    P.lo = lo; P.hi = hi; P.s0 = s0; P.s1 = s1; P.s2 = s2;
    return DIRT_OK;
}

size_t dirt_shade_sh_scratch_bytes(long long scenes, long long pixels)
{
    return dirt::shade_scratch_bytes(scenes, pixels, dirt::SH_SPAN, DIRT_SHADE_SH_PARAMS);
}

int dirt_shade_sh_forward(const float* gbuffer, const float* colors, const float* params, float* out, long long scenes, long long pixels,
                          int Cg, int color_stride, int off_colors, int off_normals, int off_mask, int param_scenes, float scale0,
                          float scale1, float scale2, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_shade_sh_forward";
    dirt::ShadeShParams P{};
    int rc = shade_sh_check(who, colors != nullptr, scenes, pixels, Cg, color_stride, off_colors, off_normals, off_mask, param_scenes, scale0,
                            scale1, scale2, clamp_lo, clamp_hi, flags, P);
    if (rc) return rc;
    if (scenes * pixels == 0) return dirt::stage_ok(report);
    if (!gbuffer || !params || !out) STAGE_FAIL("%s: gbuffer / params / out is NULL", who);
    if (pixels > 0x7fffffffll * dirt::SH_BLOCK) STAGE_FAIL("%s: too many pixels per scene", who);
    P.g = gbuffer; P.col = colors ? colors : gbuffer + off_colors; P.prm = params; P.out = out;
    const dim3 grid((unsigned)((pixels + dirt::SH_BLOCK - 1) / dirt::SH_BLOCK), (unsigned)scenes);
    hipLaunchKernelGGL(dirt::shade_sh_forward_kernel, grid, dim3(dirt::SH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_shade_sh_backward(const float* gbuffer, const float* colors, const float* params, const float* grad_out, float* grad_gbuffer,
                           float* grad_colors, float* grad_params, void* scratch, size_t scratch_bytes, long long scenes, long long pixels,
                           int Cg, int color_stride, int off_colors, int off_normals, int off_mask, int param_scenes, float scale0,
                           float scale1, float scale2, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_shade_sh_backward";
    dirt::ShadeShParams P{};
    int rc = shade_sh_check(who, colors != nullptr, scenes, pixels, Cg, color_stride, off_colors, off_normals, off_mask, param_scenes, scale0,
                            scale1, scale2, clamp_lo, clamp_hi, flags, P);
    if (rc) return rc;
    if (grad_colors && !colors) STAGE_FAIL("%s: grad_colors without colors (the channel path's is part of grad_gbuffer)", who);
    if (scenes * pixels == 0 || (!grad_gbuffer && !grad_params && !grad_colors)) return dirt::stage_ok(report);
    if (!gbuffer || !params || !grad_out) STAGE_FAIL("%s: gbuffer / params / grad_out is NULL", who);
    if (grad_params) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_shade_sh_scratch_bytes(scenes, pixels), "dirt_shade_sh_scratch_bytes");
        if (rc) return rc;
    }
    const long long blocks = dirt::shade_blocks(pixels, dirt::SH_SPAN);
    if (blocks > 0x7fffffffll) STAGE_FAIL("%s: too many pixels per scene", who);
    P.g = gbuffer; P.col = colors ? colors : gbuffer + off_colors; P.prm = params; P.gout = grad_out; P.gg = grad_gbuffer; P.gcol = grad_colors;
    P.partial = static_cast<float*>(scratch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks, (unsigned)scenes);
    const bool params_wanted = grad_params != nullptr, gbuf = grad_gbuffer != nullptr;
    if (colors) dirt::shade_sh_launch_backward<true>(P, params_wanted, gbuf, grid, s);
    else dirt::shade_sh_launch_backward<false>(P, params_wanted, gbuf, grid, s);
    return dirt::shade_backward_finish(who, scratch, grad_params, scenes, blocks, DIRT_SHADE_SH_PARAMS, param_scenes, s);
}

}  // extern "C"
