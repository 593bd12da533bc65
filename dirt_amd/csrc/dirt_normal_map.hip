// dirt_normal_map.hip -- tangent-space normal mapping of a G-buffer, fused: one pass forward, one backward.
//
// The pixel side of normal mapping (the vertex side is dirt_tangent.hip): a pixel's interpolated normal and tangent frame and
// a normal-map texel become its shading normal, written into a copy of the G-buffer that the shaders of dirt_shade*.hip take
// with the same channel indices.  The specification (DESIGN.md §7g restates it; dirt_amd/lighting.py::perturb_normals is
// its readable form, which tests/normal_map_reference.py restates in float64), per pixel with normal n, tangent t,
// handedness w and texel m:
//
//     d = 2 m - 1 (DIRT_NORMAL_MAP_ENCODED) or m;   d.xy *= strength
//     N = n / |n|       x = t - N (N . t),  T = x / |x|       Bv = w (N x T)
//     y = (d.x T + d.y Bv) + d.z N          out = y / |y|
//
//  where n . n > 0, x . x > 0 and y . y > 0; any other pixel (a background's zero normal, a zero tangent, a tangent parallel to
//  the normal, a zero decoded vector) keeps its normal and hands the incoming gradient to it alone.  Gradients, with
//  g = d loss / d out:
//
//     gy = (g - out (out . g)) / |y|       d d = (gy . T, gy . Bv, gy . N)      gC = w d.y gy      d w = d.y gy . (N x T)
//     gT = d.x gy + gC x N                 gx = (gT - T (T . gT)) / |x|         d t = gx - N (N . gx)
//     gN = d.z gy + T x gC - ((N . t) gx + t (N . gx))                          d n = (gN - N (N . gN)) / |n|
//     d m = (strength, strength, 1) d d, doubled when encoded
//
// Kernels: normal_map_forward_kernel, normal_map_backward_kernel; NM_ITER passes of NM_BLOCK pixels per workgroup
// (dirt_shade_common.h holds the tile walk and the attribute check this file shares with the shaders).  A lane computes one
// pixel from its seven channels and its texel and leaves the result in LDS; then the workgroup walks the pass's
// NM_BLOCK * Cg floats in order, lane after lane, taking each from the source row (the G-buffer forward, grad_out backward)
// or from LDS: every row is read and written whole, whatever Cg.  d normal_map is dense, one 12-byte store per lane.  There
// are no parameter sums: no reduction, no scratch, no atomics.  `encoded` and the two outputs of the backward are
// wave-uniform branches, not template arguments: the kernels are bound by their memory traffic, not by registers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"

namespace dirt {

constexpr int NM_BLOCK = 256;      // lanes of a workgroup, pixels of one of its passes
constexpr int NM_ITER = 4;         // passes of a workgroup
constexpr int NM_ROW = 7;          // floats of a pixel's row in the backward's LDS tile: dn[3], dt[3], dw (odd: no bank conflicts)
constexpr int NM_PASS = 255;       // in the channel map: the channel passes through

struct NormalMapParams {
    const float* g;        // [n, Cg]
    const float* map;      // a pixel's texel: three floats, mstride apart
    float* out;            // [n, Cg]
    const float* gout;     // [n, Cg]
    float* gg;             // [n, Cg] or nullptr
    float* gmap;           // [n, 3] or nullptr
    long long n;           // pixels of all scenes
    int Cg, mstride, on, ot;
    int encoded;
    float strength;
};

struct NmPixel {
    float n[3], t[3], w, d[3];
    float N[3], T[3], C[3], y[3], o[3];
    float ln, lx, ly, s;
    bool valid;
};

// v / |v| with a denominator of 1 at v = 0; returns whether v . v > 0
__device__ __forceinline__ bool guarded_unit(const float (&v)[3], float (&u)[3], float& len)
{
    const float vv = dot3(v, v);
    const bool ok = vv > 0.f;
    len = sqrtf(ok ? vv : 1.f);
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = v[j] / len;
    return ok;
}

// loads a pixel and builds its frame and its shading normal
__device__ __forceinline__ void nm_pixel(const NormalMapParams& P, long long pix, NmPixel& px)
{
    const float* __restrict__ row = P.g + pix * P.Cg;
    load3(row + P.on, px.n);
    const Float4 tw = *reinterpret_cast<const Float4*>(row + P.ot);
    px.t[0] = tw.x; px.t[1] = tw.y; px.t[2] = tw.z; px.w = tw.w;
    float m[3];
    load3(P.map + pix * P.mstride, m);
#pragma unroll
    for (int j = 0; j < 3; ++j) px.d[j] = P.encoded ? 2.f * m[j] - 1.f : m[j];
    px.d[0] *= P.strength; px.d[1] *= P.strength;
    const bool ok_n = guarded_unit(px.n, px.N, px.ln);
    px.s = dot3(px.N, px.t);
    float x[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = px.t[j] - px.N[j] * px.s;
    const bool ok_x = guarded_unit(x, px.T, px.lx);
    cross3(px.N, px.T, px.C);
#pragma unroll
    for (int j = 0; j < 3; ++j) px.y[j] = (px.d[0] * px.T[j] + px.d[1] * (px.w * px.C[j])) + px.d[2] * px.N[j];
    const bool ok_y = guarded_unit(px.y, px.o, px.ly);
    px.valid = ok_n && ok_x && ok_y;
}

// ---- forward: the G-buffer copied, its normal channels replaced
__global__ __launch_bounds__(NM_BLOCK) void normal_map_forward_kernel(NormalMapParams P)
{
    __shared__ float s_v[NM_BLOCK * 3];
    __shared__ unsigned char s_src[DIRT_SHADE_MAX_CHANNELS];
    const int tid = threadIdx.x, Cg = P.Cg;
    for (int ch = tid; ch < Cg; ch += NM_BLOCK) s_src[ch] = (unsigned char)((unsigned)(ch - P.on) < 3u ? ch - P.on : NM_PASS);
    const TileWalk wk = tile_walk<NM_BLOCK>(Cg, tid);
    for (int it = 0; it < NM_ITER; ++it) {
        const long long first = ((long long)blockIdx.x * NM_ITER + it) * NM_BLOCK;   // (uniform)
        if (first >= P.n) break;
        const int npx = (int)(P.n - first < NM_BLOCK ? P.n - first : NM_BLOCK);
        if (tid < npx) {
            NmPixel px;
            nm_pixel(P, first + tid, px);
#pragma unroll
            for (int j = 0; j < 3; ++j) s_v[tid * 3 + j] = px.valid ? px.o[j] : px.n[j];
        }
        __syncthreads();
        const float* __restrict__ src = P.g + first * Cg;
        float* __restrict__ dst = P.out + first * Cg;
        tile_for_each<NM_BLOCK>(npx, Cg, tid, wk, [&](int e, int pxi, int ch) {
            const int k = s_src[ch];
            const float through = src[e];
            dst[e] = k == NM_PASS ? through : s_v[pxi * 3 + k];
        });
        __syncthreads();
    }
}

// ---- backward: d gbuffer = grad_out with the normal channels replaced by d n and d t, d w added to the tangent channels
// (P.gg, or nothing); d normal_map (P.gmap, or nothing)
__global__ __launch_bounds__(NM_BLOCK) void normal_map_backward_kernel(NormalMapParams P)
{
    __shared__ float s_v[NM_BLOCK * NM_ROW];
    __shared__ unsigned char s_src[DIRT_SHADE_MAX_CHANNELS];
    const int tid = threadIdx.x, Cg = P.Cg;
    for (int ch = tid; ch < Cg; ch += NM_BLOCK)
        s_src[ch] = (unsigned char)((unsigned)(ch - P.on) < 3u ? ch - P.on : ((unsigned)(ch - P.ot) < 4u ? 3 + ch - P.ot : NM_PASS));
    const TileWalk wk = tile_walk<NM_BLOCK>(Cg, tid);
    for (int it = 0; it < NM_ITER; ++it) {
        const long long first = ((long long)blockIdx.x * NM_ITER + it) * NM_BLOCK;   // (uniform)
        if (first >= P.n) break;
        const int npx = (int)(P.n - first < NM_BLOCK ? P.n - first : NM_BLOCK);
        if (tid < npx) {
            const long long pix = first + tid;
            NmPixel px;
            nm_pixel(P, pix, px);
            float g[3];
            load3(P.gout + pix * Cg + P.on, g);
            float gn[3] = {g[0], g[1], g[2]}, gt[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f}, gw = 0.f;
            if (px.valid) {
                const float og = dot3(px.o, g);
                float gy[3], Bv[3], gC[3], gT[3], gN[3], gx[3], a[3], b[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) { gy[j] = (g[j] - px.o[j] * og) / px.ly; Bv[j] = px.w * px.C[j]; }
                gd[0] = dot3(gy, px.T); gd[1] = dot3(gy, Bv); gd[2] = dot3(gy, px.N);
                gw = px.d[1] * dot3(gy, px.C);
#pragma unroll
                for (int j = 0; j < 3; ++j) gC[j] = (px.w * px.d[1]) * gy[j];
                cross3(gC, px.N, a);     // C = N x T:  d T = gC x N,  d N = T x gC
                cross3(px.T, gC, b);
#pragma unroll
                for (int j = 0; j < 3; ++j) gT[j] = px.d[0] * gy[j] + a[j];
                const float tg = dot3(px.T, gT);
#pragma unroll
                for (int j = 0; j < 3; ++j) gx[j] = (gT[j] - px.T[j] * tg) / px.lx;
                const float ngx = dot3(px.N, gx);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    gt[j] = gx[j] - px.N[j] * ngx;
                    gN[j] = (px.d[2] * gy[j] + b[j]) - (px.s * gx[j] + px.t[j] * ngx);
                }
                const float nn = dot3(px.N, gN);
#pragma unroll
                for (int j = 0; j < 3; ++j) gn[j] = (gN[j] - px.N[j] * nn) / px.ln;
                gd[0] *= P.strength; gd[1] *= P.strength;
                if (P.encoded) { gd[0] *= 2.f; gd[1] *= 2.f; gd[2] *= 2.f; }
            }
            if (P.gmap) store3(P.gmap + pix * 3, gd);
            if (P.gg) {   // (uniform)
                float* __restrict__ r = s_v + tid * NM_ROW;
#pragma unroll
                for (int j = 0; j < 3; ++j) { r[j] = gn[j]; r[3 + j] = gt[j]; }
                r[6] = gw;
            }
        }
        if (!P.gg) continue;   // (uniform)
        __syncthreads();
        const float* __restrict__ src = P.gout + first * Cg;
        float* __restrict__ dst = P.gg + first * Cg;
        tile_for_each<NM_BLOCK>(npx, Cg, tid, wk, [&](int e, int pxi, int ch) {
            const int k = s_src[ch];
            const float through = src[e];
            const float mine = k == NM_PASS ? 0.f : s_v[pxi * NM_ROW + k];
            dst[e] = k == NM_PASS ? through : (k < 3 ? mine : through + mine);
        });
        __syncthreads();
    }
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

static int normal_map_check(const char* who, long long scenes, long long pixels, int Cg, int map_stride, int off_normals, int off_tangents,
                            unsigned flags, dirt::NormalMapParams& P)
{
    if (scenes < 0 || pixels < 0) STAGE_FAIL("%s: negative sizes (scenes=%lld pixels=%lld)", who, scenes, pixels);
    if (scenes > 65535) STAGE_FAIL("%s: %lld scenes, at most 65535", who, scenes);
    if (pixels > (1ll << 40) || scenes * pixels > (1ll << 40)) STAGE_FAIL("%s: %lld x %lld pixels, at most 2^40", who, scenes, pixels);
    if (Cg < 7 || Cg > DIRT_SHADE_MAX_CHANNELS) STAGE_FAIL("%s: %d G-buffer channels, 7..%d", who, Cg, DIRT_SHADE_MAX_CHANNELS);
    if (map_stride < 3) STAGE_FAIL("%s: map_stride=%d, a pixel's texel is 3 floats", who, map_stride);
    if (flags & ~DIRT_NORMAL_MAP_ENCODED) STAGE_FAIL("%s: unknown flags 0x%x", who, flags);
    const int off[2] = {off_normals, off_tangents}, width[2] = {3, 4};
    const bool absent[2] = {false, false};
    const char* const names[2] = {"normals", "tangents"};
    if (int rc = dirt::shade_check_attributes(who, Cg, 2, off, width, absent, names)) return rc;
    P.n = scenes * pixels; P.Cg = Cg; P.mstride = map_stride; P.on = off_normals; P.ot = off_tangents;
    P.encoded = (flags & DIRT_NORMAL_MAP_ENCODED) ? 1 : 0;
    return DIRT_OK;
}

int dirt_normal_map_forward(const float* gbuffer, const float* normal_map, float* out, long long scenes, long long pixels, int Cg, int map_stride,
                            int off_normals, int off_tangents, float strength, unsigned flags, void* stream)
{
    const char* who = "dirt_normal_map_forward";
    dirt::NormalMapParams P{};
    int rc = normal_map_check(who, scenes, pixels, Cg, map_stride, off_normals, off_tangents, flags, P);
    if (rc) return rc;
    if (P.n == 0) return dirt::stage_ok(report);
    if (!gbuffer || !normal_map || !out) STAGE_FAIL("%s: gbuffer / normal_map / out is NULL", who);
    P.g = gbuffer; P.map = normal_map; P.out = out; P.strength = strength;
    hipLaunchKernelGGL(dirt::normal_map_forward_kernel, dim3((unsigned)dirt::shade_blocks(P.n, dirt::NM_BLOCK * dirt::NM_ITER)), dim3(dirt::NM_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_normal_map_backward(const float* gbuffer, const float* normal_map, const float* grad_out, float* grad_gbuffer, float* grad_normal_map,
                             long long scenes, long long pixels, int Cg, int map_stride, int off_normals, int off_tangents, float strength,
                             unsigned flags, void* stream)
{
    const char* who = "dirt_normal_map_backward";
    dirt::NormalMapParams P{};
    int rc = normal_map_check(who, scenes, pixels, Cg, map_stride, off_normals, off_tangents, flags, P);
    if (rc) return rc;
    if (P.n == 0 || (!grad_gbuffer && !grad_normal_map)) return dirt::stage_ok(report);
    if (!gbuffer || !normal_map || !grad_out) STAGE_FAIL("%s: gbuffer / normal_map / grad_out is NULL", who);
    P.g = gbuffer; P.map = normal_map; P.gout = grad_out; P.gg = grad_gbuffer; P.gmap = grad_normal_map; P.strength = strength;
    hipLaunchKernelGGL(dirt::normal_map_backward_kernel, dim3((unsigned)dirt::shade_blocks(P.n, dirt::NM_BLOCK * dirt::NM_ITER)), dim3(dirt::NM_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

}  // extern "C"
