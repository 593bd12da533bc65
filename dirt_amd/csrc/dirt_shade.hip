// dirt_shade.hip -- the lighting step of a deferred shader, fused: one pass over the G-buffer forward, one backward.
//
// Replaces the torch composition every deferred shader starts from (the reference's samples/deferred.py:59-98): ambient +
// the three reflectance models of dirt/lighting.py:175-344 evaluated per pixel, composited over a background colour through
// the mask channel and clamped.  The specification (DESIGN.md §7b restates it; tests/shade_reference.py composes it from
// dirt_amd/lighting.py in float64), per pixel with colour c, normal n, position p, mask m (1 without a mask channel):
//
//     lit = ambient * c + sum_i L_i(p, n, c)          out = clamp(lit * m + background * (1 - m), lo, hi)
//
//  L_i, with light vector d (a direction or a position), light colour k, and x = |cos| (double sided) or max(cos, 0):
//     diffuse_directional  (dirt/lighting.py:175-218): cos = n . (-d);                                    L = (k c) x
//     specular_directional (dirt/lighting.py:221-283): r = d + 2 (n . (-d)) n, t = camera - p,
//                                                      cos = (t / |t| + 1e-12) . r;                       L = (k c) pow(x, s)
//     diffuse_point        (dirt/lighting.py:286-344): e = p - d, cos = n . (e / (|e| + 1e-12));          L = (k c) x
//  Nothing is renormalised.  Gradients are those of this composition under torch's conventions at the kinks: max(x, 0) and
//  clamp pass the gradient at their edges, abs gives 0 at 0, pow(0, s) has gradient 0 to s and s pow(0, s - 1) to its base
//  (0 for s > 1, 1 at s = 1), a zero-length vector's norm has gradient 0.
//
// The parameter block the kernels read is [scenes or 1, 9 + 8 lights] floats: ambient, background, camera position, then
// per light {vector[3], colour[3], shininess, 0}.  Kind and sidedness of the lights are launch arguments.
//
// Kernels: the forward one pixel per lane.  The backward one pixel per lane, four pixels per lane in a row, on workgroups of
// 1024 pixels that never span two scenes: it recomputes the forward, sends d gbuffer through an LDS tile so that every row
// is written whole (zeros in the channels no attribute uses) with consecutive lanes on consecutive floats, and keeps the
// parameter gradients in registers; these are summed over the wave with DPP adds, over the four waves in LDS, and leave the
// workgroup as ONE row of partial sums in caller-owned scratch.  shade_reduce_kernel adds the rows in a fixed order: no
// atomics, and the same bits on every run.  The tile walk, the clamp, the host checks and the backward's epilogue are those of
// dirt_shade_common.h, shared with dirt_shade_sh.hip, dirt_shade_pbr.hip and dirt_normal_map.hip.
//
// ALBEDO: the colour comes from a second image, [scenes, pixels, >= 3 floats apart], instead of three channels of the G-buffer,
// and its gradient leaves as a second, dense image (dirt_shade_albedo_forward / _backward): the flag changes where px.c is
// loaded from and where gc[3] is stored, nothing after the load.  This file is two translation units of the parallel build:
// by itself the kernels and entry points of the channel path, and through dirt_shade_albedo.hip (which defines
// DIRT_SHADE_ALBEDO_UNIT and includes it) the ALBEDO = true instantiations and their two entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"

#ifdef DIRT_SHADE_ALBEDO_UNIT
#define SHADE_UNIT_ALBEDO true
#else
#define SHADE_UNIT_ALBEDO false
#endif

namespace dirt {

constexpr int SHADE_HEAD = DIRT_SHADE_PARAM_HEAD, SHADE_LIGHT = DIRT_SHADE_PARAM_LIGHT;
constexpr int SHADE_BLOCK = 256;      // lanes of a workgroup, pixels of one of its passes
constexpr int SHADE_ITER = 4;         // passes of a backward workgroup
constexpr int SHADE_SPAN = SHADE_BLOCK * SHADE_ITER;   // pixels of a backward workgroup
constexpr int SHADE_ROW = 11;         // floats of a pixel's row in the LDS tile: dc[3], dn[3], dp[3], dm, 0
constexpr int SHADE_ZERO = 10;        // the row's zero

struct ShadeParams {
    const float* g;        // [scenes, pixels, Cg]
    const float* prm;      // [scenes or 1, 9 + 8 nl]
    float* out;            // [scenes, pixels, 3]
    const float* gout;     // [scenes, pixels, 3]
    float* gg;             // [scenes, pixels, Cg] or nullptr
    float* partial;        // [scenes, blocks, 9 + 8 nl] or nullptr
    long long pixels;      // of one scene
    int Cg, oc, on, op, om, nl, pstride;   // channel offsets (op, om: -1 = absent); pstride: 0 = one block for every scene
    unsigned kinds, dsided;               // two bits / one bit per light
    int clamp;
    float lo, hi;
};

// what the ALBEDO kernels take: in a struct of its own, so that the argument segment of the channel path's kernels (and with it
// the offsets of their hidden arguments and the widths of their scalar loads) stays what it was
struct ShadeAlbedoParams : ShadeParams {
    const float* col;      // [scenes, pixels, cstride]: the first three floats of a pixel are its colour
    float* gcol;           // [scenes, pixels, 3] or nullptr
    int cstride;           // floats between consecutive pixels' colours, >= 3
};
template <bool ALBEDO> using ShadeArgs = std::conditional_t<ALBEDO, ShadeAlbedoParams, ShadeParams>;

__device__ __forceinline__ float fold_cos(float c, bool ds) { return ds ? fabsf(c) : (c < 0.f ? 0.f : c); }

// the geometry of one light at one pixel: the cosine, and what its gradient needs
struct LightGeo {
    float cosv;
    float a[3];    // specular: the reflected direction r;  point: the incident direction e / (|e| + 1e-12)
    float b[3];    // specular: v = t / |t| + 1e-12;        point: e
    float t[3];    // specular: t
    float ndl, len, inv;   // n . (-d); |t| or |e|; 1 / |t| or 1 / (|e| + 1e-12)
};

__device__ __forceinline__ void light_geometry(int kind, const float* __restrict__ L, const float (&cam)[3], const float (&n)[3],
                                               const float (&p)[3], LightGeo& q)
{
    const float d[3] = {L[0], L[1], L[2]};
    if (kind == DIRT_SHADE_DIFFUSE_DIRECTIONAL) {
        const float tl[3] = {-d[0], -d[1], -d[2]};
        q.cosv = dot3(n, tl);
    } else if (kind == DIRT_SHADE_SPECULAR_DIRECTIONAL) {
        const float tl[3] = {-d[0], -d[1], -d[2]};
        q.ndl = dot3(n, tl);
        const float k2 = 2.f * q.ndl;
#pragma unroll
        for (int j = 0; j < 3; ++j) { q.a[j] = d[j] + k2 * n[j]; q.t[j] = cam[j] - p[j]; }
        q.len = sqrtf(dot3(q.t, q.t));
        q.inv = 1.f / q.len;
#pragma unroll
        for (int j = 0; j < 3; ++j) q.b[j] = q.t[j] * q.inv + 1.e-12f;
        q.cosv = dot3(q.b, q.a);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) q.b[j] = p[j] - d[j];
        q.len = sqrtf(dot3(q.b, q.b));
        q.inv = 1.f / (q.len + 1.e-12f);
#pragma unroll
        for (int j = 0; j < 3; ++j) q.a[j] = q.b[j] * q.inv;
        q.cosv = dot3(n, q.a);
    }
}

// x or pow(x, s): the scalar factor of a light's term
__device__ __forceinline__ float light_factor(int kind, float x, float s) { return kind == DIRT_SHADE_SPECULAR_DIRECTIONAL ? powf(x, s) : x; }

struct Pixel { float c[3], n[3], p[3], m; };

template <bool ALBEDO>
__device__ __forceinline__ void load_pixel(const ShadeArgs<ALBEDO>& P, long long pix, Pixel& px)
{
    const float* __restrict__ row = P.g + pix * P.Cg;
    if constexpr (ALBEDO) load3(P.col + pix * P.cstride, px.c);
    else load3(row + P.oc, px.c);
    load3(row + P.on, px.n);
    px.p[0] = px.p[1] = px.p[2] = 0.f;
    if (P.op >= 0) load3(row + P.op, px.p);
    px.m = P.om >= 0 ? row[P.om] : 1.f;
}

// ---- forward: one pixel per lane; the lights are a wave-uniform loop over the parameter block (scalar loads)
template <bool ALBEDO = false>
__global__ __launch_bounds__(SHADE_BLOCK) void shade_forward_kernel(ShadeArgs<ALBEDO> P)
{
    const long long i = (long long)blockIdx.x * SHADE_BLOCK + threadIdx.x;
    if (i >= P.pixels) return;
    const long long pix = (long long)blockIdx.y * P.pixels + i;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    Pixel px;
    load_pixel<ALBEDO>(P, pix, px);
    const float cam[3] = {prm[6], prm[7], prm[8]};
    float lit[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) lit[j] = prm[j] * px.c[j];
    for (int l = 0; l < P.nl; ++l) {
        const float* __restrict__ L = prm + SHADE_HEAD + SHADE_LIGHT * l;
        const int kind = (P.kinds >> (2 * l)) & 3;
        LightGeo q;
        light_geometry(kind, L, cam, px.n, px.p, q);
        const float f = light_factor(kind, fold_cos(q.cosv, (P.dsided >> l) & 1), L[6]);
#pragma unroll
        for (int j = 0; j < 3; ++j) lit[j] += (L[3 + j] * px.c[j]) * f;
    }
    const float om = 1.f - px.m;
    const float o[3] = {clamp_out(P, lit[0] * px.m + prm[3] * om), clamp_out(P, lit[1] * px.m + prm[4] * om), clamp_out(P, lit[2] * px.m + prm[5] * om)};
    store3(P.out + pix * 3, o);
}

// which value of a pixel's LDS row goes to channel `ch` of d gbuffer; with ALBEDO no channel is a colour
// (oc is -1 there, which the range test below would take for channels 0 and 1)
template <bool ALBEDO>
__device__ __forceinline__ int shade_source(const ShadeParams& P, int ch)
{
    if constexpr (!ALBEDO)
        if ((unsigned)(ch - P.oc) < 3u) return ch - P.oc;
    if ((unsigned)(ch - P.on) < 3u) return 3 + ch - P.on;
    if (P.op >= 0 && (unsigned)(ch - P.op) < 3u) return 6 + ch - P.op;
    if (ch == P.om) return 9;
    return SHADE_ZERO;
}

// ---- backward.  NL: the number of lights (the per-lane parameter sums are registers, indexed at compile time);
// PARAMS: whether the parameter block wants its gradient; GBUF: whether the G-buffer does.  With ALBEDO the colours' gradient
// leaves by one store per lane (a wave's rows are contiguous) where P.gcol is there, and the tile's dc[3] stay unused.
template <int NL, bool PARAMS, bool GBUF, bool ALBEDO = false>
__global__ __launch_bounds__(SHADE_BLOCK) void shade_backward_kernel(ShadeArgs<ALBEDO> P)
{
    constexpr int NP = SHADE_HEAD + SHADE_LIGHT * NL;
    constexpr int NA = PARAMS ? NP : 1;
    __shared__ float s_g[GBUF ? SHADE_BLOCK * SHADE_ROW : 1];
    __shared__ unsigned char s_src[GBUF ? DIRT_SHADE_MAX_CHANNELS : 1];
    __shared__ float s_part[PARAMS ? 4 * NP : 1];
    const int tid = threadIdx.x;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    const float cam[3] = {prm[6], prm[7], prm[8]};
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
    const int Cg = P.Cg;
    const TileWalk walk = tile_walk<SHADE_BLOCK>(Cg, tid);
    if constexpr (GBUF) {
        for (int ch = tid; ch < Cg; ch += SHADE_BLOCK) s_src[ch] = (unsigned char)shade_source<ALBEDO>(P, ch);
        s_g[tid * SHADE_ROW + SHADE_ZERO] = 0.f;
    }
    for (int it = 0; it < SHADE_ITER; ++it) {
        const long long first = ((long long)blockIdx.x * SHADE_ITER + it) * SHADE_BLOCK;   // (uniform)
        if (first >= P.pixels) break;
        const int npx = (int)(P.pixels - first < SHADE_BLOCK ? P.pixels - first : SHADE_BLOCK);
        const long long pix = (long long)blockIdx.y * P.pixels + first + tid;
        if (tid < npx) {
            Pixel px;
            load_pixel<ALBEDO>(P, pix, px);
            float go[3];
            load3(P.gout + pix * 3, go);
            // the forward again: every light's cosine and factor, and the value the clamp saw
            float lit[3], cosv[NL ? NL : 1], fac[NL ? NL : 1];
#pragma unroll
            for (int j = 0; j < 3; ++j) lit[j] = prm[j] * px.c[j];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const float* __restrict__ L = prm + SHADE_HEAD + SHADE_LIGHT * l;
                const int kind = (P.kinds >> (2 * l)) & 3;
                LightGeo q;
                light_geometry(kind, L, cam, px.n, px.p, q);
                cosv[l] = q.cosv;
                fac[l] = light_factor(kind, fold_cos(q.cosv, (P.dsided >> l) & 1), L[6]);
#pragma unroll
                for (int j = 0; j < 3; ++j) lit[j] += (L[3 + j] * px.c[j]) * fac[l];
            }
            const float om = 1.f - px.m;
            float glit[3], gc[3], gn[3] = {0.f, 0.f, 0.f}, gp[3] = {0.f, 0.f, 0.f}, gm = 0.f, gmb = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float pre = lit[j] * px.m + prm[3 + j] * om;
                const float gpre = clamp_gate(P, pre, go[j]);
                glit[j] = gpre * px.m;
                gm += gpre * lit[j];
                gmb += gpre * prm[3 + j];
                if constexpr (PARAMS) { acc[3 + j] += gpre * om; acc[j] += glit[j] * px.c[j]; }
                gc[j] = glit[j] * prm[j];
            }
            gm -= gmb;   // d (background (1 - m)) / d m
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const float* __restrict__ L = prm + SHADE_HEAD + SHADE_LIGHT * l;
                const int kind = (P.kinds >> (2 * l)) & 3;
                const bool ds = (P.dsided >> l) & 1;
                const int a0 = SHADE_HEAD + SHADE_LIGHT * l;
                float gf = 0.f;   // to the scalar factor
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float t = glit[j] * fac[l];
                    if constexpr (PARAMS) acc[a0 + 3 + j] += t * px.c[j];
                    gc[j] += t * L[3 + j];
                    gf += glit[j] * (L[3 + j] * px.c[j]);
                }
                const float x = fold_cos(cosv[l], ds);
                float gx = gf;
                if (kind == DIRT_SHADE_SPECULAR_DIRECTIONAL) {
                    const float s = L[6];
                    gx = s == 0.f ? 0.f : gf * (s * powf(x, s - 1.f));
                    if constexpr (PARAMS) acc[a0 + 6] += (x == 0.f && s >= 0.f) ? 0.f : gf * (fac[l] * logf(x));
                }
                const float c0 = cosv[l];
                const float gcos = ds ? gx * ((c0 > 0.f ? 1.f : 0.f) - (c0 < 0.f ? 1.f : 0.f)) : (c0 >= 0.f ? gx : 0.f);
                LightGeo q;
                light_geometry(kind, L, cam, px.n, px.p, q);
                if (kind == DIRT_SHADE_DIFFUSE_DIRECTIONAL) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        gn[j] += gcos * -L[j];
                        if constexpr (PARAMS) acc[a0 + j] -= gcos * px.n[j];
                    }
                } else if (kind == DIRT_SHADE_SPECULAR_DIRECTIONAL) {
                    // cos = v . r;  v = t / |t| + 1e-12;  r = d + 2 (n . tl) n,  tl = -d
                    float gr[3], gv[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) { gr[j] = gcos * q.b[j]; gv[j] = gcos * q.a[j]; }
                    const float glen = -(dot3(gv, q.t) * q.inv) * q.inv;
                    const float gl = q.len == 0.f ? 0.f : glen * q.inv;            // d |t| / d t = t / |t|, 0 at a zero vector
                    const float gndl = 2.f * dot3(gr, px.n);
                    const float k2 = 2.f * q.ndl;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float gt = gv[j] * q.inv + q.t[j] * gl;
                        if constexpr (PARAMS) acc[6 + j] += gt;
                        gp[j] -= gt;
                        gn[j] += k2 * gr[j] + gndl * -L[j];
                        if constexpr (PARAMS) acc[a0 + j] += gr[j] - gndl * px.n[j];
                    }
                } else {
                    // cos = n . u;  u = e / (|e| + 1e-12);  e = p - d
                    float gu[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) { gn[j] += gcos * q.a[j]; gu[j] = gcos * px.n[j]; }
                    const float glen = -(dot3(gu, q.b) * q.inv) * q.inv;
                    const float gl = q.len == 0.f ? 0.f : glen / q.len;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float ge = gu[j] * q.inv + q.b[j] * gl;
                        gp[j] += ge;
                        if constexpr (PARAMS) acc[a0 + j] -= ge;
                    }
                }
            }
            if constexpr (ALBEDO)
                if (P.gcol) store3(P.gcol + pix * 3, gc);
            if constexpr (GBUF) {
                float* __restrict__ r = s_g + tid * SHADE_ROW;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if constexpr (!ALBEDO) r[j] = gc[j];
                    r[3 + j] = gn[j]; r[6 + j] = gp[j];
                }
                r[9] = gm;
            }
        }
        if constexpr (GBUF)
            tile_rows_out<SHADE_BLOCK, SHADE_ROW>(s_g, s_src, P.gg + ((long long)blockIdx.y * P.pixels + first) * Cg, npx, Cg, tid, walk);
    }
    if constexpr (PARAMS) {
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const bool pad = k >= SHADE_HEAD && (k - SHADE_HEAD) % SHADE_LIGHT == SHADE_LIGHT - 1;
            const float s = pad ? 0.f : wave_sum(acc[k]);
            if (lane == 0) s_part[wave * NP + k] = s;
        }
        __syncthreads();
        if (tid < NP) fold_waves_to_row<NP>(s_part, P.partial, tid);
    }
}

// ---- the rows of partial sums of one scene (or of all of them, for a block shared by the batch) added up in a fixed order:
// workgroup (k, b) sums value k (block_column_sum).  One copy for every unit (dirt_shade_common.h declares the launcher).
#ifndef DIRT_SHADE_ALBEDO_UNIT
__global__ __launch_bounds__(SHADE_BLOCK) void shade_reduce_kernel(const float* __restrict__ partial, float* __restrict__ grad_params,
                                                                   long long rows, int NP)
{
    __shared__ float s_sum[SHADE_BLOCK];
    const int k = blockIdx.x;
    const float total = block_column_sum<SHADE_BLOCK>(partial + (size_t)blockIdx.y * rows * NP + k, rows, NP, s_sum);
    if (threadIdx.x == 0) grad_params[(size_t)blockIdx.y * NP + k] = total;
}

void shade_launch_reduce(const float* partial, float* grad_params, long long rows, int NP, int param_scenes, hipStream_t s)
{
    hipLaunchKernelGGL(shade_reduce_kernel, dim3((unsigned)NP, (unsigned)param_scenes), dim3(SHADE_BLOCK), 0, s, partial, grad_params, rows, NP);
}
#endif

// (`params` and `gbuf` both false: the colours' gradient alone, an instantiation only ALBEDO has; the channel path is not called so)
template <int NL, bool ALBEDO>
void shade_launch_backward(const ShadeArgs<ALBEDO>& P, bool params, bool gbuf, dim3 grid, hipStream_t s)
{
    if (params && gbuf) hipLaunchKernelGGL((shade_backward_kernel<NL, true, true, ALBEDO>), grid, dim3(SHADE_BLOCK), 0, s, P);
    else if (params) hipLaunchKernelGGL((shade_backward_kernel<NL, true, false, ALBEDO>), grid, dim3(SHADE_BLOCK), 0, s, P);
    else if (gbuf || !ALBEDO) hipLaunchKernelGGL((shade_backward_kernel<NL, false, true, ALBEDO>), grid, dim3(SHADE_BLOCK), 0, s, P);
    else if constexpr (ALBEDO) hipLaunchKernelGGL((shade_backward_kernel<NL, false, false, true>), grid, dim3(SHADE_BLOCK), 0, s, P);
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

// What the entry points of this translation unit take their colours from: channels off_colors.. of the G-buffer, or (ALBEDO) the
// image `colors`, whose pixels are color_stride floats apart.  The checks and the launches below are written once for both;
// what differs is written out where it does.
static constexpr bool ALBEDO = SHADE_UNIT_ALBEDO;

static int shade_check(const char* who, long long scenes, long long pixels, int Cg, int off_colors, int color_stride, int off_normals,
                       int off_positions, int off_mask, int param_scenes, int lights, unsigned light_kinds, unsigned flags, float lo, float hi,
                       dirt::ShadeParams& P)
{
    if (int rc = dirt::shade_check_sizes(who, scenes, pixels, Cg)) return rc;
    if (ALBEDO && color_stride < 3) STAGE_FAIL("%s: color_stride=%d, a pixel's colour is 3 floats", who, color_stride);
    if (lights < 0 || lights > DIRT_SHADE_MAX_LIGHTS) STAGE_FAIL("%s: %d lights, at most %d", who, lights, DIRT_SHADE_MAX_LIGHTS);
    if (param_scenes != 1 && param_scenes != scenes) STAGE_FAIL("%s: param_scenes=%d is neither 1 nor scenes=%lld", who, param_scenes, scenes);
    // ALBEDO: the G-buffer has no colour channels (off_colors is -1), so three channels of normals are the smallest one
    const int off[4] = {off_colors, off_normals, off_positions, off_mask}, width[4] = {3, 3, 3, 1};
    const bool absent[4] = {ALBEDO, false, off_positions == -1, off_mask == -1};
    const char* const names[4] = {"colors", "normals", "positions", "mask"};
    if (int rc = dirt::shade_check_attributes(who, Cg, 4, off, width, absent, names)) return rc;
    for (int l = 0; l < lights; ++l) {
        const int kind = (light_kinds >> (2 * l)) & 3;
        if (kind > DIRT_SHADE_DIFFUSE_POINT) STAGE_FAIL("%s: light %d has unknown kind %d", who, l, kind);
        if (kind != DIRT_SHADE_DIFFUSE_DIRECTIONAL && off_positions < 0) STAGE_FAIL("%s: light %d needs positions, the G-buffer has none", who, l);
        if (kind == DIRT_SHADE_SPECULAR_DIRECTIONAL && !(flags & DIRT_SHADE_HAS_CAMERA))
            STAGE_FAIL("%s: light %d is specular and needs a camera position (DIRT_SHADE_HAS_CAMERA)", who, l);
    }
    if (int rc = dirt::shade_check_clamp(who, flags, lo, hi)) return rc;
    P.pixels = pixels; P.Cg = Cg; P.oc = ALBEDO ? -1 : off_colors; P.on = off_normals; P.op = off_positions; P.om = off_mask; P.nl = lights;
    P.pstride = dirt::shade_pstride(param_scenes, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights);
    P.kinds = light_kinds; P.clamp = (flags & DIRT_SHADE_CLAMP) ? 1 : 0; P.lo = lo; P.hi = hi;
    return DIRT_OK;
}

static void shade_set_colors(dirt::ShadeParams&, const float*, int, float*) {}   // the channel path has nothing to set
static void shade_set_colors(dirt::ShadeAlbedoParams& P, const float* colors, int color_stride, float* grad_colors)
{
    P.col = colors; P.cstride = color_stride; P.gcol = grad_colors;
}

// `colors`, `color_stride`: ALBEDO only (the channel path passes nullptr, 0); `off_colors`: the channel path only (ALBEDO passes -1)
static int shade_forward(const char* who, const float* gbuffer, const float* colors, const float* params, float* out, long long scenes,
                         long long pixels, int Cg, int off_colors, int color_stride, int off_normals, int off_positions, int off_mask,
                         int param_scenes, int lights, unsigned light_kinds, unsigned double_sided, float clamp_lo, float clamp_hi,
                         unsigned flags, void* stream)
{
    dirt::ShadeArgs<ALBEDO> P{};
    int rc = shade_check(who, scenes, pixels, Cg, off_colors, color_stride, off_normals, off_positions, off_mask, param_scenes, lights, light_kinds,
                         flags, clamp_lo, clamp_hi, P);
    if (rc) return rc;
    if (scenes * pixels == 0) return dirt::stage_ok(report);
    if (!gbuffer || !params || !out) STAGE_FAIL("%s: gbuffer / params / out is NULL", who);
    if (ALBEDO && !colors) STAGE_FAIL("%s: colors is NULL", who);
    if (pixels > 0x7fffffffll * dirt::SHADE_BLOCK) STAGE_FAIL("%s: too many pixels per scene", who);
    P.g = gbuffer; P.prm = params; P.out = out; P.dsided = double_sided;
    shade_set_colors(P, colors, color_stride, nullptr);
    const dim3 grid((unsigned)((pixels + dirt::SHADE_BLOCK - 1) / dirt::SHADE_BLOCK), (unsigned)scenes);
    hipLaunchKernelGGL(dirt::shade_forward_kernel<ALBEDO>, grid, dim3(dirt::SHADE_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

// `grad_colors`: ALBEDO only (the channel path passes nullptr: its colours' gradient is part of grad_gbuffer)
static int shade_backward(const char* who, const float* gbuffer, const float* colors, const float* params, const float* grad_out,
                          float* grad_gbuffer, float* grad_colors, float* grad_params, void* scratch, size_t scratch_bytes, long long scenes,
                          long long pixels, int Cg, int off_colors, int color_stride, int off_normals, int off_positions, int off_mask,
                          int param_scenes, int lights, unsigned light_kinds, unsigned double_sided, float clamp_lo, float clamp_hi,
                          unsigned flags, void* stream)
{
    dirt::ShadeArgs<ALBEDO> P{};
    int rc = shade_check(who, scenes, pixels, Cg, off_colors, color_stride, off_normals, off_positions, off_mask, param_scenes, lights, light_kinds,
                         flags, clamp_lo, clamp_hi, P);
    if (rc) return rc;
    if (scenes * pixels == 0 || (!grad_gbuffer && !grad_params && !grad_colors)) return dirt::stage_ok(report);
    if (!gbuffer || !params || !grad_out) STAGE_FAIL("%s: gbuffer / params / grad_out is NULL", who);
    if (ALBEDO && !colors) STAGE_FAIL("%s: colors is NULL", who);
    if (grad_params) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_shade_scratch_bytes(scenes, pixels, lights), "dirt_shade_scratch_bytes");
        if (rc) return rc;
    }
    const long long blocks = dirt::shade_blocks(pixels, dirt::SHADE_SPAN);
    if (blocks > 0x7fffffffll) STAGE_FAIL("%s: too many pixels per scene", who);
    P.g = gbuffer; P.prm = params; P.gout = grad_out; P.gg = grad_gbuffer; P.partial = static_cast<float*>(scratch); P.dsided = double_sided;
    shade_set_colors(P, colors, color_stride, grad_colors);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks, (unsigned)scenes);
    const bool params_wanted = grad_params != nullptr, gbuf = grad_gbuffer != nullptr;
    switch (lights) {
    case 0: dirt::shade_launch_backward<0, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    case 1: dirt::shade_launch_backward<1, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    case 2: dirt::shade_launch_backward<2, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    case 3: dirt::shade_launch_backward<3, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    case 4: dirt::shade_launch_backward<4, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    case 5: dirt::shade_launch_backward<5, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    case 6: dirt::shade_launch_backward<6, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    case 7: dirt::shade_launch_backward<7, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    default: dirt::shade_launch_backward<8, ALBEDO>(P, params_wanted, gbuf, grid, s); break;
    }
    return dirt::shade_backward_finish(who, scratch, grad_params, scenes, blocks, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights, param_scenes, s);
}

#ifndef DIRT_SHADE_ALBEDO_UNIT

size_t dirt_shade_scratch_bytes(long long scenes, long long pixels, int lights)
{
    if (lights < 0 || lights > DIRT_SHADE_MAX_LIGHTS) return 0;
    return dirt::shade_scratch_bytes(scenes, pixels, dirt::SHADE_SPAN, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights);
}

int dirt_shade_forward(const float* gbuffer, const float* params, float* out, long long scenes, long long pixels, int Cg, int off_colors,
                       int off_normals, int off_positions, int off_mask, int param_scenes, int lights, unsigned light_kinds,
                       unsigned double_sided, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    return shade_forward("dirt_shade_forward", gbuffer, nullptr, params, out, scenes, pixels, Cg, off_colors, 0, off_normals, off_positions, off_mask,
                         param_scenes, lights, light_kinds, double_sided, clamp_lo, clamp_hi, flags, stream);
}

int dirt_shade_backward(const float* gbuffer, const float* params, const float* grad_out, float* grad_gbuffer, float* grad_params,
                        void* scratch, size_t scratch_bytes, long long scenes, long long pixels, int Cg, int off_colors, int off_normals,
                        int off_positions, int off_mask, int param_scenes, int lights, unsigned light_kinds, unsigned double_sided,
                        float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    return shade_backward("dirt_shade_backward", gbuffer, nullptr, params, grad_out, grad_gbuffer, nullptr, grad_params, scratch, scratch_bytes,
                          scenes, pixels, Cg, off_colors, 0, off_normals, off_positions, off_mask, param_scenes, lights, light_kinds, double_sided,
                          clamp_lo, clamp_hi, flags, stream);
}

#else

int dirt_shade_albedo_forward(const float* gbuffer, const float* colors, const float* params, float* out, long long scenes, long long pixels,
                              int Cg, int color_stride, int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                              unsigned light_kinds, unsigned double_sided, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    return shade_forward("dirt_shade_albedo_forward", gbuffer, colors, params, out, scenes, pixels, Cg, -1, color_stride, off_normals, off_positions,
                         off_mask, param_scenes, lights, light_kinds, double_sided, clamp_lo, clamp_hi, flags, stream);
}

int dirt_shade_albedo_backward(const float* gbuffer, const float* colors, const float* params, const float* grad_out, float* grad_gbuffer,
                               float* grad_colors, float* grad_params, void* scratch, size_t scratch_bytes, long long scenes, long long pixels,
                               int Cg, int color_stride, int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                               unsigned light_kinds, unsigned double_sided, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    return shade_backward("dirt_shade_albedo_backward", gbuffer, colors, params, grad_out, grad_gbuffer, grad_colors, grad_params, scratch,
                          scratch_bytes, scenes, pixels, Cg, -1, color_stride, off_normals, off_positions, off_mask, param_scenes, lights, light_kinds,
                          double_sided, clamp_lo, clamp_hi, flags, stream);
}

#endif

}  // extern "C"
