// dirt_shade_pbr.hip -- Cook-Torrance (metallic-roughness) lighting of a G-buffer, fused: one pass forward, one backward.
//
// The material model of inverse rendering: albedo, roughness and metalness per pixel, GGX distribution, Smith-Schlick
// visibility, Schlick Fresnel, up to four directional or point lights.  The specification (DESIGN.md §7b restates it;
// dirt_amd/lighting.py::cook_torrance is its readable form, which tests/shade_pbr_reference.py composes in float64), per
// pixel with albedo c, normal n, position p, roughness r, metalness mu, mask m (1 without a mask channel):
//
//     N = n / max(|n|, 1e-12)               v = normalize(cam - p)          (torch.nn.functional.normalize, eps 1e-12, everywhere)
//     rho = clamp(r, min_roughness, 1)      a2 = (rho^2)^2                  k = (rho + 1)^2 / 8
//     F0_j = dielectric_f0 (1 - mu) + c_j mu                                nv = max(N . v, 0)
//     per light:  l = normalize(-d_i) (directional)  |  normalize(d_i - p) (point)
//                 h = normalize(l + v)      nl = max(N . l, 0)   nh = max(N . h, 0)   vh = max(v . h, 0)
//                 D   = a2 / (pi den^2),  den = |N x h|^2 + a2 nh^2
//                 Vis = 0.25 / ((nl (1 - k) + k) (nv (1 - k) + k))
//                 w = 1 - vh,  F_j = F0_j + (1 - F0_j) ((w w)(w w) w)       kd_j = (1 - F_j)(1 - mu)
//                 L_i,j = (kd_j c_j / pi + D Vis F_j) k_i,j nl          with a visibility s_i (below):  ... ((k_i,j nl) s_i)
//     out_j = clamp((ambient_j c_j + sum_i L_i,j) m + background_j (1 - m), lo, hi)
//
//  Gradients are torch autograd's for that composition: max(x, 0) and the clamps pass the gradient at their edges, the norm
//  of a zero vector has gradient 0, and max(|x|, 1e-12) passes the gradient to |x| from 1e-12 up.
//
// Visibility (VIS; dirt_shade_pbr_visibility_forward / _backward): one factor s_i per light and pixel, the output of
// dirt_shadow_forward, scales the light's weight: (k_i,j nl) s_i, one more float32 multiplication of a value the kernel has,
// nothing reordered -- s = 1 gives the bits of the kernels without it.  s is not clamped (a NaN, an inf or a value outside
// [0, 1] behaves as IEEE says), the ambient term is not shadowed.  With gknl_j = glit_j B_j:  d s_i = sum_j gknl_j (k_i,j nl);
// the colour's and nl's gradients take gknl_j s_i for gknl_j; gB_j = glit_j ((k_i,j nl) s_i).
//
// The parameter block is [scenes or 1, 9 + 8 lights] floats in the layout of dirt_shade.hip's: ambient, background, camera,
// then per light {vector[3], colour[3], 0, 0}.  The light kinds (one bit per light), the two scalars of the material model,
// the clamp and the flag are launch arguments.
//
// Kernels: the tiling, the clamp and, with dirt_shade_ibl.hip, a pixel's material (MaterialPixel), the channel map and the host
// checks of dirt_shade_common.h.  Forward one pixel per lane; a pixel's colours are three floats and its material two floats
// `cstride` / `mstride` apart, which is channels of the G-buffer (stride Cg) as well as a tensor of their own, so
// the forward is one kernel for the four source combinations.  Backward four passes of 256 pixels per workgroup inside one
// scene: the forward again, d gbuffer through an LDS tile so that every row leaves whole, the tensors' gradients by one dense
// store per lane, the parameter sums in registers under compile-time indices (hence the template on the light count), then
// wave_sum -> fold_waves_to_row -> one row per workgroup in caller scratch -> shade_launch_reduce in a fixed order.  No atomics.
// VIS is a compile-time parameter of the kernels, one value per translation unit (PBR_VIS): a pixel's factors are `lights`
// consecutive floats, `vstride` apart from pixel to pixel, read in place; d visibility leaves dense, [scenes, pixels, lights],
// by a store per lane and light where P.gvis is there.  This file is two translation units of the parallel build: by itself
// the kernels and entry points without a visibility, and through dirt_shade_pbr_visibility.hip (which defines
// DIRT_SHADE_PBR_VISIBILITY_UNIT, includes it and holds the two entry points) the VIS = true kernels, lights 1..4, under names
// of their own.  (As one templated body behind two sets of __global__ wrappers the kernels without VIS took other registers.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"

namespace dirt {

constexpr int PBR_BLOCK = 256;     // lanes of a workgroup, pixels of one of its passes
constexpr int PBR_ITER = 4;        // passes of a backward workgroup
constexpr int PBR_SPAN = PBR_BLOCK * PBR_ITER;   // pixels of a backward workgroup
constexpr int PBR_HEAD = DIRT_SHADE_PARAM_HEAD, PBR_LIGHT = DIRT_SHADE_PARAM_LIGHT;
constexpr float PBR_PI = 3.14159265358979323846f, PBR_INV_PI = 0.31830988618379067154f;

struct ShadePbrParams {
    const float* g;        // [scenes, pixels, Cg]
    const float* col;      // a pixel's colour: three floats, cstride apart (g + off_colors with cstride = Cg, or the colour tensor)
    const float* mat;      // a pixel's roughness and metalness: two floats, mstride apart (likewise)
    const float* prm;      // [scenes or 1, 9 + 8 lights]
    float* out;            // [scenes, pixels, 3]
    const float* gout;     // [scenes, pixels, 3]
    float* gg;             // [scenes, pixels, Cg] or nullptr
    float* gcol;           // [scenes, pixels, 3] or nullptr (colour tensor)
    float* gmat;           // [scenes, pixels, 2] or nullptr (material tensor)
    float* partial;        // [scenes, blocks, 9 + 8 lights] or nullptr
    long long pixels;      // of one scene
    int Cg, cstride, mstride, oc, omat, on, op, om, pstride;   // channel offsets (oc / omat: -1 with a tensor; om: -1 = absent); pstride: 0 = one block for every scene
    int nl;                // lights
    unsigned kinds;        // bit i: light i is a point light
    int clamp;
    float lo, hi, min_roughness, f0;
};

// with a visibility: what the VIS kernels take (the others' argument stays as it is)
struct ShadePbrVisParams : ShadePbrParams {
    const float* vis;      // a pixel's factors: nl floats, vstride apart
    float* gvis;           // [scenes, pixels, nl] or nullptr
    int vstride;
};

#ifdef DIRT_SHADE_PBR_VISIBILITY_UNIT   // this unit's kernels: their names, their argument, whether they take a visibility
#define PBR_FORWARD_KERNEL shade_visible_pbr_forward_kernel
#define PBR_BACKWARD_KERNEL shade_visible_pbr_backward_kernel
typedef ShadePbrVisParams PbrUnitParams;
constexpr bool PBR_VIS = true;
#else
#define PBR_FORWARD_KERNEL shade_pbr_forward_kernel
#define PBR_BACKWARD_KERNEL shade_pbr_backward_kernel
typedef ShadePbrParams PbrUnitParams;
constexpr bool PBR_VIS = false;
#endif

// light l's factor at a pixel, and where its gradient goes (templates, so that only the VIS unit's argument needs the fields)
template <bool VIS, class PRM>
__device__ __forceinline__ float pbr_visibility(const PRM& P, long long pix, int l)
{
    if constexpr (VIS) return P.vis[pix * P.vstride + l];
    else return 1.f;
}

template <bool VIS, int NL, class PRM>
__device__ __forceinline__ void pbr_store_grad_visibility(const PRM& P, long long pix, int l, float g)
{
    if constexpr (VIS) {
        if (P.gvis) P.gvis[pix * NL + l] = g;
    }
}

// what the lights of a pixel share: the material's, and the GGX terms
struct PbrPixel : MaterialPixel { float rho2, a2, k, omk, gv; };

// one light at a pixel
struct PbrLight {
    float tl[3], l[3], len_l, inv_l, th[3], h[3], len_h, inv_h;
    float nl_raw, nh_raw, vh_raw, nl, nh, vh;
    float x[3], den, D, gl, Vis, w4, w5, F[3], kd[3], B[3];   // B: kd c / pi + D Vis F
};

// loads a pixel and evaluates what its lights share
__device__ __forceinline__ void pbr_pixel(const ShadePbrParams& P, const float* __restrict__ prm, long long pix, PbrPixel& px)
{
    material_load(P, prm, pix, px);
    px.rho2 = px.rho * px.rho;
    px.a2 = px.rho2 * px.rho2;
    px.k = ((px.rho + 1.f) * (px.rho + 1.f)) * 0.125f;
    px.omk = 1.f - px.k;
    material_fresnel(P, px);   // (behind the terms of rho: dirt_shade_common.h says why)
    px.gv = px.nv * px.omk + px.k;
}

// one light: lp its eight floats of the block, point whether it is a point light
__device__ __forceinline__ void pbr_light(const float* __restrict__ lp, bool point, const PbrPixel& px, PbrLight& L)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) L.tl[j] = point ? lp[j] - px.p[j] : -lp[j];
    unit3(L.tl, L.l, L.len_l, L.inv_l);
#pragma unroll
    for (int j = 0; j < 3; ++j) L.th[j] = L.l[j] + px.v[j];
    unit3(L.th, L.h, L.len_h, L.inv_h);
    L.nl_raw = dot3(px.N, L.l); L.nh_raw = dot3(px.N, L.h); L.vh_raw = dot3(px.v, L.h);
    L.nl = max0(L.nl_raw); L.nh = max0(L.nh_raw); L.vh = max0(L.vh_raw);
    cross3(px.N, L.h, L.x);
    L.den = dot3(L.x, L.x) + px.a2 * (L.nh * L.nh);
    L.D = px.a2 / (PBR_PI * (L.den * L.den));
    L.gl = L.nl * px.omk + px.k;
    L.Vis = 0.25f / (L.gl * px.gv);
    const float w = 1.f - L.vh, w2 = w * w;
    L.w4 = w2 * w2;
    L.w5 = L.w4 * w;
    const float S = L.D * L.Vis;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        L.F[j] = px.F0[j] + (1.f - px.F0[j]) * L.w5;
        L.kd[j] = (1.f - L.F[j]) * px.ommu;
        L.B[j] = (L.kd[j] * px.c[j]) * PBR_INV_PI + S * L.F[j];
    }
}

// ---- forward: one pixel per lane; the parameters are wave-uniform (scalar loads), the loop over the lights is uniform
__global__ __launch_bounds__(PBR_BLOCK) void PBR_FORWARD_KERNEL(PbrUnitParams P)
{
    const long long i = (long long)blockIdx.x * PBR_BLOCK + threadIdx.x;
    if (i >= P.pixels) return;
    const long long pix = (long long)blockIdx.y * P.pixels + i;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    PbrPixel px;
    pbr_pixel(P, prm, pix, px);
    float lit[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) lit[j] = prm[j] * px.c[j];
    for (int l = 0; l < P.nl; ++l) {   // (uniform)
        const float* __restrict__ lp = prm + PBR_HEAD + PBR_LIGHT * l;
        PbrLight L;
        pbr_light(lp, (P.kinds >> l) & 1u, px, L);
        if constexpr (PBR_VIS) {
            const float sv = pbr_visibility<PBR_VIS>(P, pix, l);
#pragma unroll
            for (int j = 0; j < 3; ++j) lit[j] += L.B[j] * ((lp[3 + j] * L.nl) * sv);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) lit[j] += L.B[j] * (lp[3 + j] * L.nl);
        }
    }
    const float om = 1.f - px.m;
    float o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = clamp_out(P, lit[j] * px.m + prm[3 + j] * om);
    store3(P.out + pix * 3, o);
}

// ---- backward.  NL: the light count; PARAMS: the parameter block wants its gradient; GBUF: the G-buffer does.  The
// gradients of a colour / material tensor leave by one store per lane where P.gcol / P.gmat is there, the visibility's
// (VIS) by one per lane and light where P.gvis is.
template <int NL, bool PARAMS, bool GBUF>
__global__ __launch_bounds__(PBR_BLOCK) void PBR_BACKWARD_KERNEL(PbrUnitParams P)
{
    constexpr int NP = PBR_HEAD + PBR_LIGHT * NL;
    constexpr int NA = PARAMS ? NP : 1;
    __shared__ float s_g[GBUF ? PBR_BLOCK * MATERIAL_ROW : 1];
    __shared__ unsigned char s_src[GBUF ? DIRT_SHADE_MAX_CHANNELS : 1];
    __shared__ float s_part[PARAMS ? 4 * NP : 1];
    const int tid = threadIdx.x;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
    const int Cg = P.Cg;
    const TileWalk walk = tile_walk<PBR_BLOCK>(Cg, tid);
    if constexpr (GBUF) {
        for (int ch = tid; ch < Cg; ch += PBR_BLOCK) s_src[ch] = (unsigned char)material_source(P, ch);
        s_g[tid * MATERIAL_ROW + MATERIAL_ZERO] = 0.f;
    }
    for (int it = 0; it < PBR_ITER; ++it) {
        const long long first = ((long long)blockIdx.x * PBR_ITER + it) * PBR_BLOCK;   // (uniform)
        if (first >= P.pixels) break;
        const int npx = (int)(P.pixels - first < PBR_BLOCK ? P.pixels - first : PBR_BLOCK);
        const long long pix = (long long)blockIdx.y * P.pixels + first + tid;
        if (tid < npx) {
            PbrPixel px;
            pbr_pixel(P, prm, pix, px);
            float go[3];
            load3(P.gout + pix * 3, go);
            // the forward: the lights' sum decides where the clamp passes the gradient.  A rolled loop, so that no light's
            // state is kept from here to its gradient below: a light is evaluated twice
            float lit[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) lit[j] = prm[j] * px.c[j];
#pragma unroll 1
            for (int l = 0; l < NL; ++l) {
                const float* __restrict__ lp = prm + PBR_HEAD + PBR_LIGHT * l;
                PbrLight L;
                pbr_light(lp, (P.kinds >> l) & 1u, px, L);
                if constexpr (PBR_VIS) {
                    const float sv = pbr_visibility<PBR_VIS>(P, pix, l);
#pragma unroll
                    for (int j = 0; j < 3; ++j) lit[j] += L.B[j] * ((lp[3 + j] * L.nl) * sv);
                } else {
#pragma unroll
                    for (int j = 0; j < 3; ++j) lit[j] += L.B[j] * (lp[3 + j] * L.nl);
                }
            }
            const float om = 1.f - px.m;
            float glit[3], gc[3], gm = 0.f, gmb = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float pre = lit[j] * px.m + prm[3 + j] * om;
                const float gpre = clamp_gate(P, pre, go[j]);
                glit[j] = gpre * px.m;
                gm += gpre * lit[j];
                gmb += gpre * prm[3 + j];
                gc[j] = glit[j] * prm[j];
                if constexpr (PARAMS) {
                    acc[j] += glit[j] * px.c[j];
                    acc[3 + j] += gpre * om;
                }
            }
            gm -= gmb;   // d (background (1 - m)) / d m
            // what the lights leave for the values they share
            float gN[3] = {0.f, 0.f, 0.f}, gvv[3] = {0.f, 0.f, 0.f}, gp[3] = {0.f, 0.f, 0.f}, gF0[3] = {0.f, 0.f, 0.f};
            float g_gv = 0.f, g_k = 0.f, g_a2 = 0.f, g_ommu = 0.f;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const float* __restrict__ lp = prm + PBR_HEAD + PBR_LIGHT * l;
                const bool point = (P.kinds >> l) & 1u;   // (uniform)
                PbrLight L;
                pbr_light(lp, point, px, L);
                const float S = L.D * L.Vis;
                float g_nl = 0.f, gS = 0.f, g_w5 = 0.f;
                [[maybe_unused]] const float sv = pbr_visibility<PBR_VIS>(P, pix, l);
                [[maybe_unused]] float gsv = 0.f;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    float gB, gknl;
                    if constexpr (PBR_VIS) {
                        const float knl = lp[3 + j] * L.nl;
                        gB = glit[j] * (knl * sv);
                        gknl = glit[j] * L.B[j];
                        gsv += gknl * knl;
                        gknl = gknl * sv;
                    } else {
                        gB = glit[j] * (lp[3 + j] * L.nl);
                        gknl = glit[j] * L.B[j];
                    }
                    if constexpr (PARAMS) acc[PBR_HEAD + PBR_LIGHT * l + 3 + j] += gknl * L.nl;
                    g_nl += gknl * lp[3 + j];
                    const float gkd = (gB * px.c[j]) * PBR_INV_PI;
                    gc[j] += (gB * L.kd[j]) * PBR_INV_PI;
                    gS += gB * L.F[j];
                    const float gF = gB * S - gkd * px.ommu;
                    g_ommu += gkd * (1.f - L.F[j]);
                    gF0[j] += gF * (1.f - L.w5);
                    g_w5 += gF * (1.f - px.F0[j]);
                }
                if constexpr (PBR_VIS) pbr_store_grad_visibility<PBR_VIS, NL>(P, pix, l, gsv);
                const float g_vh = -(g_w5 * (5.f * L.w4));
                const float gD = gS * L.Vis, gVis = gS * L.D;
                const float t = -(gVis * L.Vis);          // Vis = 0.25 / (gl gv)
                const float g_gl = t / L.gl;
                g_gv += t / px.gv;
                g_nl += g_gl * px.omk;                    // gl = nl (1 - k) + k
                g_k += g_gl * (1.f - L.nl);
                const float g_den = -2.f * ((L.D / L.den) * gD);   // D = a2 / (pi den^2)
                g_a2 += gD / (PBR_PI * (L.den * L.den)) + g_den * (L.nh * L.nh);
                const float g_nh = g_den * (px.a2 * (2.f * L.nh));   // den = |N x h|^2 + a2 nh^2
                float gx[3], t1[3], gh[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) gx[j] = (2.f * g_den) * L.x[j];
                cross3(L.h, gx, t1);       // x = N x h: d N = h x gx, d h = gx x N
                cross3(gx, px.N, gh);
                const float g_nl_raw = L.nl_raw >= 0.f ? g_nl : 0.f, g_nh_raw = L.nh_raw >= 0.f ? g_nh : 0.f;
                const float g_vh_raw = L.vh_raw >= 0.f ? g_vh : 0.f;
                float gl[3], gth[3], gtl[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    gN[j] += (t1[j] + g_nl_raw * L.l[j]) + g_nh_raw * L.h[j];
                    gh[j] += g_nh_raw * px.N[j] + g_vh_raw * px.v[j];
                }
                unit3_backward(gh, L.th, L.len_h, L.inv_h, gth);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    gl[j] = g_nl_raw * px.N[j] + gth[j];
                    gvv[j] += g_vh_raw * L.h[j] + gth[j];
                }
                unit3_backward(gl, L.tl, L.len_l, L.inv_l, gtl);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    gp[j] -= point ? gtl[j] : 0.f;
                    if constexpr (PARAMS) acc[PBR_HEAD + PBR_LIGHT * l + j] += point ? gtl[j] : -gtl[j];
                }
            }
            const float g_nv = g_gv * px.omk;             // gv = nv (1 - k) + k
            g_k += g_gv * (1.f - px.nv);
            const float g_nv_raw = px.nv_raw >= 0.f ? g_nv : 0.f;
            float gtv[3], gn[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gN[j] += g_nv_raw * px.v[j];
                gvv[j] += g_nv_raw * px.N[j];
            }
            unit3_backward(gvv, px.tv, px.len_v, px.inv_v, gtv);
            unit3_backward(gN, px.n, px.len_n, px.inv_n, gn);
            float gmu = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gp[j] -= gtv[j];
                if constexpr (PARAMS) acc[6 + j] += gtv[j];
                g_ommu += P.f0 * gF0[j];                  // F0 = f0 (1 - mu) + c mu
                gc[j] += gF0[j] * px.mu;
                gmu += gF0[j] * px.c[j];
            }
            gmu -= g_ommu;
            const float g_rho = g_k * ((px.rho + 1.f) * 0.25f) + (g_a2 * (2.f * px.rho2)) * (2.f * px.rho);
            const float gr = (px.r >= P.min_roughness && px.r <= 1.f) ? g_rho : 0.f;   // closed at both edges; 0 at a NaN
            if (P.gcol) store3(P.gcol + pix * 3, gc);
            if (P.gmat) { P.gmat[pix * 2] = gr; P.gmat[pix * 2 + 1] = gmu; }
            if constexpr (GBUF) {
                float* __restrict__ r = s_g + tid * MATERIAL_ROW;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    r[j] = gc[j];
                    r[3 + j] = gn[j];
                    r[6 + j] = gp[j];
                }
                r[9] = gr; r[10] = gmu; r[11] = gm;
            }
        }
        if constexpr (GBUF)
            tile_rows_out<PBR_BLOCK, MATERIAL_ROW>(s_g, s_src, P.gg + ((long long)blockIdx.y * P.pixels + first) * Cg, npx, Cg, tid, walk);
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

template <int NL>
static void shade_pbr_launch_backward(const PbrUnitParams& P, bool params, bool gbuf, dim3 grid, hipStream_t s)
{
    if (params && gbuf) hipLaunchKernelGGL((PBR_BACKWARD_KERNEL<NL, true, true>), grid, dim3(PBR_BLOCK), 0, s, P);
    else if (params) hipLaunchKernelGGL((PBR_BACKWARD_KERNEL<NL, true, false>), grid, dim3(PBR_BLOCK), 0, s, P);
    else if (gbuf) hipLaunchKernelGGL((PBR_BACKWARD_KERNEL<NL, false, true>), grid, dim3(PBR_BLOCK), 0, s, P);
    else hipLaunchKernelGGL((PBR_BACKWARD_KERNEL<NL, false, false>), grid, dim3(PBR_BLOCK), 0, s, P);
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

// what this file's entry points refuse (the shared refusals, and `a`: dirt_shade_common.h)
static int shade_pbr_check(const char* who, const dirt::MaterialArgs& a, long long pixels, int lights, unsigned light_kinds, dirt::ShadePbrParams& P)
{
    if (int rc = dirt::material_check_sizes(who, a, pixels)) return rc;
    if (lights < 0 || lights > DIRT_SHADE_PBR_MAX_LIGHTS) STAGE_FAIL("%s: %d lights, at most %d", who, lights, DIRT_SHADE_PBR_MAX_LIGHTS);
    if (light_kinds >> lights) STAGE_FAIL("%s: light_kinds 0x%x has bits beyond %d lights", who, light_kinds, lights);
    if (int rc = dirt::material_check_layout(who, a)) return rc;
    if (int rc = dirt::material_check_scalars(who, a)) return rc;
    dirt::material_fill(P, a, pixels, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights);
    P.nl = lights; P.kinds = light_kinds;
    return DIRT_OK;
}

#ifndef DIRT_SHADE_PBR_VISIBILITY_UNIT

size_t dirt_shade_pbr_scratch_bytes(long long scenes, long long pixels, int lights)
{
    if (lights < 0 || lights > DIRT_SHADE_PBR_MAX_LIGHTS) return 0;
    return dirt::shade_scratch_bytes(scenes, pixels, dirt::PBR_SPAN, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights);
}

int dirt_shade_pbr_forward(const float* gbuffer, const float* colors, const float* material, const float* params, float* out,
                           long long scenes, long long pixels, int Cg, int color_stride, int material_stride, int off_colors,
                           int off_material, int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                           unsigned light_kinds, float min_roughness, float dielectric_f0, float clamp_lo, float clamp_hi, unsigned flags,
                           void* stream)
{
    const char* who = "dirt_shade_pbr_forward";
    const dirt::MaterialArgs a{gbuffer, colors, material, scenes, Cg, color_stride, material_stride, off_colors, off_material, off_normals,
                               off_positions, off_mask, param_scenes, min_roughness, dielectric_f0, clamp_lo, clamp_hi, flags};
    dirt::ShadePbrParams P{};
    if (int rc = shade_pbr_check(who, a, pixels, lights, light_kinds, P)) return rc;
    if (scenes * pixels == 0) return dirt::stage_ok(report);
    if (!gbuffer || !params || !out) STAGE_FAIL("%s: gbuffer / params / out is NULL", who);
    if (pixels > 0x7fffffffll * dirt::PBR_BLOCK) STAGE_FAIL("%s: too many pixels per scene", who);
    dirt::material_inputs(P, a);
    P.prm = params; P.out = out;
    const dim3 grid((unsigned)((pixels + dirt::PBR_BLOCK - 1) / dirt::PBR_BLOCK), (unsigned)scenes);
    hipLaunchKernelGGL(dirt::shade_pbr_forward_kernel, grid, dim3(dirt::PBR_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_shade_pbr_backward(const float* gbuffer, const float* colors, const float* material, const float* params, const float* grad_out,
                            float* grad_gbuffer, float* grad_colors, float* grad_material, float* grad_params, void* scratch,
                            size_t scratch_bytes, long long scenes, long long pixels, int Cg, int color_stride, int material_stride,
                            int off_colors, int off_material, int off_normals, int off_positions, int off_mask, int param_scenes, int lights,
                            unsigned light_kinds, float min_roughness, float dielectric_f0, float clamp_lo, float clamp_hi, unsigned flags,
                            void* stream)
{
    const char* who = "dirt_shade_pbr_backward";
    const dirt::MaterialArgs a{gbuffer, colors, material, scenes, Cg, color_stride, material_stride, off_colors, off_material, off_normals,
                               off_positions, off_mask, param_scenes, min_roughness, dielectric_f0, clamp_lo, clamp_hi, flags};
    dirt::ShadePbrParams P{};
    int rc = shade_pbr_check(who, a, pixels, lights, light_kinds, P);
    if (!rc) rc = dirt::material_check_grads(who, a, grad_colors, grad_material);
    if (rc) return rc;
    if (scenes * pixels == 0 || (!grad_gbuffer && !grad_params && !grad_colors && !grad_material)) return dirt::stage_ok(report);
    if (!gbuffer || !params || !grad_out) STAGE_FAIL("%s: gbuffer / params / grad_out is NULL", who);
    if (grad_params) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_shade_pbr_scratch_bytes(scenes, pixels, lights),
                                 "dirt_shade_pbr_scratch_bytes");
        if (rc) return rc;
    }
    const long long blocks = dirt::shade_blocks(pixels, dirt::PBR_SPAN);
    if (blocks > 0x7fffffffll) STAGE_FAIL("%s: too many pixels per scene", who);
    dirt::material_inputs(P, a);
    P.prm = params; P.gout = grad_out; P.gg = grad_gbuffer; P.gcol = grad_colors; P.gmat = grad_material;
    P.partial = static_cast<float*>(scratch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks, (unsigned)scenes);
    const bool params_wanted = grad_params != nullptr, gbuf = grad_gbuffer != nullptr;
    switch (lights) {
    case 0: dirt::shade_pbr_launch_backward<0>(P, params_wanted, gbuf, grid, s); break;
    case 1: dirt::shade_pbr_launch_backward<1>(P, params_wanted, gbuf, grid, s); break;
    case 2: dirt::shade_pbr_launch_backward<2>(P, params_wanted, gbuf, grid, s); break;
    case 3: dirt::shade_pbr_launch_backward<3>(P, params_wanted, gbuf, grid, s); break;
    default: dirt::shade_pbr_launch_backward<4>(P, params_wanted, gbuf, grid, s); break;
    }
    return dirt::shade_backward_finish(who, scratch, grad_params, scenes, blocks, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights, param_scenes, s);
}

#endif   // (the entry points with a visibility: dirt_shade_pbr_visibility.hip)

}  // extern "C"
