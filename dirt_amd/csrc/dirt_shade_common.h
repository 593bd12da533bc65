// dirt_shade_common.h -- what the G-buffer kernels share (dirt_shade.hip and its second unit dirt_shade_albedo.hip: the three
// reflectance models; dirt_shade_sh.hip: spherical harmonics; dirt_shade_pbr.hip: Cook-Torrance; dirt_shade_ibl.hip: image-based lighting; dirt_normal_map.hip: normal
// mapping), each piece written and explained once here.  Device: the tile walk that makes every row of a [pixels, Cg] image leave
// whole, the channel map it reads, the clamp and its gradient gate; of the two material shaders (Cook-Torrance, image-based
// lighting) a pixel's material before any light and the channel map's source function.  Host: the refusals every *_check repeats
// (each file calls them in its own order, with its own checks in between: the order decides which message a caller with two faults
// sees), the scratch size, what follows a backward launch; of the material shaders the parameter struct's fields they have in
// common.  NOT shared: the wave-sum / lane-0 / barrier / fold tail of the backward kernels (dirt_stage.h says why at
// fold_waves_to_row), the other units' shade_*_source functions, the channel map's fill, the pixel arithmetic: what the files differ in.
#pragma once
#include "dirt_stage.h"

namespace dirt {

// ---- device ---------------------------------------------------------------------------------------------------------------

// (The workgroup's shape -- BLOCK lanes, ITER passes -- stays a pair of constants in each file, SHADE_ / SH_ / PBR_ / NM_BLOCK
// and _ITER: each file's tests read them there by name.  Everything below takes them as arguments.)

// A pass is npx <= BLOCK consecutive pixels, npx * Cg consecutive floats of the image.  The workgroup walks them in order, lane
// after lane: lane tid takes elements e = tid, tid + BLOCK, ..., so that consecutive lanes touch consecutive floats whatever
// Cg.  Element e is channel e % Cg of pixel e / Cg; the walk keeps both without dividing inside the loop: it starts at
// (tid / Cg, tid % Cg) and a step adds (BLOCK / Cg, BLOCK % Cg), carrying once where the channel passes Cg (BLOCK % Cg < Cg:
// one carry is enough).  With Cg > BLOCK a step is (0, BLOCK) and the carry does all the pixel's counting.
struct TileWalk { int step_px, step_ch, px0, ch0; };

template <int BLOCK>
__device__ __forceinline__ TileWalk tile_walk(int Cg, int tid) { return TileWalk{BLOCK / Cg, BLOCK % Cg, tid / Cg, tid % Cg}; }

// f(e, pxi, ch) for this lane's elements of a pass of npx pixels (a partial last pass: npx < BLOCK, and the loop ends early)
template <int BLOCK, class F>
__device__ __forceinline__ void tile_for_each(int npx, int Cg, int tid, const TileWalk& wk, F&& f)
{
    const int total = npx * Cg;
    int pxi = wk.px0, ch = wk.ch0;
    for (int e = tid; e < total; e += BLOCK) {
        f(e, pxi, ch);
        pxi += wk.step_px; ch += wk.step_ch;
        if (ch >= Cg) { ch -= Cg; ++pxi; }
    }
}

// A pass's rows (ROW floats a pixel) leave the LDS tile s_g for dst (the pass's first float of the image): every row whole.
// s_src[ch] is the channel map: which value of a pixel's row goes to channel ch, the row's zero for a channel no attribute
// uses.  The first barrier waits for the lanes' rows (and, in the first pass, for the map), the second keeps the next pass
// from overwriting a row that is still being read.
// (Each kernel fills its map, `for (ch = tid; ch < Cg; ch += BLOCK) s_src[ch] = its source function of ch` -- Cg may exceed
// BLOCK: a second turn -- and writes its row's zero itself: with that loop in a helper here, whether it took a lambda or the
// function as a template argument, the compiler laid every kernel of the five units out differently.)
template <int BLOCK, int ROW>
__device__ __forceinline__ void tile_rows_out(const float* s_g, const unsigned char* s_src, float* __restrict__ dst, int npx, int Cg,
                                              int tid, const TileWalk& wk)
{
    __syncthreads();
    tile_for_each<BLOCK>(npx, Cg, tid, wk, [&](int e, int pxi, int ch) { dst[e] = s_g[pxi * ROW + s_src[ch]]; });
    __syncthreads();
}

// The clamp of the output (P: a parameter struct with clamp, lo, hi) and where it passes the gradient g
template <class P>
__device__ __forceinline__ float clamp_out(const P& p, float pre)
{
    if (!p.clamp) return pre;
    return pre < p.lo ? p.lo : (pre > p.hi ? p.hi : pre);   // a NaN stays NaN, as torch.clamp leaves it
}

template <class P>
__device__ __forceinline__ float clamp_gate(const P& p, float pre, float g)
{
    return (!p.clamp || (pre >= p.lo && pre <= p.hi)) ? g : 0.f;   // closed at both edges; 0 at a NaN
}

// ---- what the material shaders share (dirt_shade_pbr.hip, dirt_shade_ibl.hip)

// y = x / max(|x|, 1e-12)
__device__ __forceinline__ void unit3(const float (&x)[3], float (&y)[3], float& len, float& inv)
{
    len = sqrtf(dot3(x, x));
    inv = 1.f / (len < 1.e-12f ? 1.e-12f : len);
#pragma unroll
    for (int j = 0; j < 3; ++j) y[j] = x[j] * inv;
}

// its gradient: gy arrives at y, gx leaves for x
__device__ __forceinline__ void unit3_backward(const float (&gy)[3], const float (&x)[3], float len, float inv, float (&gx)[3])
{
    const float gden = -(dot3(gy, x) * inv) * inv;
    const float glen = len >= 1.e-12f ? gden : 0.f;            // max passes the gradient at its edge
    // d |x| / d x = x / |x|, 0 at a zero vector.  The division stands before the choice, not in one arm of it, where it
    // becomes a branch: a light stays straight-line code
    const float q = glen / (len == 0.f ? 1.f : len);
    const float gl = len == 0.f ? 0.f : q;
#pragma unroll
    for (int j = 0; j < 3; ++j) gx[j] = gy[j] * inv + x[j] * gl;
}

__device__ __forceinline__ float max0(float x) { return x < 0.f ? 0.f : x; }   // a NaN stays NaN, as torch.clamp leaves it

// what the lights of a pixel share, whatever lights it (P below: ShadePbrParams or ShadeIblParams, which name these fields alike)
struct MaterialPixel {
    float c[3], n[3], p[3], r, mu, m;
    float N[3], len_n, inv_n;        // the unit normal
    float tv[3], v[3], len_v, inv_v; // cam - p and its unit vector
    float rho, ommu, F0[3], nv_raw, nv;
};

// loads a pixel and evaluates that, in two parts, one behind the other: dirt_shade_pbr.hip has its GGX terms of rho between
// them (as one function, with those terms behind it, that unit's kernels were scheduled otherwise: 1693 lines of assembly differed)
template <class P>
__device__ __forceinline__ void material_load(const P& p, const float* __restrict__ prm, long long pix, MaterialPixel& px)
{
    const float* __restrict__ row = p.g + pix * p.Cg;
    load3(p.col + pix * p.cstride, px.c);
    load3(row + p.on, px.n);
    load3(row + p.op, px.p);
    const float* __restrict__ mt = p.mat + pix * p.mstride;
    px.r = mt[0]; px.mu = mt[1];
    px.m = p.om >= 0 ? row[p.om] : 1.f;
    unit3(px.n, px.N, px.len_n, px.inv_n);
#pragma unroll
    for (int j = 0; j < 3; ++j) px.tv[j] = prm[6 + j] - px.p[j];
    unit3(px.tv, px.v, px.len_v, px.inv_v);
    px.rho = px.r < p.min_roughness ? p.min_roughness : (px.r > 1.f ? 1.f : px.r);
}

template <class P>
__device__ __forceinline__ void material_fresnel(const P& p, MaterialPixel& px)
{
    px.ommu = 1.f - px.mu;
#pragma unroll
    for (int j = 0; j < 3; ++j) px.F0[j] = p.f0 * px.ommu + px.c[j] * px.mu;
    px.nv_raw = dot3(px.N, px.v);
    px.nv = max0(px.nv_raw);
}

// floats of a pixel's row in the LDS tile: dc[3], dn[3], dp[3], d roughness, d metalness, dm, 0 (odd: no bank conflicts); its zero
// (a lane's twelve stores into its row stay in each kernel: in a helper here, its arrays by reference, by pointer or by value,
// every kernel of dirt_shade_pbr.hip came out with other registers, 27869 lines of assembly)
constexpr int MATERIAL_ROW = 13, MATERIAL_ZERO = 12;

// which value of a pixel's LDS row goes to channel `ch` of d gbuffer (oc / omat are -1 with a tensor: no channel is theirs)
template <class P>
__device__ __forceinline__ int material_source(const P& p, int ch)
{
    if (p.oc >= 0 && (unsigned)(ch - p.oc) < 3u) return ch - p.oc;
    if ((unsigned)(ch - p.on) < 3u) return 3 + ch - p.on;
    if ((unsigned)(ch - p.op) < 3u) return 6 + ch - p.op;
    if (p.omat >= 0 && (unsigned)(ch - p.omat) < 2u) return 9 + ch - p.omat;
    if (ch == p.om) return 11;
    return MATERIAL_ZERO;
}

// dirt_shade.hip: the rows of partial sums of one scene (or of all of them, for a block shared by the batch) added up in a
// fixed order, one workgroup per value.  One copy for every unit: the others call the launcher.
void shade_launch_reduce(const float* partial, float* grad_params, long long rows, int NP, int param_scenes, hipStream_t s);

// ---- host (every G-buffer stage reports into dirt_last_error) -----------------------------------------------------------------

// workgroups of `span` = BLOCK * ITER pixels for `pixels` pixels
inline long long shade_blocks(long long pixels, int span) { return (pixels + span - 1) / span; }

// the sizes a shader takes: blockIdx.y is the scene, 2^40 pixels keep every index inside a long long
inline int shade_check_sizes(const char* who, long long scenes, long long pixels, int Cg)
{
    if (scenes < 0 || pixels < 0) STAGE_FAIL("%s: negative sizes (scenes=%lld pixels=%lld)", who, scenes, pixels);
    if (scenes > 65535) STAGE_FAIL("%s: %lld scenes, at most 65535", who, scenes);
    if (pixels > (1ll << 40)) STAGE_FAIL("%s: %lld pixels per scene, at most 2^40", who, pixels);
    if (Cg < 1 || Cg > DIRT_SHADE_MAX_CHANNELS) STAGE_FAIL("%s: %d G-buffer channels, 1..%d", who, Cg, DIRT_SHADE_MAX_CHANNELS);
    return DIRT_OK;
}

// `count` attributes of a pixel, attribute a in channels off[a] .. off[a] + width[a] - 1 unless absent[a] (no such channels, or
// a tensor of its own: off[a] is not read): each fits in the Cg channels and overlaps none before it
inline int shade_check_attributes(const char* who, int Cg, int count, const int* off, const int* width, const bool* absent,
                                  const char* const* names)
{
    for (int a = 0; a < count; ++a) {
        if (absent[a]) continue;
        if (off[a] < 0 || off[a] + width[a] > Cg) STAGE_FAIL("%s: %s at channel %d does not fit in %d channels", who, names[a], off[a], Cg);
        for (int b = 0; b < a; ++b)
            if (!absent[b] && off[a] < off[b] + width[b] && off[b] < off[a] + width[a])
                STAGE_FAIL("%s: %s (channel %d) overlaps %s (channel %d)", who, names[a], off[a], names[b], off[b]);
    }
    return DIRT_OK;
}

inline int shade_check_clamp(const char* who, unsigned flags, float lo, float hi)
{
    if ((flags & DIRT_SHADE_CLAMP) && !(lo <= hi)) STAGE_FAIL("%s: clamp bounds lo=%g > hi=%g", who, lo, hi);
    return DIRT_OK;
}

// floats between two scenes' parameter blocks of NP floats: 0 = one block for every scene
inline int shade_pstride(int param_scenes, int NP) { return param_scenes == 1 ? 0 : NP; }

// ---- host, what the material shaders share: the arguments both units' entry points take, under the names they take them by
// (colors / material: a tensor of its own, which has no channels -- its offset is not read --, or nullptr for channels) ...
struct MaterialArgs {
    const float *gbuffer, *colors, *material;
    long long scenes;
    int Cg, color_stride, material_stride, off_colors, off_material, off_normals, off_positions, off_mask, param_scenes;
    float min_roughness, f0, lo, hi; unsigned flags;
};

// ... three refusals, which each unit calls in this order with its own in between, a fourth for a backward's missing tensors ...
inline int material_check_sizes(const char* who, const MaterialArgs& a, long long pixels)
{
    if (int rc = shade_check_sizes(who, a.scenes, pixels, a.Cg)) return rc;
    if (a.colors && a.color_stride < 3) STAGE_FAIL("%s: color_stride=%d, a pixel's colour is 3 floats", who, a.color_stride);
    if (a.material && a.material_stride < 2) STAGE_FAIL("%s: material_stride=%d, a pixel's material is 2 floats", who, a.material_stride);
    return DIRT_OK;
}

inline int material_check_layout(const char* who, const MaterialArgs& a)
{
    if (a.param_scenes != 1 && a.param_scenes != a.scenes) STAGE_FAIL("%s: param_scenes=%d is neither 1 nor scenes=%lld", who, a.param_scenes, a.scenes);
    if (a.flags & ~DIRT_SHADE_CLAMP) STAGE_FAIL("%s: unknown flags 0x%x", who, a.flags);
    const int off[5] = {a.off_colors, a.off_material, a.off_normals, a.off_positions, a.off_mask}, width[5] = {3, 2, 3, 3, 1};
    const bool absent[5] = {a.colors != nullptr, a.material != nullptr, false, false, a.off_mask == -1};
    const char* const names[5] = {"colors", "material", "normals", "positions", "mask"};
    return shade_check_attributes(who, a.Cg, 5, off, width, absent, names);
}

inline int material_check_scalars(const char* who, const MaterialArgs& a)
{
    if (!(a.min_roughness > 0.f && a.min_roughness <= 1.f)) STAGE_FAIL("%s: min_roughness=%g is not in (0, 1]", who, a.min_roughness);
    if (!(a.f0 >= 0.f && a.f0 <= 1.f)) STAGE_FAIL("%s: dielectric_f0=%g is not in [0, 1]", who, a.f0);
    return shade_check_clamp(who, a.flags, a.lo, a.hi);
}

inline int material_check_grads(const char* who, const MaterialArgs& a, const float* grad_colors, const float* grad_material)
{
    if (grad_colors && !a.colors) STAGE_FAIL("%s: grad_colors without colors (the channel path's is part of grad_gbuffer)", who);
    if (grad_material && !a.material) STAGE_FAIL("%s: grad_material without material (the channel path's is part of grad_gbuffer)", who);
    return DIRT_OK;
}

// ... and the fields of the parameter struct P that follow from them: after the checks everything but the pointers and what
// the unit adds (pixels of a scene, NP floats of a parameter block); before the launch (below) where a pixel's attributes are read
template <class P>
inline void material_fill(P& p, const MaterialArgs& a, long long pixels, int NP)
{
    p.pixels = pixels; p.Cg = a.Cg; p.oc = a.colors ? -1 : a.off_colors; p.omat = a.material ? -1 : a.off_material;
    p.on = a.off_normals; p.op = a.off_positions; p.om = a.off_mask;
    p.cstride = a.colors ? a.color_stride : a.Cg; p.mstride = a.material ? a.material_stride : a.Cg;
    p.pstride = shade_pstride(a.param_scenes, NP);
    p.clamp = (a.flags & DIRT_SHADE_CLAMP) ? 1 : 0;
    p.lo = a.lo; p.hi = a.hi; p.min_roughness = a.min_roughness; p.f0 = a.f0;
}
template <class P>
inline void material_inputs(P& p, const MaterialArgs& a)
{
    p.g = a.gbuffer; p.col = a.colors ? a.colors : a.gbuffer + a.off_colors; p.mat = a.material ? a.material : a.gbuffer + a.off_material;
}

// the scratch of a backward pass: one row of NP partial sums per workgroup; 0 for sizes the entry points refuse
inline size_t shade_scratch_bytes(long long scenes, long long pixels, int span, int NP)
{
    if (scenes < 0 || scenes > 65535 || pixels < 0 || pixels > (1ll << 40)) return 0;
    return sizeof(float) * (size_t)scenes * (size_t)shade_blocks(pixels, span) * (size_t)NP;
}

// after the launch of a backward kernel on (blocks, scenes) workgroups: its launch error, then (grad_params: the parameter
// block wants its gradient) the sum of the rows it left in scratch, then the status the entry point returns
inline int shade_backward_finish(const char* who, const void* scratch, float* grad_params, long long scenes, long long blocks, int NP,
                                 int param_scenes, hipStream_t s)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return stage_hip(set_last_error, who, e);
    if (grad_params) {
        const long long rows = param_scenes == 1 ? scenes * blocks : blocks;
        shade_launch_reduce(static_cast<const float*>(scratch), grad_params, rows, NP, param_scenes, s);
        e = hipGetLastError();
    }
    return stage_hip(set_last_error, who, e);
}

}  // namespace dirt
