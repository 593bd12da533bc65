// dirt_shade_ibl.hip -- split-sum image-based lighting of a G-buffer, fused: one pass forward; backward one per-pixel pass and
// the cube look-up's own backward kernels for the scatter into the two cubes.
//
// The light of dirt_shade_pbr.hip's material under an environment instead of point lights: the GGX-prefiltered pyramid of
// texture.prefilter_cube looked up at the mirrored view vector, the irradiance cube of convolve_cube(kind='lambert') looked up
// at the normal, and the table of lighting.environment_brdf that holds what the specular lobe reflects of a white environment.
// The specification (DESIGN.md §7b restates it; dirt_amd/lighting.py::image_based_lighting is its readable form, which
// tests/shade_ibl_reference.py composes in float64), per pixel with albedo c, normal n, position p, roughness r, metalness mu,
// mask m (1 without a mask channel):
//
//     N = n / max(|n|, 1e-12)               v = normalize(cam - p)          nv_raw = N . v         nv = max(nv_raw, 0)
//     rho = clamp(r, min_roughness, 1)      F0_j = dielectric_f0 (1 - mu) + c_j mu
//     R = 2 nv_raw N - v                    (the unclamped product)
//     (A, B) = bilinear look-up of the table [S, S, 2] at col = clamp(nv S - 0.5, 0, S - 1), row = clamp(rho S - 0.5, 0, S - 1)
//     S_j = F0_j A + B
//     spec_j = trilinear look-up of the pyramid at R, lod = rho (L - 1)     (spec 5 of dirt_texture_cube.hip)
//     E_j = bilinear look-up of the irradiance cube at n                    (the raw normal: an all-zero n gives 0)
//     L_j = intensity_j ((1 - S_j)(1 - mu) c_j E_j + S_j spec_j)
//     out_j = clamp(L_j m + background_j (1 - m), lo, hi)
//
//  Gradients are torch autograd's for that composition: max(x, 0) and the clamps pass the gradient at their edges (d col / d nv
//  is S where nv S - 0.5 lies in [0, S - 1], bounds included: the rule of cube_index), the norm of a zero vector has gradient 0,
//  an invalid direction adds nothing, d spec / d lod is the difference of the two levels inside (0, L - 1) and 0 outside.
//
// The parameter block is [scenes or 1, 9] floats in the layout of dirt_shade.hip's head: intensity (in the ambient slot),
// background, camera.
//
// Kernels: the tiling, the clamp, MaterialPixel, the channel map and the host checks of dirt_shade_common.h; the look-ups of
// dirt_texture_cube.h (cube_sample: a level's three channels with their derivatives).  Forward one pixel per lane: 16 texels
// of the pyramid, 4 of the irradiance cube, 4 of the table, read through the cache (the table is 8 KB at S = 32 and every lane of a wave reads neighbouring texels of it).  Backward IBL_ITER
// passes of 256 pixels per workgroup inside one scene: the forward again with the derivative of every look-up by its own index,
// d gbuffer through an LDS tile, the tensors' gradients by one dense store per lane, the nine parameter sums wave_sum ->
// fold_waves_to_row -> one row per workgroup -> shade_launch_reduce.  No atomics.  What the two cubes' gradients need it leaves
// in caller scratch per pixel -- R, lod, and the gradients arriving at spec and at E -- and the entry point hands those to
// cube_backward_launch twice: the scatter stays with the kernels that have the LDS-patch scheme.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"
#include "dirt_texture_cube.h"

namespace dirt {

constexpr int IBL_BLOCK = 256;     // lanes of a workgroup, pixels of one of its passes
constexpr int IBL_ITER = 4;       // passes of a backward workgroup
constexpr int IBL_SPAN = IBL_BLOCK * IBL_ITER;   // pixels of a backward workgroup
constexpr int IBL_NP = DIRT_SHADE_PARAM_HEAD;    // floats of the parameter block
constexpr int IBL_PIXEL_FLOATS = 10;   // per-pixel floats of the scratch: R[3], lod, d spec[3], d E[3]

struct ShadeIblParams {
    const float *g, *col, *mat;   // the G-buffer, a pixel's colour and its material: as ShadePbrParams'
    const float* prm;      // [scenes or 1, 9]
    const float* pyr;      // [6, face_floats]: the prefiltered pyramid, 3 channels
    const float* irr;      // [6, M, M, 3]
    const float* tab;      // [S, S, 2]
    float* out;            // [scenes, pixels, 3]
    const float* gout;     // [scenes, pixels, 3]
    float *gg, *gcol, *gmat;   // their gradients, each or nullptr: as ShadePbrParams'
    float* partial;       // [scenes, blocks, 9] or nullptr
    float* s_dir;          // [scenes, pixels, 3]: R; these four or nullptr (no cube wants its gradient)
    float* s_lod;          // [scenes, pixels]
    float* s_gspec;        // [scenes, pixels, 3]: what arrives at spec
    float* s_girr;         // [scenes, pixels, 3]: what arrives at E
    long long pixels, face_floats;   // pixels of one scene, floats of a face of the pyramid
    int Cg, cstride, mstride, oc, omat, on, op, om, pstride;   // as ShadePbrParams'
    int N, L, M, S;        // pyramid size and levels, irradiance size, table size
    int clamp;
    float lo, hi, min_roughness, f0;
};

// everything the forward computes at a pixel; the derivatives only where GRAD
struct IblEval {
    float R[3], lod, f;
    bool inside;                     // d spec / d lod is the levels' difference here
    CubeLook qr, qn;
    CubeSample s0, s1, e;             // the two levels of the pyramid at R, the irradiance at n
    float spec[3], A, B, A_nv, A_rho, B_nv, B_rho;
    float S[3], wd[3], T[3];         // S_j; (1 - S_j)(1 - mu) c_j; the light before the intensity
};

// x S - 0.5 clamped to the table, and d index / d x
__device__ __forceinline__ float ibl_table_index(float x, int S, float& d)
{
    const float i = x * (float)S - 0.5f, top = (float)(S - 1);
    d = i >= 0.f && i <= top ? (float)S : 0.f;
    return i < 0.f ? 0.f : (i > top ? top : i);
}

template <bool GRAD>
__device__ __forceinline__ void ibl_eval(const ShadeIblParams& P, const MaterialPixel& px, IblEval& e)
{
    // the table
    float drow, dcol;
    const float row = ibl_table_index(px.rho, P.S, drow), col = ibl_table_index(px.nv, P.S, dcol);
    const Taps k = bilinear_taps(row, col, P.S, P.S);
    const Four<size_t> o = tap_offsets(k, P.S, 2, 0);
    const float* __restrict__ t = P.tab;
    const Four<float> ta = {t[o.tl], t[o.tr], t[o.bl], t[o.br]}, tb = {t[o.tl + 1], t[o.tr + 1], t[o.bl + 1], t[o.br + 1]};
    e.A = bilinear_blend(ta.tl, ta.tr, ta.bl, ta.br, k);
    e.B = bilinear_blend(tb.tl, tb.tr, tb.bl, tb.br, k);
    if constexpr (GRAD) {
        float e_fr, e_fc;
        tap_gradients(1.f, ta, k, e_fr, e_fc);
        e.A_nv = e_fc * dcol; e.A_rho = e_fr * drow;
        tap_gradients(1.f, tb, k, e_fr, e_fc);
        e.B_nv = e_fc * dcol; e.B_rho = e_fr * drow;
    }
    // the pyramid at the mirrored view vector
#pragma unroll
    for (int j = 0; j < 3; ++j) e.R[j] = (2.f * px.nv_raw) * px.N[j] - px.v[j];
    e.lod = px.rho * (float)(P.L - 1);
    int l;
    mip_split(e.lod, P.L, l, e.f);
    e.inside = e.lod > 0.f && e.lod < (float)(P.L - 1);
    e.qr = cube_look(e.R[0], e.R[1], e.R[2]);
    cube_sample_clear(e.s0); cube_sample_clear(e.s1);
    if (e.qr.valid) {
        const float* __restrict__ face = P.pyr + (size_t)e.qr.face() * P.face_floats;
        const int n0 = mip_dim(P.N, l);
        cube_sample<GRAD>(face + cube_level_offset(P.N, n0, 3), n0, e.qr, e.s0);
        if (e.f != 0.f || (GRAD && e.inside)) {   // the second level: blended in where it carries weight, read for d lod inside
            const int n1 = mip_dim(P.N, l + 1);
            cube_sample<GRAD>(face + cube_level_offset(P.N, n1, 3), n1, e.qr, e.s1);
        }
    }
    const float w0 = 1.f - e.f;
    // the irradiance at the raw normal
    e.qn = cube_look(px.n[0], px.n[1], px.n[2]);
    cube_sample_clear(e.e);
    if (e.qn.valid) cube_sample<GRAD>(P.irr + (size_t)e.qn.face() * ((size_t)P.M * P.M * 3), P.M, e.qn, e.e);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        e.spec[j] = e.f != 0.f ? w0 * e.s0.v[j] + e.f * e.s1.v[j] : e.s0.v[j];
        e.S[j] = px.F0[j] * e.A + e.B;
        e.wd[j] = ((1.f - e.S[j]) * px.ommu) * px.c[j];
        e.T[j] = e.wd[j] * e.e.v[j] + e.S[j] * e.spec[j];
    }
}

// ---- forward: one pixel per lane; the parameters are wave-uniform (scalar loads)
__global__ __launch_bounds__(IBL_BLOCK) void shade_ibl_forward_kernel(ShadeIblParams P)
{
    const long long i = (long long)blockIdx.x * IBL_BLOCK + threadIdx.x;
    if (i >= P.pixels) return;
    const long long pix = (long long)blockIdx.y * P.pixels + i;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    MaterialPixel px;
    material_load(P, prm, pix, px); material_fresnel(P, px);
    IblEval e;
    ibl_eval<false>(P, px, e);
    const float om = 1.f - px.m;
    float o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = clamp_out(P, (prm[j] * e.T[j]) * px.m + prm[3 + j] * om);
    store3(P.out + pix * 3, o);
}

// ---- backward.  PARAMS: the parameter block wants its gradient; GBUF: the G-buffer does.  The gradients of a colour /
// material tensor leave by one store per lane where P.gcol / P.gmat is there, the cubes' per-pixel scratch where P.s_dir is.
template <bool PARAMS, bool GBUF>
__global__ __launch_bounds__(IBL_BLOCK) void shade_ibl_backward_kernel(ShadeIblParams P)
{
    constexpr int NP = IBL_NP;
    constexpr int NA = PARAMS ? NP : 1;
    __shared__ float s_g[GBUF ? IBL_BLOCK * MATERIAL_ROW : 1];
    __shared__ unsigned char s_src[GBUF ? DIRT_SHADE_MAX_CHANNELS : 1];
    __shared__ float s_part[PARAMS ? 4 * NP : 1];
    const int tid = threadIdx.x;
    const float* __restrict__ prm = P.prm + (size_t)blockIdx.y * P.pstride;
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
    const int Cg = P.Cg;
    const TileWalk walk = tile_walk<IBL_BLOCK>(Cg, tid);
    if constexpr (GBUF) {
        for (int ch = tid; ch < Cg; ch += IBL_BLOCK) s_src[ch] = (unsigned char)material_source(P, ch);
        s_g[tid * MATERIAL_ROW + MATERIAL_ZERO] = 0.f;
    }
    for (int it = 0; it < IBL_ITER; ++it) {
        const long long first = ((long long)blockIdx.x * IBL_ITER + it) * IBL_BLOCK;   // (uniform)
        if (first >= P.pixels) break;
        const int npx = (int)(P.pixels - first < IBL_BLOCK ? P.pixels - first : IBL_BLOCK);
        const long long pix = (long long)blockIdx.y * P.pixels + first + tid;
        if (tid < npx) {
            MaterialPixel px;
            material_load(P, prm, pix, px); material_fresnel(P, px);
            IblEval e;
            ibl_eval<true>(P, px, e);
            float go[3];
            load3(P.gout + pix * 3, go);
            const float om = 1.f - px.m;
            float gc[3], gspec[3], girr[3], gF0[3], gm = 0.f, g_ommu = 0.f, gA = 0.f, gB = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float lit = prm[j] * e.T[j];
                const float gpre = clamp_gate(P, lit * px.m + prm[3 + j] * om, go[j]);
                const float glit = gpre * px.m;
                gm += gpre * (lit - prm[3 + j]);
                if constexpr (PARAMS) {
                    acc[j] += glit * e.T[j];
                    acc[3 + j] += gpre * om;
                }
                const float gT = glit * prm[j];
                gspec[j] = gT * e.S[j];
                girr[j] = gT * e.wd[j];
                const float ce = px.c[j] * e.e.v[j], oms = 1.f - e.S[j];
                const float gS = gT * (e.spec[j] - px.ommu * ce);        // T = (1 - S)(1 - mu) c E + S spec
                g_ommu += gT * (oms * ce);
                gc[j] = gT * ((oms * px.ommu) * e.e.v[j]);
                gF0[j] = gS * e.A;                                       // S = F0 A + B
                gA += gS * px.F0[j];
                gB += gS;
            }
            // the look-ups: d spec / d (sc / a, tc / a, lod) and d E / d (sc / a, tc / a), each with what arrives at it
            const float w0 = 1.f - e.f;
            const bool two = e.f != 0.f;
            float gs_r = 0.f, gt_r = 0.f, gs_n = 0.f, gt_n = 0.f, g_lod = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gs_r += gspec[j] * (two ? w0 * e.s0.ds[j] + e.f * e.s1.ds[j] : e.s0.ds[j]);
                gt_r += gspec[j] * (two ? w0 * e.s0.dt[j] + e.f * e.s1.dt[j] : e.s0.dt[j]);
                g_lod += gspec[j] * (e.s1.v[j] - e.s0.v[j]);
                gs_n += girr[j] * e.e.ds[j];
                gt_n += girr[j] * e.e.dt[j];
            }
            float gR[3] = {0.f, 0.f, 0.f}, gn_raw[3] = {0.f, 0.f, 0.f};
            if (e.qr.valid) cube_direction_gradient(e.qr, gs_r, gt_r, gR);
            if (e.qn.valid) cube_direction_gradient(e.qn, gs_n, gt_n, gn_raw);
            float g_rho = (e.inside && e.qr.valid) ? g_lod * (float)(P.L - 1) : 0.f;
            g_rho += gA * e.A_rho + gB * e.B_rho;
            const float g_nv = gA * e.A_nv + gB * e.B_nv;
            // R = 2 nv_raw N - v, nv = max(nv_raw, 0), nv_raw = N . v
            const float g_nv_raw = 2.f * dot3(gR, px.N) + (px.nv_raw >= 0.f ? g_nv : 0.f);
            float gN[3], gvv[3], gtv[3], gn[3], gp[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gN[j] = (2.f * px.nv_raw) * gR[j] + g_nv_raw * px.v[j];
                gvv[j] = g_nv_raw * px.N[j] - gR[j];
            }
            unit3_backward(gvv, px.tv, px.len_v, px.inv_v, gtv);
            unit3_backward(gN, px.n, px.len_n, px.inv_n, gn);
            float gmu = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gn[j] += gn_raw[j];
                gp[j] = -gtv[j];
                if constexpr (PARAMS) acc[6 + j] += gtv[j];
                g_ommu += P.f0 * gF0[j];                  // F0 = f0 (1 - mu) + c mu
                gc[j] += gF0[j] * px.mu;
                gmu += gF0[j] * px.c[j];
            }
            gmu -= g_ommu;
            const float gr = (px.r >= P.min_roughness && px.r <= 1.f) ? g_rho : 0.f;   // closed at both edges; 0 at a NaN
            if (P.gcol) store3(P.gcol + pix * 3, gc);
            if (P.gmat) { P.gmat[pix * 2] = gr; P.gmat[pix * 2 + 1] = gmu; }
            if (P.s_dir) {
                store3(P.s_dir + pix * 3, e.R);
                P.s_lod[pix] = e.lod;
                store3(P.s_gspec + pix * 3, gspec);
                store3(P.s_girr + pix * 3, girr);
            }
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
            tile_rows_out<IBL_BLOCK, MATERIAL_ROW>(s_g, s_src, P.gg + ((long long)blockIdx.y * P.pixels + first) * Cg, npx, Cg, tid, walk);
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

// the floats of the partial rows in front of the per-pixel scratch
inline long long shade_ibl_partial_floats(long long scenes, long long pixels) { return scenes * shade_blocks(pixels, IBL_SPAN) * IBL_NP; }

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

// what this file's entry points refuse (the shared refusals, and `a`: dirt_shade_common.h)
static int shade_ibl_check(const char* who, const dirt::MaterialArgs& a, long long rows, long long cols, int size, int levels,
                           int irradiance_size, int table_size, dirt::ShadeIblParams& P)
{
    if (rows < 0 || cols < 0 || (rows > 0 && cols > (1ll << 40) / rows))
        STAGE_FAIL("%s: bad pixel grid (rows=%lld cols=%lld)", who, rows, cols);
    if (int rc = dirt::material_check_sizes(who, a, rows * cols)) return rc;
    if (int rc = dirt::material_check_layout(who, a)) return rc;
    if (size < 1 || size > 32768) STAGE_FAIL("%s: pyramid size %d, 1..32768", who, size);
    const int most = dirt::mip_level_count(size, size, -1);
    if (levels < 1 || levels > most) STAGE_FAIL("%s: %d levels, a %d x %d face has 1..%d", who, levels, size, size, most);
    if (irradiance_size < 1 || irradiance_size > 32768) STAGE_FAIL("%s: irradiance size %d, 1..32768", who, irradiance_size);
    if (table_size < 2 || table_size > DIRT_SHADE_IBL_MAX_TABLE)
        STAGE_FAIL("%s: table size %d, 2..%d", who, table_size, DIRT_SHADE_IBL_MAX_TABLE);
    if (int rc = dirt::material_check_scalars(who, a)) return rc;
    dirt::material_fill(P, a, rows * cols, dirt::IBL_NP);
    P.N = size; P.L = levels; P.M = irradiance_size; P.S = table_size;
    P.face_floats = dirt::cube_face_floats(size, levels, 3);
    return DIRT_OK;
}

size_t dirt_shade_ibl_scratch_bytes(long long scenes, long long rows, long long cols)
{
    if (scenes < 0 || scenes > 65535 || rows < 0 || cols < 0 || (rows > 0 && cols > (1ll << 40) / rows)) return 0;
    return sizeof(float) * (size_t)(dirt::shade_ibl_partial_floats(scenes, rows * cols) + scenes * rows * cols * dirt::IBL_PIXEL_FLOATS);
}

int dirt_shade_ibl_forward(const float* gbuffer, const float* colors, const float* material, const float* params, const float* pyramid,
                           const float* irradiance, const float* table, float* out, long long scenes, long long rows, long long cols,
                           int Cg, int color_stride, int material_stride, int off_colors, int off_material, int off_normals,
                           int off_positions, int off_mask, int param_scenes, int size, int levels, int irradiance_size, int table_size,
                           float min_roughness, float dielectric_f0, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_shade_ibl_forward";
    const dirt::MaterialArgs a{gbuffer, colors, material, scenes, Cg, color_stride, material_stride, off_colors, off_material, off_normals,
                               off_positions, off_mask, param_scenes, min_roughness, dielectric_f0, clamp_lo, clamp_hi, flags};
    dirt::ShadeIblParams P{};
    if (int rc = shade_ibl_check(who, a, rows, cols, size, levels, irradiance_size, table_size, P)) return rc;
    if (scenes * P.pixels == 0) return dirt::stage_ok(report);
    if (!gbuffer || !params || !out) STAGE_FAIL("%s: gbuffer / params / out is NULL", who);
    if (!pyramid || !irradiance || !table) STAGE_FAIL("%s: pyramid / irradiance / table is NULL", who);
    if (P.pixels > 0x7fffffffll * dirt::IBL_BLOCK) STAGE_FAIL("%s: too many pixels per scene", who);
    dirt::material_inputs(P, a);
    P.prm = params; P.pyr = pyramid; P.irr = irradiance; P.tab = table; P.out = out;
    const dim3 grid((unsigned)((P.pixels + dirt::IBL_BLOCK - 1) / dirt::IBL_BLOCK), (unsigned)scenes);
    hipLaunchKernelGGL(dirt::shade_ibl_forward_kernel, grid, dim3(dirt::IBL_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_shade_ibl_backward(const float* gbuffer, const float* colors, const float* material, const float* params, const float* pyramid,
                            const float* irradiance, const float* table, const float* grad_out, float* grad_gbuffer, float* grad_colors,
                            float* grad_material, float* grad_params, float* grad_pyramid, float* grad_irradiance, void* scratch,
                            size_t scratch_bytes, long long scenes, long long rows, long long cols, int Cg, int color_stride,
                            int material_stride, int off_colors, int off_material, int off_normals, int off_positions, int off_mask,
                            int param_scenes, int size, int levels, int irradiance_size, int table_size, float min_roughness,
                            float dielectric_f0, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_shade_ibl_backward";
    const dirt::MaterialArgs a{gbuffer, colors, material, scenes, Cg, color_stride, material_stride, off_colors, off_material, off_normals,
                               off_positions, off_mask, param_scenes, min_roughness, dielectric_f0, clamp_lo, clamp_hi, flags};
    dirt::ShadeIblParams P{};
    int rc = shade_ibl_check(who, a, rows, cols, size, levels, irradiance_size, table_size, P);
    if (!rc) rc = dirt::material_check_grads(who, a, grad_colors, grad_material);
    if (rc) return rc;
    const bool cubes = grad_pyramid || grad_irradiance;
    if (!grad_gbuffer && !grad_params && !grad_colors && !grad_material && !cubes) return dirt::stage_ok(report);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long n = scenes * P.pixels;
    if (n == 0) {   // no pixel adds to a cube: its gradient is zero
        hipError_t e = grad_pyramid ? dirt::clear_floats(grad_pyramid, 6 * P.face_floats, s) : hipSuccess;
        if (e == hipSuccess && grad_irradiance) e = dirt::clear_floats(grad_irradiance, 6ll * irradiance_size * irradiance_size * 3, s);
        return dirt::stage_hip(report, who, e);
    }
    if (!gbuffer || !params || !grad_out) STAGE_FAIL("%s: gbuffer / params / grad_out is NULL", who);
    if (!pyramid || !irradiance || !table) STAGE_FAIL("%s: pyramid / irradiance / table is NULL", who);
    if (grad_params || cubes) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_shade_ibl_scratch_bytes(scenes, rows, cols),
                                 "dirt_shade_ibl_scratch_bytes");
        if (rc) return rc;
    }
    const long long blocks = dirt::shade_blocks(P.pixels, dirt::IBL_SPAN);
    if (blocks > 0x7fffffffll) STAGE_FAIL("%s: too many pixels per scene", who);
    // the grid of the cubes' scatter: the scenes' images one below the other (a flat list: one row)
    const long long grid_rows = rows == 1 ? 1 : scenes * rows, grid_cols = rows == 1 ? n : cols;
    if (cubes && (dirt::tile_grid(grid_rows, grid_cols).tiles > 0x7fffffffll || grid_cols > 0x7fffffffll || grid_rows > 0x7fffffffll))
        STAGE_FAIL("%s: pixel grid too large (scenes=%lld rows=%lld cols=%lld)", who, scenes, rows, cols);
    dirt::material_inputs(P, a);
    P.prm = params; P.pyr = pyramid; P.irr = irradiance; P.tab = table;
    P.gout = grad_out; P.gg = grad_gbuffer; P.gcol = grad_colors; P.gmat = grad_material;
    P.partial = static_cast<float*>(scratch);
    if (cubes) {
        P.s_dir = static_cast<float*>(scratch) + dirt::shade_ibl_partial_floats(scenes, P.pixels);
        P.s_lod = P.s_dir + 3 * n; P.s_gspec = P.s_lod + n; P.s_girr = P.s_gspec + 3 * n;
    }
    const dim3 grid((unsigned)blocks, (unsigned)scenes);
    const bool params_wanted = grad_params != nullptr, gbuf = grad_gbuffer != nullptr;
    if (params_wanted && gbuf) hipLaunchKernelGGL((dirt::shade_ibl_backward_kernel<true, true>), grid, dim3(dirt::IBL_BLOCK), 0, s, P);
    else if (params_wanted) hipLaunchKernelGGL((dirt::shade_ibl_backward_kernel<true, false>), grid, dim3(dirt::IBL_BLOCK), 0, s, P);
    else if (gbuf) hipLaunchKernelGGL((dirt::shade_ibl_backward_kernel<false, true>), grid, dim3(dirt::IBL_BLOCK), 0, s, P);
    else hipLaunchKernelGGL((dirt::shade_ibl_backward_kernel<false, false>), grid, dim3(dirt::IBL_BLOCK), 0, s, P);
    rc = dirt::shade_backward_finish(who, scratch, grad_params, scenes, blocks, dirt::IBL_NP, param_scenes, s);
    if (rc) return rc;
    // the scatter into the two cubes, by the cube look-up's backward kernels (no gradient to a direction or to lod: this file's kernel made those)
    dirt::CubeParams c{};
    c.n = n; c.Ct = 3; c.grad_dirs = nullptr; c.grad_lod = nullptr; c.gdir_stride = 3; c.lod_bias = 0.f; c.flags = 0;
    hipError_t e = hipSuccess;
    if (grad_pyramid) {
        c.pyr = pyramid; c.dirs = P.s_dir; c.dir_stride = 3; c.lod = P.s_lod; c.N = size; c.L = levels; c.face_floats = P.face_floats;
        c.grad_out = P.s_gspec; c.grad_pyr = grad_pyramid;
        e = dirt::cube_backward_launch(c, grid_rows, grid_cols, s);
    }
    if (e == hipSuccess && grad_irradiance) {
        c.pyr = irradiance; c.dirs = gbuffer + off_normals; c.dir_stride = Cg; c.lod = nullptr; c.N = irradiance_size; c.L = 1;
        c.face_floats = dirt::cube_face_floats(irradiance_size, 1, 3);
        c.grad_out = P.s_girr; c.grad_pyr = grad_irradiance;
        e = dirt::cube_backward_launch(c, grid_rows, grid_cols, s);
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
