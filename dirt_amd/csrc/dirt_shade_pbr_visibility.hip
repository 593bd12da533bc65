// dirt_shade_pbr_visibility.hip -- the second translation unit of dirt_shade_pbr.hip: its kernels with VIS = true (a factor per
// light and pixel, the output of dirt_shadow_forward, scales the light's weight; its gradient is written to a dense image) and
// the entry points dirt_shade_pbr_visibility_forward / _backward, below.  The kernels' source is one; it is compiled twice so
// that the 21 kernels without a visibility and these 17 build side by side.
#define DIRT_SHADE_PBR_VISIBILITY_UNIT 1
#include "dirt_shade_pbr.hip"

extern "C" {

// what they refuse beyond shade_pbr_check: a visibility needs a light to scale, and a pixel's factors lie side by side
static int shade_pbr_check_visibility(const char* who, int lights, int visibility_stride)
{
    if (lights == 0) STAGE_FAIL("%s: a visibility needs at least one light (dirt_shade_pbr_forward / _backward shade without one)", who);
    if (visibility_stride < lights) STAGE_FAIL("%s: visibility_stride=%d, a pixel's visibility is %d floats (one per light)", who, visibility_stride, lights);
    return DIRT_OK;
}

int dirt_shade_pbr_visibility_forward(const float* gbuffer, const float* colors, const float* material, const float* visibility,
                                      const float* params, float* out, long long scenes, long long pixels, int Cg, int color_stride,
                                      int material_stride, int visibility_stride, int off_colors, int off_material, int off_normals,
                                      int off_positions, int off_mask, int param_scenes, int lights, unsigned light_kinds,
                                      float min_roughness, float dielectric_f0, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_shade_pbr_visibility_forward";
    const dirt::MaterialArgs a{gbuffer, colors, material, scenes, Cg, color_stride, material_stride, off_colors, off_material, off_normals,
                               off_positions, off_mask, param_scenes, min_roughness, dielectric_f0, clamp_lo, clamp_hi, flags};
    dirt::ShadePbrVisParams P{};
    int rc = shade_pbr_check(who, a, pixels, lights, light_kinds, P);
    if (!rc) rc = shade_pbr_check_visibility(who, lights, visibility_stride);
    if (rc) return rc;
    if (scenes * pixels == 0) return dirt::stage_ok(report);
    if (!visibility) STAGE_FAIL("%s: visibility is NULL with pixels to shade", who);
    if (!gbuffer || !params || !out) STAGE_FAIL("%s: gbuffer / params / out is NULL", who);
    if (pixels > 0x7fffffffll * dirt::PBR_BLOCK) STAGE_FAIL("%s: too many pixels per scene", who);
    dirt::material_inputs(P, a);
    P.prm = params; P.out = out; P.vis = visibility; P.vstride = visibility_stride;
    const dim3 grid((unsigned)((pixels + dirt::PBR_BLOCK - 1) / dirt::PBR_BLOCK), (unsigned)scenes);
    hipLaunchKernelGGL(dirt::shade_visible_pbr_forward_kernel, grid, dim3(dirt::PBR_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_shade_pbr_visibility_backward(const float* gbuffer, const float* colors, const float* material, const float* visibility,
                                       const float* params, const float* grad_out, float* grad_gbuffer, float* grad_colors,
                                       float* grad_material, float* grad_visibility, float* grad_params, void* scratch, size_t scratch_bytes,
                                       long long scenes, long long pixels, int Cg, int color_stride, int material_stride,
                                       int visibility_stride, int off_colors, int off_material, int off_normals, int off_positions,
                                       int off_mask, int param_scenes, int lights, unsigned light_kinds, float min_roughness,
                                       float dielectric_f0, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_shade_pbr_visibility_backward";
    const dirt::MaterialArgs a{gbuffer, colors, material, scenes, Cg, color_stride, material_stride, off_colors, off_material, off_normals,
                               off_positions, off_mask, param_scenes, min_roughness, dielectric_f0, clamp_lo, clamp_hi, flags};
    dirt::ShadePbrVisParams P{};
    int rc = shade_pbr_check(who, a, pixels, lights, light_kinds, P);
    if (!rc) rc = shade_pbr_check_visibility(who, lights, visibility_stride);
    if (!rc) rc = dirt::material_check_grads(who, a, grad_colors, grad_material);
    if (rc) return rc;
    if (scenes * pixels == 0 || (!grad_gbuffer && !grad_params && !grad_colors && !grad_material && !grad_visibility)) return dirt::stage_ok(report);
    if (!visibility) STAGE_FAIL("%s: visibility is NULL with pixels to shade", who);
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
    P.vis = visibility; P.vstride = visibility_stride; P.gvis = grad_visibility;
    P.partial = static_cast<float*>(scratch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks, (unsigned)scenes);
    const bool params_wanted = grad_params != nullptr, gbuf = grad_gbuffer != nullptr;
    switch (lights) {
    case 1: dirt::shade_pbr_launch_backward<1>(P, params_wanted, gbuf, grid, s); break;
    case 2: dirt::shade_pbr_launch_backward<2>(P, params_wanted, gbuf, grid, s); break;
    case 3: dirt::shade_pbr_launch_backward<3>(P, params_wanted, gbuf, grid, s); break;
    default: dirt::shade_pbr_launch_backward<4>(P, params_wanted, gbuf, grid, s); break;
    }
    return dirt::shade_backward_finish(who, scratch, grad_params, scenes, blocks, DIRT_SHADE_PARAM_HEAD + DIRT_SHADE_PARAM_LIGHT * lights, param_scenes, s);
}

}  // extern "C"
