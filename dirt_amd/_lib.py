"""ctypes binding of libdirt_hip.so (the C ABI declared in include/dirt_hip.h).

This is the counterpart of `tf.load_op_library(.../librasterise.so)` in the reference
(dirt/rasterise_ops.py:5-10).  Unlike the reference, which swallows a load failure with a warning and
leaves `_rasterise_module = None`, a missing or unloadable library raises as soon as an op is used:
there is no CPU or eager fallback behind these entry points.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DIRT_AMD_LIBRARY') or os.path.join(_HERE, 'libdirt_hip.so')  # override: instrumented builds (tools/)
ABI_VERSION = 4

FLAG_Q1_INTENDED = 1
FLAG_KEEP_STATE = 2
FLAG_REUSE_STATE = 4
FLAG_DENSE_FROM_STATE = 8   # backward: sum in the state's interleaved accumulators, copy out into the caller's dense tensors
FLAG_OUTPUTS_CLEARED = 0x10  # backward: the dense outputs are the ones dirt_rasterise_forward_train cleared (checked by the library)
FLAG_PROFILE = 0x100
FLAG_TILES_LARGE = 0x200
FLAG_TILES_SMALL = 0x400
FLAG_SHARED_FACES = 0x800
FLAG_GRAD_ROWS = 0x1000    # gradient kernel: every 8x8 block walks its own faces (default for small frames)
FLAG_GRAD_PAIRS = 0x2000   # ... or pairs of blocks share a face (default otherwise)
FLAG_GRAD_SMALL = 0x4000   # ... or the one-pixel-per-lane kernel on 16x16 tiles (default for small frames with 1, 3 or 4 channels)
FLAG_GRAD_PX2 = 0x8000    # ... or the two-pixels-per-lane kernel on 32x16 tiles (1, 3, 4 channels)
FLAG_GRAD_PX4 = 0x10000   # ... or the four-pixels-per-lane kernel where the library would choose px2
FLAG_GRAD_STREAM = 0x20000  # reserved: accepted and ignored (it pinned an experimental kernel, since removed)
TEX_CLAMP = 1
TEX_NEAREST = 2
ENVMAP_GGX, ENVMAP_LAMBERT = 0, 1   # the kind of dirt_envmap_filter_forward / _backward
SHADE_MAX_LIGHTS = 8
SHADE_PARAM_HEAD, SHADE_PARAM_LIGHT = 9, 8   # floats of the parameter block: ambient, background, camera; then per light
SHADE_KINDS = {'diffuse_directional': 0, 'specular_directional': 1, 'diffuse_point': 2}
SHADE_CLAMP = 1
SHADE_HAS_CAMERA = 2
SHADE_SH_NORMALIZE = 4
SHADE_SH_PARAMS = 30   # floats of the spherical-harmonic parameter block: 9 coefficients x 3 channels, then the background
SHADE_PBR_MAX_LIGHTS = 4
SHADE_PBR_KINDS = {'directional': 0, 'point': 1}   # the bit of a light in light_kinds
SHADE_IBL_MAX_TABLE = 128   # the largest environment-BRDF table of dirt_shade_ibl_forward
NORMAL_MAP_ENCODED = 1
SHADOW_MAX_LIGHTS = 4   # = SHADE_PBR_MAX_LIGHTS: the lights of dirt_shadow_forward, one map and one matrix each
SHADOW_KERNELS = (1, 3, 5)   # the sides of its percentage-closer filter
BACKGROUND_FILTERS = {'nearest': 0, 'bilinear': 1, 'trilinear': 2}   # the filter of dirt_background_forward
BACKGROUND_FOOTPRINT = 1   # its flag: the level of detail from the pixel's footprint
RESOLVE_MAX_FACTOR, RESOLVE_MAX_CHANNELS = 4, 4   # of dirt_resolve_forward
RESOLVE_CURVES = {'linear': 0, 'reinhard': 1, 'aces': 2}
RESOLVE_ENCODINGS = {'linear': 0, 'srgb': 1}
RESOLVE_CLAMP = 1
PANORAMA_MAX_SAMPLES = 4   # of dirt_panorama_to_cube_forward / dirt_cube_to_panorama_forward: samples x samples per texel
GEOM_PRE_SPLIT = 1
GEOM_LONG_LIST_SHIFT, GEOM_LONG_LIST_MASK, GEOM_LONG_LIST_DEFAULT = 8, 0xffff00, 64   # lists longer than this are summed by a wave
GEOM_MAX_VERTICES, GEOM_MAX_FACES = 1 << 28, 1 << 29
SKIN_MAX_INFLUENCES, SKIN_MAX_BONES, SKIN_LDS_BONES, SKIN_MAX_VERTICES, SKIN_MAX_ENTRIES = 8, 65536, 256, 1 << 28, 1 << 30   # up to SKIN_LDS_BONES the bone blocks are staged in LDS

KINEMATICS_MAX_JOINTS = 256   # = SKIN_LDS_BONES: a scene's joints live in LDS
BLEND_MAX_SHAPES, BLEND_MAX_VERTICES, BLEND_MAX_JOINTS, BLEND_MAX_ENTRIES = 4096, 1 << 26, 256, 1 << 30   # BLEND_MAX_JOINTS = KINEMATICS_MAX_JOINTS

E_INVALID_ARGUMENT = -1
E_TOO_MANY_VERTICES = -2
E_WORKSPACE = -3
E_HIP = -4

_lib = None

# every symbol include/dirt_hip.h declares (tests/test_boundary.py checks header <-> library)
SYMBOLS = ('dirt_abi_version', 'dirt_last_error', 'dirt_workspace_bytes', 'dirt_rasterise_forward', 'dirt_rasterise_forward_train',
           'dirt_rasterise_backward', 'dirt_rasterise_visibility', 'dirt_state_grad_buffers', 'dirt_profile_count',
           'dirt_profile_name',
           'dirt_profile_read', 'dirt_profile_reset', 'dirt_texture_sample_forward', 'dirt_texture_sample_backward',
           'dirt_texture_sample_backward_image', 'dirt_texture_last_error', 'dirt_texture_mip_levels', 'dirt_texture_mip_build',
           'dirt_texture_mip_collapse', 'dirt_texture_sample_mip_forward', 'dirt_texture_sample_mip_backward',
           'dirt_texture_sample_batch_forward', 'dirt_texture_sample_batch_backward_image', 'dirt_texture_mip_build_batch',
           'dirt_texture_mip_collapse_batch', 'dirt_texture_sample_mip_batch_forward', 'dirt_texture_sample_mip_batch_backward',
           'dirt_texture_cube_forward', 'dirt_texture_cube_backward', 'dirt_envmap_filter_forward', 'dirt_envmap_filter_backward',
           'dirt_shade_scratch_bytes', 'dirt_shade_forward', 'dirt_shade_backward', 'dirt_shade_albedo_forward', 'dirt_shade_albedo_backward',
           'dirt_shade_sh_scratch_bytes', 'dirt_shade_sh_forward', 'dirt_shade_sh_backward',
           'dirt_shade_pbr_scratch_bytes', 'dirt_shade_pbr_forward', 'dirt_shade_pbr_backward',
           'dirt_shade_pbr_visibility_forward', 'dirt_shade_pbr_visibility_backward',
           'dirt_shade_ibl_scratch_bytes', 'dirt_shade_ibl_forward', 'dirt_shade_ibl_backward',
           'dirt_geometry_scratch_bytes', 'dirt_geometry_forward', 'dirt_geometry_backward',
           'dirt_skin_scratch_bytes', 'dirt_skin_forward', 'dirt_skin_backward',
           'dirt_kinematics_scratch_bytes', 'dirt_kinematics_forward', 'dirt_kinematics_backward',
           'dirt_blend_scratch_bytes', 'dirt_blend_forward', 'dirt_blend_backward',
           'dirt_tangent_scratch_bytes', 'dirt_tangent_forward', 'dirt_tangent_backward',
           'dirt_normal_map_forward', 'dirt_normal_map_backward',
           'dirt_shadow_scratch_bytes', 'dirt_shadow_forward', 'dirt_shadow_backward',
           'dirt_background_scratch_bytes', 'dirt_background_forward', 'dirt_background_backward',
           'dirt_resolve_scratch_bytes', 'dirt_resolve_forward', 'dirt_resolve_backward',
           'dirt_panorama_scratch_bytes', 'dirt_panorama_to_cube_forward', 'dirt_panorama_to_cube_backward',
           'dirt_cube_to_panorama_forward', 'dirt_cube_to_panorama_backward')


class DirtLibraryError(RuntimeError):
    pass


def load():
    """dlopen libdirt_hip.so and declare the prototypes.  Raises DirtLibraryError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DirtLibraryError(
            'libdirt_hip.so is missing (%s): build it with `python -m dirt_amd.build` (hipcc, gfx950). '
            'dirt_amd has no fallback path.' % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise DirtLibraryError('failed to load %s: %s' % (LIB_PATH, e))
    vp, fp, ip = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p  # raw device addresses
    i, sz, u = ctypes.c_int, ctypes.c_size_t, ctypes.c_uint
    lib.dirt_abi_version.restype = i
    lib.dirt_last_error.restype = ctypes.c_char_p
    lib.dirt_workspace_bytes.argtypes = [i] * 6
    lib.dirt_workspace_bytes.restype = sz
    lib.dirt_rasterise_forward.argtypes = [fp, fp, fp, ip, fp, i, i, i, i, i, i, vp, sz, u, vp]
    lib.dirt_rasterise_forward.restype = i
    lib.dirt_rasterise_forward_train.argtypes = [fp, fp, fp, ip, fp, fp, fp, i, i, i, i, i, i, vp, sz, u, vp]
    lib.dirt_rasterise_forward_train.restype = i
    lib.dirt_rasterise_backward.argtypes = [fp, ip, fp, fp, fp, fp, fp, fp, i, i, i, i, i, i, vp, sz, u, vp]
    lib.dirt_rasterise_backward.restype = i
    lib.dirt_rasterise_visibility.argtypes = [fp, ip, ip, i, i, i, i, i, vp, sz, u, vp]
    lib.dirt_rasterise_visibility.restype = i
    lib.dirt_state_grad_buffers.argtypes = [vp, sz, i, i, i, i, i, i, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                            ctypes.POINTER(i), ctypes.POINTER(i)]
    lib.dirt_state_grad_buffers.restype = i
    lib.dirt_profile_count.restype = i
    lib.dirt_profile_name.argtypes = [i]
    lib.dirt_profile_name.restype = ctypes.c_char_p
    lib.dirt_profile_read.argtypes = [i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]
    lib.dirt_profile_read.restype = i
    lib.dirt_profile_reset.restype = i
    ll = ctypes.c_longlong
    lib.dirt_texture_sample_forward.argtypes = [fp, fp, fp, ll, i, i, i, i, u, vp]
    lib.dirt_texture_sample_forward.restype = i
    lib.dirt_texture_sample_backward.argtypes = [fp, fp, fp, fp, fp, ll, i, i, i, i, i, u, vp]
    lib.dirt_texture_sample_backward.restype = i
    override = bool(os.environ.get('DIRT_AMD_LIBRARY'))   # an A/B build of another round (tools/): older ABIs are let through
    if hasattr(lib, 'dirt_texture_sample_backward_image') or not override:
        lib.dirt_texture_sample_backward_image.argtypes = [fp, fp, fp, fp, fp, ll, ll, i, i, i, i, i, u, vp]
        lib.dirt_texture_sample_backward_image.restype = i
    lib.dirt_texture_last_error.restype = ctypes.c_char_p
    if hasattr(lib, 'dirt_texture_mip_levels') or not override:   # trilinear look-up (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_texture_mip_levels.argtypes = [i, i, i, i, ctypes.POINTER(ll)]
        lib.dirt_texture_mip_levels.restype = i
        lib.dirt_texture_mip_build.argtypes = [fp, fp, i, i, i, i, vp]
        lib.dirt_texture_mip_build.restype = i
        lib.dirt_texture_mip_collapse.argtypes = [fp, fp, i, i, i, i, vp]
        lib.dirt_texture_mip_collapse.restype = i
        lib.dirt_texture_sample_mip_forward.argtypes = [fp, fp, fp, fp, fp, ll, ll, i, i, i, i, i, i, i, f32, u, vp]
        lib.dirt_texture_sample_mip_forward.restype = i
        lib.dirt_texture_sample_mip_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, fp, fp, ll, ll, i, i, i, i, i, i, i, i, f32, u, vp]
        lib.dirt_texture_sample_mip_backward.restype = i
    if hasattr(lib, 'dirt_texture_sample_batch_forward') or not override:   # a texture per scene (ABI 4, additive): `scenes` after the pointers
        f32 = ctypes.c_float
        lib.dirt_texture_sample_batch_forward.argtypes = [fp, fp, fp, ll, ll, i, i, i, i, u, vp]
        lib.dirt_texture_sample_batch_forward.restype = i
        lib.dirt_texture_sample_batch_backward_image.argtypes = [fp, fp, fp, fp, fp, ll, ll, ll, i, i, i, i, i, u, vp]
        lib.dirt_texture_sample_batch_backward_image.restype = i
        lib.dirt_texture_mip_build_batch.argtypes = [fp, fp, ll, i, i, i, i, vp]
        lib.dirt_texture_mip_build_batch.restype = i
        lib.dirt_texture_mip_collapse_batch.argtypes = [fp, fp, ll, i, i, i, i, vp]
        lib.dirt_texture_mip_collapse_batch.restype = i
        lib.dirt_texture_sample_mip_batch_forward.argtypes = [fp, fp, fp, fp, fp, ll, ll, ll, i, i, i, i, i, i, i, f32, u, vp]
        lib.dirt_texture_sample_mip_batch_forward.restype = i
        lib.dirt_texture_sample_mip_batch_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, fp, fp, ll, ll, ll, i, i, i, i, i, i, i, i, f32, u, vp]
        lib.dirt_texture_sample_mip_batch_backward.restype = i
    if hasattr(lib, 'dirt_texture_cube_forward') or not override:   # cube-map look-up (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_texture_cube_forward.argtypes = [fp, fp, fp, fp, ll, i, i, i, i, f32, u, vp]
        lib.dirt_texture_cube_forward.restype = i
        lib.dirt_texture_cube_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, ll, ll, i, i, i, i, i, f32, u, vp]
        lib.dirt_texture_cube_backward.restype = i
    if hasattr(lib, 'dirt_envmap_filter_forward') or not override:   # environment prefilter (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_envmap_filter_forward.argtypes = [fp, fp, fp, i, i, ll, f32, u, vp]
        lib.dirt_envmap_filter_forward.restype = i
        lib.dirt_envmap_filter_backward.argtypes = [fp, fp, fp, i, i, ll, f32, u, vp]
        lib.dirt_envmap_filter_backward.restype = i
    if hasattr(lib, 'dirt_shade_forward') or not override:   # fused G-buffer lighting (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_shade_scratch_bytes.argtypes = [ll, ll, i]
        lib.dirt_shade_scratch_bytes.restype = sz
        lib.dirt_shade_forward.argtypes = [fp, fp, fp, ll, ll, i, i, i, i, i, i, i, u, u, f32, f32, u, vp]
        lib.dirt_shade_forward.restype = i
        lib.dirt_shade_backward.argtypes = [fp, fp, fp, fp, fp, vp, sz, ll, ll, i, i, i, i, i, i, i, u, u, f32, f32, u, vp]
        lib.dirt_shade_backward.restype = i
    if hasattr(lib, 'dirt_shade_albedo_forward') or not override:   # ... with the colours in an image of their own (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_shade_albedo_forward.argtypes = [fp, fp, fp, fp, ll, ll, i, i, i, i, i, i, i, u, u, f32, f32, u, vp]
        lib.dirt_shade_albedo_forward.restype = i
        lib.dirt_shade_albedo_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, vp, sz, ll, ll, i, i, i, i, i, i, i, u, u, f32, f32, u, vp]
        lib.dirt_shade_albedo_backward.restype = i
    if hasattr(lib, 'dirt_shade_sh_forward') or not override:   # spherical-harmonic G-buffer lighting (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_shade_sh_scratch_bytes.argtypes = [ll, ll]
        lib.dirt_shade_sh_scratch_bytes.restype = sz
        lib.dirt_shade_sh_forward.argtypes = [fp, fp, fp, fp, ll, ll, i, i, i, i, i, i, f32, f32, f32, f32, f32, u, vp]
        lib.dirt_shade_sh_forward.restype = i
        lib.dirt_shade_sh_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, vp, sz, ll, ll, i, i, i, i, i, i, f32, f32, f32, f32, f32, u, vp]
        lib.dirt_shade_sh_backward.restype = i
    if hasattr(lib, 'dirt_shade_pbr_forward') or not override:   # Cook-Torrance G-buffer lighting (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_shade_pbr_scratch_bytes.argtypes = [ll, ll, i]
        lib.dirt_shade_pbr_scratch_bytes.restype = sz
        lib.dirt_shade_pbr_forward.argtypes = [fp, fp, fp, fp, fp, ll, ll] + [i] * 10 + [u, f32, f32, f32, f32, u, vp]
        lib.dirt_shade_pbr_forward.restype = i
        lib.dirt_shade_pbr_backward.argtypes = [fp] * 9 + [vp, sz, ll, ll] + [i] * 10 + [u, f32, f32, f32, f32, u, vp]
        lib.dirt_shade_pbr_backward.restype = i
    if hasattr(lib, 'dirt_shade_pbr_visibility_forward') or not override:   # ... with a visibility per light (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_shade_pbr_visibility_forward.argtypes = [fp] * 6 + [ll, ll] + [i] * 11 + [u, f32, f32, f32, f32, u, vp]
        lib.dirt_shade_pbr_visibility_forward.restype = i
        lib.dirt_shade_pbr_visibility_backward.argtypes = [fp] * 11 + [vp, sz, ll, ll] + [i] * 11 + [u, f32, f32, f32, f32, u, vp]
        lib.dirt_shade_pbr_visibility_backward.restype = i
    if hasattr(lib, 'dirt_shade_ibl_forward') or not override:   # image-based G-buffer lighting (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_shade_ibl_scratch_bytes.argtypes = [ll, ll, ll]
        lib.dirt_shade_ibl_scratch_bytes.restype = sz
        lib.dirt_shade_ibl_forward.argtypes = [fp] * 8 + [ll, ll, ll] + [i] * 13 + [f32, f32, f32, f32, u, vp]
        lib.dirt_shade_ibl_forward.restype = i
        lib.dirt_shade_ibl_backward.argtypes = [fp] * 14 + [vp, sz, ll, ll, ll] + [i] * 13 + [f32, f32, f32, f32, u, vp]
        lib.dirt_shade_ibl_backward.restype = i
    if hasattr(lib, 'dirt_geometry_forward') or not override:   # fused vertex stage (ABI 4, additive)
        lib.dirt_geometry_scratch_bytes.argtypes = [ll, ll, ll]
        lib.dirt_geometry_scratch_bytes.restype = sz
        lib.dirt_geometry_forward.argtypes = [fp, i, ip, ip, ip, fp, i, fp, i, fp, fp, fp, ll, ll, ll, u, vp]
        lib.dirt_geometry_forward.restype = i
        lib.dirt_geometry_backward.argtypes = [fp, i, ip, ip, ip, fp, i, fp, i, fp, fp, fp, fp, fp, fp, vp, sz, ll, ll, ll, u, vp]
        lib.dirt_geometry_backward.restype = i
    if hasattr(lib, 'dirt_skin_forward') or not override:   # fused linear-blend skinning (ABI 4, additive)
        lib.dirt_skin_scratch_bytes.argtypes = [ll, ll]
        lib.dirt_skin_scratch_bytes.restype = sz
        lib.dirt_skin_forward.argtypes = [fp, i, i, ip, fp, fp, i, fp, ll, ll, i, i, u, vp]
        lib.dirt_skin_forward.restype = i
        lib.dirt_skin_backward.argtypes = [fp, i, i, ip, fp, fp, i, ip, ip, ip, fp, fp, fp, fp, vp, sz, ll, ll, i, i, ll, u, vp]
        lib.dirt_skin_backward.restype = i
    if hasattr(lib, 'dirt_kinematics_forward') or not override:   # fused forward kinematics (ABI 4, additive)
        lib.dirt_kinematics_scratch_bytes.argtypes = [ll, ll]
        lib.dirt_kinematics_scratch_bytes.restype = sz
        lib.dirt_kinematics_forward.argtypes = [fp, i, fp, i, ip, ip, ip, i, fp, fp, ll, i, u, vp]
        lib.dirt_kinematics_forward.restype = i
        lib.dirt_kinematics_backward.argtypes = [fp, i, fp, i, ip, ip, ip, i, ip, ip, fp, fp, fp, fp, vp, sz, ll, i, u, vp]
        lib.dirt_kinematics_backward.restype = i
    if hasattr(lib, 'dirt_blend_forward') or not override:   # fused blend shapes (ABI 4, additive)
        lib.dirt_blend_scratch_bytes.argtypes = [ll, ll, ll]
        lib.dirt_blend_scratch_bytes.restype = sz
        lib.dirt_blend_forward.argtypes = [fp, i, fp, i, fp, ll, ip, ip, fp, fp, fp, fp, ll, ll, i, i, i, u, vp]
        lib.dirt_blend_forward.restype = i
        lib.dirt_blend_backward.argtypes = [i, i, fp, ll, ip, ip, fp, fp, fp, fp, fp, fp, vp, sz, ll, ll, i, i, i, u, vp]
        lib.dirt_blend_backward.restype = i
    if hasattr(lib, 'dirt_tangent_forward') or not override:   # tangent-space normal mapping (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_tangent_scratch_bytes.argtypes = [ll, ll, ll]
        lib.dirt_tangent_scratch_bytes.restype = sz
        lib.dirt_tangent_forward.argtypes = [fp, i, fp, fp, ip, ip, ip, fp, ll, ll, ll, vp]
        lib.dirt_tangent_forward.restype = i
        lib.dirt_tangent_backward.argtypes = [fp, i, fp, fp, ip, ip, ip, fp, fp, fp, vp, sz, ll, ll, ll, vp]
        lib.dirt_tangent_backward.restype = i
        lib.dirt_normal_map_forward.argtypes = [fp, fp, fp, ll, ll, i, i, i, i, f32, u, vp]
        lib.dirt_normal_map_forward.restype = i
        lib.dirt_normal_map_backward.argtypes = [fp, fp, fp, fp, fp, ll, ll, i, i, i, i, f32, u, vp]
        lib.dirt_normal_map_backward.restype = i
    if hasattr(lib, 'dirt_shadow_forward') or not override:   # shadow-map look-up (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_shadow_scratch_bytes.argtypes = [ll, ll, ll, i]
        lib.dirt_shadow_scratch_bytes.restype = sz
        lib.dirt_shadow_forward.argtypes = [fp] * 4 + [ll, ll] + [i] * 10 + [f32, f32, f32, vp]
        lib.dirt_shadow_forward.restype = i
        lib.dirt_shadow_backward.argtypes = [fp] * 7 + [vp, sz, ll, ll, ll] + [i] * 10 + [f32, f32, f32, vp]
        lib.dirt_shadow_backward.restype = i
    if hasattr(lib, 'dirt_background_forward') or not override:   # the environment behind the mesh (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_background_scratch_bytes.argtypes = [ll, ll, ll]
        lib.dirt_background_scratch_bytes.restype = sz
        lib.dirt_background_forward.argtypes = [fp] * 5 + [ll, ll, ll] + [i] * 7 + [f32, f32, u, vp]
        lib.dirt_background_forward.restype = i
        lib.dirt_background_backward.argtypes = [fp] * 9 + [vp, sz, ll, ll, ll] + [i] * 7 + [f32, f32, u, vp]
        lib.dirt_background_backward.restype = i
    if hasattr(lib, 'dirt_resolve_forward') or not override:   # resolve, tone map, encode (ABI 4, additive)
        f32 = ctypes.c_float
        lib.dirt_resolve_scratch_bytes.argtypes = [ll, ll, ll, i, i]
        lib.dirt_resolve_scratch_bytes.restype = sz
        lib.dirt_resolve_forward.argtypes = [fp] * 6 + [ll, ll, ll] + [i] * 10 + [f32, f32, u, vp]
        lib.dirt_resolve_forward.restype = i
        lib.dirt_resolve_backward.argtypes = [fp] * 8 + [vp, sz, ll, ll, ll] + [i] * 6 + [f32, f32, u, vp]
        lib.dirt_resolve_backward.restype = i
    if hasattr(lib, 'dirt_panorama_to_cube_forward') or not override:   # lat-long environment maps (ABI 4, additive)
        lib.dirt_panorama_scratch_bytes.argtypes = [ll, ll, i, i, i, i]
        lib.dirt_panorama_scratch_bytes.restype = sz
        for name in ('dirt_panorama_to_cube', 'dirt_cube_to_panorama'):
            getattr(lib, name + '_forward').argtypes = [fp] * 3 + [ll, ll, i, i, i, vp]
            getattr(lib, name + '_forward').restype = i
            getattr(lib, name + '_backward').argtypes = [fp] * 5 + [vp, sz, ll, ll, i, i, i, vp]
            getattr(lib, name + '_backward').restype = i
    if lib.dirt_abi_version() != ABI_VERSION and not override:
        raise DirtLibraryError('libdirt_hip.so ABI %d != expected %d' % (lib.dirt_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def last_error():
    return load().dirt_last_error().decode('utf-8', 'replace')


def check(rc):
    """Map a C-ABI return code to the exception the reference raises for the same condition:
    errors::InvalidArgument -> ValueError (csrc/rasterise_egl.cpp:302-316); HIP failures, which the
    reference turns into LOG(FATAL), -> RuntimeError."""
    if rc == 0:
        return
    msg = last_error()
    if rc in (E_INVALID_ARGUMENT, E_TOO_MANY_VERTICES, E_WORKSPACE):
        raise ValueError(msg)
    raise RuntimeError(msg)


def profile_reset():
    check(load().dirt_profile_reset())


def profile_read():
    """{kernel name: (total_ms, launches)} for calls made with FLAG_PROFILE on this thread."""
    lib = load()
    out = {}
    for slot in range(lib.dirt_profile_count()):
        ms, n = ctypes.c_double(0), ctypes.c_longlong(0)
        check(lib.dirt_profile_read(slot, ctypes.byref(ms), ctypes.byref(n)))
        out[lib.dirt_profile_name(slot).decode()] = (ms.value, n.value)
    return out
