"""`import dirt` -- the reference's package name (dirt/__init__.py:1) on the MI355X-native implementation.

The reference's samples/ and tests/ say `import dirt`, `dirt.rasterise(...)`, `import dirt.rasterise_ops`,
`dirt.matrices`, `dirt.lighting`, `dirt.projection` (and, beyond the reference, `dirt.texture`, `dirt.shading`, `dirt.geometry`, `dirt.skinning`, `dirt.kinematics`, `dirt.blendshapes`); this package re-exports `dirt_amd` under those names so
such scripts run unchanged apart from TensorFlow -> torch tensors.  `dirt.shading` carries the fused G-buffer shaders
(`shade_gbuffer`, `shade_gbuffer_sh`, `shade_gbuffer_pbr` with `dirt.lighting.cook_torrance` as its per-vertex form, and
`shade_gbuffer_ibl` with `dirt.lighting.image_based_lighting` and the table of `dirt.lighting.environment_brdf`) and
`environment_background`, the environment seen behind the mesh (`dirt.lighting.environment_background` is its torch form),
and `resolve_image`, the last stage: supersample resolve, exposure, tone curve and sRGB encode (`dirt.lighting.resolve_image`);
`dirt.texture` the look-ups, by (u, v) (`sample_texture_uv`) and by direction into a cube map (`sample_texture_cube`),
the GGX-prefiltered environment pyramid (`prefilter_cube`, looked up by `sample_cube_pyramid`), and the resamplers between a
lat-long panorama and a cube map (`panorama_to_cube`, `cube_to_panorama`).
Tangent-space normal mapping is `dirt.geometry.vertex_tangents` (per-vertex frames from the uvs) and
`dirt.shading.perturb_normals` (the shading normal, written back into the G-buffer), with `dirt.lighting.vertex_tangents` and
`dirt.lighting.perturb_normals` as their pure-torch forms.
It contains no code of its own."""
import sys as _sys

import dirt_amd as _impl
from dirt_amd.rasterise_ops import rasterise, rasterise_batch, rasterise_deferred, rasterise_batch_deferred  # noqa: F401

for _name in ('rasterise_ops', 'matrices', 'lighting', 'projection', 'texture', 'shading', 'geometry', 'skinning', 'kinematics', 'blendshapes'):
    _module = getattr(_impl, _name)
    globals()[_name] = _module
    _sys.modules[__name__ + '.' + _name] = _module   # `import dirt.lighting` finds the same module object
del _name, _module
