"""The full text of what the fused stages refuse (`vertex_stage`, `skin_vertices`, `pose_skeleton`, `blend_shapes`,
`shade_gbuffer`, `shade_gbuffer_ibl`, and the texture look-up `sample_texture_uv` / `mip_pyramid`), and `to(device)` of their built-once index objects.  The stage test files match substrings of these
messages; this table pins every character, so that the code the wrappers share cannot change a text unnoticed.  Nothing here
needs the library or a GPU: every refusal comes from types, shapes, dtypes and devices alone.
"""
import pytest
import torch

from dirt_amd import blendshapes, geometry, kinematics, shading, skinning
from dirt_amd import texture as texture_module

TOPOLOGY = geometry.MeshTopology(torch.tensor([[0, 1, 2], [0, 2, 3]]), 4)                                  # V = 4, F = 2
SKIN = skinning.SkinWeights(torch.tensor([[0, 1], [1, 0], [0, 0]]), torch.full((3, 2), .5), 2)             # V = 3, K = 2, J = 2
SKELETON = kinematics.Skeleton([-1, 0, 0])                                                                 # J = 3
SHAPES = blendshapes.BlendShapes(torch.ones(4, 5, 3), torch.full((2, 5), .2), joint_shapes=3)              # K = 4, V = 5, J = 2

V4, V3, EYE = torch.zeros(4, 3), torch.zeros(3, 3), torch.eye(4)
T = torch.eye(4).repeat(2, 1, 1)             # bone transforms of SKIN
W = torch.full((3, 2), .5)                   # replacement weights of SKIN
R, P = torch.zeros(3, 3), torch.zeros(3, 3)  # rotations and joints of SKELETON
TEMPLATE, C = torch.zeros(5, 3), torch.zeros(4)
G = torch.zeros(4, 4, 10)
TEX, UV, UV_LIST = torch.zeros(8, 8, 3), torch.zeros(4, 5, 2), torch.zeros(5, 2)   # a texture, an image of look-ups, a flat list


def many(t):
    """65536 scenes of `t`, as a view: no memory"""
    return t[None].expand((65536,) + tuple(t.shape))


def shade_checks(gbuffer, lights=(), ambient=(0., 0., 0.)):
    """the checks of `shade_gbuffer` behind its device check, which every CPU tensor fails"""
    return shading._check_arguments(gbuffer, list(lights), 4, 7, 1, 0, ambient, None, (0., 0., 0.), (0., 1.))


RAMP = (0., 0.5, 1.)
G12 = torch.zeros(4, 5, 12)


def pyramid(floats=63, channels=3, levels=3, roughness=RAMP):
    return texture_module.CubePyramid(torch.zeros(6, floats), 4, channels, levels, roughness)


def ibl(g=G12, specular=pyramid(), irradiance=torch.zeros(6, 2, 2, 3), brdf=torch.zeros(8, 8, 2), **keywords):
    """`shade_gbuffer_ibl` through its public name: every check stands in front of its device check, which every CPU tensor fails"""
    arguments = dict(colors=4, material=10, normals=7, positions=1, mask=0, camera_position=(0., 0., 4.))
    arguments.update(keywords)
    return shading.shade_gbuffer_ibl(g, specular, irradiance, brdf, **arguments)


IBL_BRDF = 'shade_gbuffer_ibl expects brdf to be a floating-point tensor [S, S, 2] with 2 <= S <= 128 (lighting.environment_brdf), got %s'
IBL_IRRADIANCE = 'shade_gbuffer_ibl expects irradiance to be a floating-point tensor [6, size, size, 3], got %s'
IBL_REFUSALS = [   # (keywords of `ibl`, the text): in the order of the checks
    (dict(g=torch.zeros(5)), 'shade_gbuffer_ibl expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (5,)'),
    (dict(g=G12.to(torch.int32)), 'shade_gbuffer_ibl expects a float32 gbuffer, got torch.int32'),
    (dict(specular=torch.zeros(6, 63)), 'shade_gbuffer_ibl expects specular to be the CubePyramid of prefilter_cube, got Tensor'),
    (dict(specular=pyramid(roughness=None)),
     'shade_gbuffer_ibl: specular is a box-filtered pyramid (roughness None): the look-up at lod = roughness (L - 1) needs the levels '
     'prefilter_cube convolves'),
    (dict(specular=pyramid(roughness=(0., 0.25, 1.))),
     'shade_gbuffer_ibl: specular was filtered at the roughnesses (0.0, 0.25, 1.0), the look-up at lod = roughness (L - 1) needs the '
     'default ramp k / (L - 1) of prefilter_cube'),
    (dict(specular=pyramid(84, channels=4)), 'shade_gbuffer_ibl: specular has 4 channels, an environment has 3'),
    (dict(specular=pyramid(60)), 'shade_gbuffer_ibl: specular.packed must be [6, 63], the 3 levels of a 4 x 4 x 3 face, got (6, 60)'),
    (dict(specular=pyramid(levels=2, roughness=(0., 1.))),
     'shade_gbuffer_ibl: specular.packed must be [6, 60], the 2 levels of a 4 x 4 x 3 face, got (6, 63)'),
    (dict(irradiance=torch.zeros(6, 2, 3, 3)), IBL_IRRADIANCE % '(6, 2, 3, 3)'),
    (dict(irradiance=torch.zeros(6, 2, 2, 4)), IBL_IRRADIANCE % '(6, 2, 2, 4)'),
    (dict(brdf=torch.zeros(1, 1, 2)), IBL_BRDF % '(1, 1, 2)'),
    (dict(brdf=torch.zeros(129, 129, 2)), IBL_BRDF % '(129, 129, 2)'),
    (dict(brdf=torch.zeros(8, 8, 3)), IBL_BRDF % '(8, 8, 3)'),
    (dict(brdf=torch.zeros(8, 8, 2, device='meta')), 'brdf is on meta, the G-buffer on cpu'),
    (dict(irradiance=torch.zeros(6, 2, 2, 3, device='meta')), 'irradiance is on meta, the G-buffer on cpu'),
    (dict(colors=torch.zeros(4, 5, 4)), "colors as a tensor must have shape [4, 5, 3] (the G-buffer's [4, 5, 12] with 3 channels), got [4, 5, 4]"),
    (dict(material=None), 'material must be the index of a G-buffer channel, got None'),
    (dict(material=6), 'material (channel 6) overlaps colors (channel 4)'),
    (dict(positions=None), 'positions must be the index of a G-buffer channel, got None'),
    (dict(mask=12), 'mask at channel 12 does not fit in the 12 channels of the G-buffer'),
    (dict(min_roughness=0.), 'min_roughness must be a number > 0 and <= 1, got 0.0'),
    (dict(dielectric_f0=1.5), 'dielectric_f0 must be a number in [0, 1], got 1.5'),
    (dict(camera_position=None), 'shade_gbuffer_ibl needs camera_position'),
    (dict(clamp=(1., 0.)), 'clamp needs lo <= hi, got (1.0, 0.0)'),
    (dict(intensity=(1., 2.)), 'intensity must be 3 numbers, got 2'),
    (dict(intensity=torch.zeros(2, 3)), 'intensity must have shape [3], got [2, 3]'),
    (dict(background=torch.zeros(4)), 'background must have shape [3], got [4]'),
    # two faults: the earlier check speaks
    (dict(specular=pyramid(84, channels=4), brdf=torch.zeros(8, 8, 3)), 'shade_gbuffer_ibl: specular has 4 channels, an environment has 3'),
    (dict(irradiance=torch.zeros(6, 2, 3, 3), material=6), IBL_IRRADIANCE % '(6, 2, 3, 3)'),
    (dict(brdf=torch.zeros(8, 8, 2, device='meta'), colors=torch.zeros(4, 5, 4)), 'brdf is on meta, the G-buffer on cpu'),
    (dict(material=6, min_roughness=0.), 'material (channel 6) overlaps colors (channel 4)'),
    (dict(dielectric_f0=1.5, camera_position=None), 'dielectric_f0 must be a number in [0, 1], got 1.5'),
    (dict(camera_position=None, clamp=(1., 0.)), 'shade_gbuffer_ibl needs camera_position'),
]


def trilinear(texture=TEX, uvs=UV, **keywords):
    return texture_module.sample_texture_uv(texture, uvs, filter='trilinear', **keywords)


CPU = ' runs on an MI355X only; there is no CPU fallback'
REFUSALS = [
    # vertex_stage ----------------------------------------------------------------------------------------------------------
    (lambda: geometry.vertex_stage(torch.zeros(4, 2), TOPOLOGY), ValueError, 'vertex_stage expects vertices [V, 3|4] or [B, V, 3|4], got (4, 2)'),
    (lambda: geometry.vertex_stage(V4.numpy(), TOPOLOGY), ValueError, 'vertex_stage expects vertices [V, 3|4] or [B, V, 3|4], got (4, 3)'),
    (lambda: geometry.vertex_stage(V4.double(), TOPOLOGY), ValueError, 'vertex_stage expects float32 vertices, got torch.float64'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY.faces), ValueError, "vertex_stage expects a MeshTopology (build it once per mesh), got 'Tensor'"),
    (lambda: geometry.vertex_stage(torch.zeros(5, 3), TOPOLOGY), ValueError, 'vertex_stage: 5 vertices, the topology was built for 4'),
    (lambda: geometry.vertex_stage(many(V4), TOPOLOGY), ValueError, 'vertex_stage: 65536 scenes, at most 65535'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY.to('meta')), ValueError,
     'vertex_stage: the topology is on meta, the vertices on cpu (use topology.to(device))'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY, torch.zeros(3, 4)), ValueError, 'model must have shape [4, 4], got (3, 4)'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY, EYE.numpy()), ValueError, 'model must have shape [4, 4], got (4, 4)'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY, EYE, 3.), ValueError, 'view_projection must have shape [4, 4], got ()'),
    (lambda: geometry.vertex_stage(torch.zeros(2, 4, 3), TOPOLOGY, None, torch.zeros(3, 4, 4)), ValueError,
     'view_projection must have shape [4, 4] or [2, 4, 4], got (3, 4, 4)'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY, EYE.double()), ValueError, 'model must be float32, got torch.float64'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY, EYE, EYE.to('meta')), ValueError, 'view_projection is on meta, the vertices on cpu'),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY, want='clip'), ValueError, "want must be a sequence of ('clip', 'world', 'normals'), got 'clip'"),
    (lambda: geometry.vertex_stage(V4, TOPOLOGY, EYE, EYE), RuntimeError, 'dirt_amd.geometry.vertex_stage' + CPU),
    (lambda: geometry.MeshTopology(torch.tensor([[0, 1, 4]]), 4), ValueError, 'MeshTopology: faces name vertices 0..4, outside [0, 4)'),
    # skin_vertices ---------------------------------------------------------------------------------------------------------
    (lambda: skinning.skin_vertices(torch.zeros(3, 5), SKIN, T), ValueError, 'skin_vertices expects vertices [V, 3|4] or [B, V, 3|4], got (3, 5)'),
    (lambda: skinning.skin_vertices([V3], SKIN, T), ValueError, 'skin_vertices expects vertices [V, 3|4] or [B, V, 3|4], got ()'),
    (lambda: skinning.skin_vertices(V3.half(), SKIN, T), ValueError, 'skin_vertices expects float32 vertices, got torch.float16'),
    (lambda: skinning.skin_vertices(V3, [SKIN], T), ValueError, "skin_vertices expects a SkinWeights (build it once per mesh), got 'list'"),
    (lambda: skinning.skin_vertices(V4, SKIN, T), ValueError, 'skin_vertices: 4 vertices, the SkinWeights was built for 3'),
    (lambda: skinning.skin_vertices(V3, SKIN.to('meta'), T), ValueError,
     'skin_vertices: the SkinWeights is on meta, the vertices on cpu (use skin.to(device))'),
    (lambda: skinning.skin_vertices(V3, SKIN, torch.zeros(3, 4, 4)), ValueError,
     'bone_transforms must have shape [2, 4, 4] or [B, 2, 4, 4], got (3, 4, 4)'),
    (lambda: skinning.skin_vertices(V3, SKIN, T.numpy()), ValueError, 'bone_transforms must have shape [2, 4, 4] or [B, 2, 4, 4], got (2, 4, 4)'),
    (lambda: skinning.skin_vertices(V3, SKIN, T.double()), ValueError, 'bone_transforms must be float32, got torch.float64'),
    (lambda: skinning.skin_vertices(V3, SKIN, T.to('meta')), ValueError, 'bone_transforms is on meta, the vertices on cpu'),
    (lambda: skinning.skin_vertices(torch.zeros(2, 3, 3), SKIN, T[None].repeat(3, 1, 1, 1)), ValueError,
     'skin_vertices: 2 scenes of vertices, 3 of bone_transforms'),
    (lambda: skinning.skin_vertices(V3, SKIN, many(T)), ValueError, 'skin_vertices: 65536 scenes, at most 65535'),
    (lambda: skinning.skin_vertices(V3, SKIN, T, torch.zeros(3, 3)), ValueError, 'weights must have shape [3, 2], got (3, 3)'),
    (lambda: skinning.skin_vertices(V3, SKIN, T, W.numpy()), ValueError, 'weights must have shape [3, 2], got (3, 2)'),
    (lambda: skinning.skin_vertices(V3, SKIN, T, W.double()), ValueError, 'weights must be float32, got torch.float64'),
    (lambda: skinning.skin_vertices(V3, SKIN, T, W.to('meta')), ValueError, 'weights is on meta, the vertices on cpu'),
    (lambda: skinning.skin_vertices(V3, SKIN, T, W), RuntimeError, 'dirt_amd.skinning.skin_vertices' + CPU),
    (lambda: skinning.SkinWeights(torch.tensor([[-1, 2]]), torch.ones(1, 2), 2), ValueError,
     'SkinWeights: bone_indices name bones -1..2, outside [0, 2)'),
    # pose_skeleton ---------------------------------------------------------------------------------------------------------
    (lambda: kinematics.pose_skeleton(torch.zeros(2, 3), P, SKELETON), ValueError, 'rotations must have shape [3, 3] or [B, 3, 3], got (2, 3)'),
    (lambda: kinematics.pose_skeleton(R, torch.zeros(1, 1, 3, 3), SKELETON), ValueError,
     'joints must have shape [3, 3] or [B, 3, 3], got (1, 1, 3, 3)'),
    (lambda: kinematics.pose_skeleton(R.numpy(), P, SKELETON), ValueError, 'rotations must have shape [3, 3] or [B, 3, 3], got (3, 3)'),
    (lambda: kinematics.pose_skeleton(R.double(), P, SKELETON), ValueError, 'rotations must be float32, got torch.float64'),
    (lambda: kinematics.pose_skeleton(R, P.half(), SKELETON), ValueError, 'joints must be float32, got torch.float16'),
    (lambda: kinematics.pose_skeleton(R, P.to('meta'), SKELETON), ValueError, 'joints is on meta, the rotations on cpu'),
    (lambda: kinematics.pose_skeleton(R, P, SKELETON.to('meta')), ValueError,
     'pose_skeleton: the Skeleton is on meta, the rotations on cpu (use skeleton.to(device))'),
    (lambda: kinematics.pose_skeleton(R.to('meta'), P.to('meta'), SKELETON), ValueError,
     'pose_skeleton: the Skeleton is on cpu, the rotations on meta (use skeleton.to(device))'),
    (lambda: kinematics.pose_skeleton(R, P, [-1, 0, 0]), ValueError, "pose_skeleton expects a Skeleton (build it once per rig), got 'list'"),
    (lambda: kinematics.pose_skeleton(torch.zeros(2, 3, 3), torch.zeros(4, 3, 3), SKELETON), ValueError,
     'pose_skeleton: 2 scenes of rotations, 4 of joints'),
    (lambda: kinematics.pose_skeleton(many(R), P, SKELETON), ValueError, 'pose_skeleton: 65536 scenes, at most 65535'),
    (lambda: kinematics.pose_skeleton(R, P[None], SKELETON), RuntimeError, 'dirt_amd.kinematics.pose_skeleton' + CPU),
    # blend_shapes ----------------------------------------------------------------------------------------------------------
    (lambda: blendshapes.blend_shapes(torch.zeros(5, 4), C, SHAPES), ValueError, 'template must have shape [5, 3] or [B, 5, 3], got (5, 4)'),
    (lambda: blendshapes.blend_shapes(TEMPLATE.numpy(), C, SHAPES), ValueError, 'template must have shape [5, 3] or [B, 5, 3], got (5, 3)'),
    (lambda: blendshapes.blend_shapes(TEMPLATE.double(), C, SHAPES), ValueError, 'template must be float32, got torch.float64'),
    (lambda: blendshapes.blend_shapes(TEMPLATE, torch.zeros(2, 2, 4), SHAPES), ValueError, 'coefficients must have shape [4] or [B, 4], got (2, 2, 4)'),
    (lambda: blendshapes.blend_shapes(TEMPLATE, [0.] * 4, SHAPES), ValueError, 'coefficients must have shape [4] or [B, 4], got ()'),
    (lambda: blendshapes.blend_shapes(TEMPLATE, C.long(), SHAPES), ValueError, 'coefficients must be float32, got torch.int64'),
    (lambda: blendshapes.blend_shapes(TEMPLATE, C.to('meta'), SHAPES), ValueError, 'coefficients is on meta, the template on cpu'),
    (lambda: blendshapes.blend_shapes(TEMPLATE, C, SHAPES.to('meta')), ValueError,
     'blend_shapes: the BlendShapes is on meta, the template on cpu (use shapes.to(device))'),
    (lambda: blendshapes.blend_shapes(TEMPLATE, C, SHAPES.packed), ValueError, "blend_shapes expects a BlendShapes (build it once per model), got 'Tensor'"),
    (lambda: blendshapes.blend_shapes(torch.zeros(2, 5, 3), torch.zeros(3, 4), SHAPES), ValueError, 'blend_shapes: 2 scenes of template, 3 of coefficients'),
    (lambda: blendshapes.blend_shapes(TEMPLATE, many(C), SHAPES), ValueError, 'blend_shapes: 65536 scenes, at most 65535'),
    (lambda: blendshapes.blend_shapes(TEMPLATE[None], C, SHAPES), RuntimeError, 'dirt_amd.blendshapes.blend_shapes' + CPU),
    (lambda: blendshapes.pose_corrective_features(torch.zeros(3)), ValueError,
     'pose_corrective_features expects rotations [.., J, 3] with J >= 1, got (3,)'),
    # shade_gbuffer ---------------------------------------------------------------------------------------------------------
    (lambda: shading.shade_gbuffer(torch.zeros(5), [], colors=0, normals=3), ValueError,
     'shade_gbuffer expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (5,)'),
    (lambda: shading.shade_gbuffer(G.numpy(), [], colors=0, normals=3), ValueError,
     'shade_gbuffer expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (4, 4, 10)'),
    (lambda: shade_checks(G.int()), ValueError, 'shade_gbuffer expects a float32 gbuffer, got torch.int32'),
    (lambda: shade_checks(G, ambient=torch.zeros(3, device='meta')), ValueError, 'ambient is on meta, the G-buffer on cpu'),
    (lambda: shade_checks(G, [('diffuse_directional', torch.zeros(2, 3), (1., 1., 1.), True)]), ValueError,
     'light 0 direction must have shape [3], got [2, 3]'),
    (lambda: shade_checks(torch.zeros(2, 4, 4, 10), ambient=torch.zeros(3, 3)), ValueError, 'ambient must have shape [3] or [2, 3], got [3, 3]'),
    (lambda: shading.shade_gbuffer(G, [], colors=4, normals=7), RuntimeError, 'dirt_amd.shading.shade_gbuffer' + CPU),
    (lambda: shading.shade_gbuffer(G.to('meta'), [], colors=4, normals=7), RuntimeError, 'dirt_amd.shading.shade_gbuffer' + CPU),
    # sample_texture_uv, mip_pyramid: what both filters check, in the order they check it; then what 'trilinear' alone does --------
    (lambda: texture_module.sample_texture_uv(torch.zeros(8, 8), UV), ValueError,
     'sample_texture_uv expects texture to be 3D [height, width, channels], got shape (8, 8)'),
    (lambda: trilinear(torch.zeros(8, 8)), ValueError, 'sample_texture_uv expects texture to be 3D [height, width, channels], got shape (8, 8)'),
    (lambda: texture_module.sample_texture_uv(TEX, torch.zeros(4, 5, 3)), ValueError, 'sample_texture_uv expects uvs of shape [..., 2], got (4, 5, 3)'),
    (lambda: texture_module.sample_texture_uv(TEX, torch.zeros(()), filter='nearest'), ValueError, 'sample_texture_uv expects uvs of shape [..., 2], got ()'),
    (lambda: trilinear(uvs=torch.zeros(4, 5, 3)), ValueError, 'sample_texture_uv expects uvs of shape [..., 2], got (4, 5, 3)'),
    (lambda: texture_module.sample_texture_uv(TEX.to('meta'), UV), ValueError, 'texture and uvs must be on the same device (meta vs cpu)'),
    (lambda: trilinear(uvs=UV.to('meta')), ValueError, 'texture and uvs must be on the same device (cpu vs meta)'),
] + [
    (lambda filt=filt, kw=kw: texture_module.sample_texture_uv(TEX, UV_LIST, filter=filt, **kw), ValueError,
     "lod, lod_bias, mask and max_level apply to filter='trilinear' only (got filter=%r)" % filt)
    for filt in ('bilinear', 'nearest') for kw in ({'lod': torch.zeros(5)}, {'lod_bias': 1.0}, {'mask': torch.ones(5)}, {'max_level': 2})
] + [
    (lambda: trilinear(max_level=-1), ValueError, 'max_level must be a non-negative int or None, got -1'),
    (lambda: trilinear(max_level=True), ValueError, 'max_level must be a non-negative int or None, got True'),
    (lambda: trilinear(max_level=1.5), ValueError, 'max_level must be a non-negative int or None, got 1.5'),
    (lambda: trilinear(lod=torch.zeros(4, 4)), ValueError, 'lod must be a tensor shaped like uvs[..., 0] (4, 5), got (4, 4)'),
    (lambda: trilinear(mask=torch.ones(5, 4)), ValueError, 'mask must be a tensor shaped like uvs[..., 0] (4, 5), got (5, 4)'),
    (lambda: trilinear(lod=[[0.] * 5] * 4), ValueError, 'lod must be a tensor shaped like uvs[..., 0] (4, 5), got ()'),
    (lambda: trilinear(mask=torch.ones(4, 5).numpy()), ValueError, 'mask must be a tensor shaped like uvs[..., 0] (4, 5), got (4, 5)'),
    (lambda: trilinear(lod=torch.zeros(4, 5, device='meta')), ValueError, 'lod and uvs must be on the same device (meta vs cpu)'),
    (lambda: trilinear(mask=torch.ones(4, 5, device='meta')), ValueError, 'mask and uvs must be on the same device (meta vs cpu)'),
    (lambda: trilinear(uvs=UV_LIST), ValueError,
     "filter='trilinear' without lod takes the level of detail from neighbouring pixels: uvs must be images [..., H, W, 2], got (5, 2)"),
    (lambda: trilinear(lod=torch.zeros(4, 5), mask=torch.ones(4, 5)), ValueError,
     'mask marks the neighbours of the footprint level of detail; it does not apply with an explicit lod'),
    (lambda: texture_module.sample_texture_uv(TEX, UV), RuntimeError, 'dirt_amd.texture.sample_texture_uv' + CPU),
    (lambda: texture_module.sample_texture_uv(TEX, UV_LIST, 'clamp', 'nearest'), RuntimeError, 'dirt_amd.texture.sample_texture_uv' + CPU),
    (lambda: trilinear(), RuntimeError, 'dirt_amd.texture.sample_texture_uv' + CPU),
    (lambda: trilinear(uvs=UV_LIST, lod=torch.zeros(5), max_level=0), RuntimeError, 'dirt_amd.texture.sample_texture_uv' + CPU),
    (lambda: texture_module.mip_pyramid(TEX), RuntimeError, 'dirt_amd.texture.mip_pyramid' + CPU),
    (lambda: texture_module.mip_pyramid(torch.zeros(8, 8)), ValueError, 'mip_pyramid expects texture to be 3D [height, width, channels], got shape (8, 8)'),
    # shade_gbuffer_ibl (at the end: a row's number is part of its test's name) ------------------------------------------------
] + [(lambda kw=kw: ibl(**kw), ValueError, text) for kw, text in IBL_REFUSALS] + [
    (lambda: ibl(), RuntimeError, 'dirt_amd.shading.shade_gbuffer_ibl' + CPU),
]


@pytest.mark.parametrize('row', range(len(REFUSALS)), ids=lambda i: '%02d-%s' % (i, REFUSALS[i][2][:40].replace(' ', '_')))
def test_the_refusal_reads_exactly(row):
    call, kind, text = REFUSALS[row]
    with pytest.raises(kind) as raised:
        call()
    assert type(raised.value) is kind and str(raised.value) == text


INDEX_OBJECTS = [   # (the object, its tensors with the one `device` reads first, its scalar attributes)
    (TOPOLOGY, ('faces', 'offsets', 'entries'), ('num_vertices', 'num_faces')),
    (SKIN, ('bone_indices', 'bone_weights', 'entries', 'offsets', 'chunk_table', 'chunk_offsets'),
     ('num_vertices', 'num_bones', 'influences', 'chunk', 'num_chunks')),
    (SKELETON, ('parents', 'order', 'level_offsets', 'child_entries', 'child_offsets'), ('num_joints', 'num_levels')),
    (SHAPES, ('packed', 'row_offsets', 'row_vertices', 'row_weights', 'column_offsets', 'column_joints', 'column_weights', 'joint_directions'),
     ('num_shapes', 'num_vertices', 'num_joints', 'joint_shapes', 'stride')),
]


@pytest.mark.parametrize('index, tensors, scalars', INDEX_OBJECTS, ids=[type(row[0]).__name__ for row in INDEX_OBJECTS])
def test_to_moves_the_tensors_and_nothing_else(index, tensors, scalars):
    assert sorted(vars(index)) == sorted(tensors + scalars)      # the lists above name every attribute
    before = {name: getattr(index, name) for name in tensors}
    moved = index.to('meta')
    assert type(moved) is type(index) and moved is not index
    assert moved.device == getattr(moved, tensors[0]).device and moved.device.type == 'meta'
    assert index.device == getattr(index, tensors[0]).device and index.device.type == 'cpu'
    for name in tensors:
        there, here = getattr(moved, name), getattr(index, name)
        assert there.device.type == 'meta' and (there.shape, there.dtype) == (here.shape, here.dtype), name
        assert here is before[name] and here.device.type == 'cpu', name
    for name in scalars:
        assert getattr(moved, name) == getattr(index, name), name
    assert sorted(vars(moved)) == sorted(vars(index))            # every attribute went along, and none was added
    same = index.to('cpu')                                       # a copy of the object even where no tensor has to move
    assert type(same) is type(index) and same is not index and all(torch.equal(getattr(same, name), before[name]) for name in tensors)
