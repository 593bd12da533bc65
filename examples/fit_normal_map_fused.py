#!/usr/bin/env python3
"""Recovers a normal map from an image on dirt_amd (MI355X): the textured cube of examples/textured.py with a 6-channel
texture (albedo, tangent-space normal map), lit by the two lights of examples/fit_material_fused.py through
`rasterise_deferred`.  Geometry is two kernels: `vertex_stage` (clip, world, normals) and `vertex_tangents` (the frames, from
the uvs).  The shader is three forward and three backward: `sample_texture_uv` looks the six channels up,
`shading.perturb_normals` reads `tex[..., 3:6]` in place and returns the G-buffer with the shading normal in its normal
channels, and `shading.shade_gbuffer_pbr` reads `tex[..., :3]` as colours -- no `torch.cat` anywhere (a 13-channel
G-buffer: mask, (u, v), normal, position, tangent and handedness).  A short descent on the normal-map texels, started
from the flat map (0.5, 0.5, 1), brings the rendering back to the target.

    python examples/fit_normal_map_fused.py
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import geometry as geom, lighting, matrices, shading, texture as tex  # noqa: E402
import textured  # noqa: E402  (examples/textured.py: the cube and its checker texture)

LAYOUT = dict(mask=0, normals=3, positions=6)
TANGENTS = 9
CHANNELS = 13
MATERIAL = (0.5, 0.1)     # roughness, metalness: constant here
LIGHT_DIRECTION = (0.5, -0.6, -0.6)
LIGHT_COLOR = (0.9, 0.8, 0.7)
POINT_LIGHT = ((-1.5, 2.5, 2.), (0.5, 0.45, 0.4))


def bumpy_texture(size=64):
    """[size, size, 6]: the checker albedo and the encoded normal map of a field of round bumps, 8 texels across"""
    y, x = np.mgrid[0:size, 0:size]
    albedo = textured.checker_texture(size) * 0.6 + 0.3
    height_x = 0.6 * np.cos(2. * np.pi * x / 8.)     # the height field's slopes
    height_y = 0.6 * np.cos(2. * np.pi * y / 8.)
    d = np.stack([-height_x, -height_y, np.ones_like(height_x)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.concatenate([albedo, (d + 1.) / 2.], -1).astype(np.float32)


def transforms(device):
    """-> (model, view_projection, the camera's world position [3]), the view of examples/fit_material_fused.py"""
    model = matrices.rodrigues(torch.tensor([0., 0.6, 0.], device=device))
    view = matrices.compose(matrices.translation(torch.tensor([0., -2., -3.2], device=device)),
                            matrices.rodrigues(torch.tensor([-0.5, 0., 0.], device=device)))
    projection = matrices.perspective_projection(near=0.1, far=20., right=0.1, aspect=0.75).to(device)
    camera = -(view[3, :3] @ view[:3, :3].t())   # row vectors, a rigid view x R + t: the camera sits at -t R^T
    return model, view @ projection, camera


def attributes_fused(vertices_object, uvs, topology, model, view_projection):
    """-> (clip [V, 4], vertex attributes [V, 13] = mask, (u, v), normal, world position, tangent and handedness): two kernels"""
    clip, world, normals = geom.vertex_stage(vertices_object, topology, model, view_projection)
    tangents = geom.vertex_tangents(world, normals, uvs, topology)
    return clip, torch.cat([torch.ones_like(world[:, :1]), uvs, normals, world[:, :3], tangents], dim=1)


def lights():
    return [shading.pbr_directional_light(LIGHT_DIRECTION, LIGHT_COLOR), shading.pbr_point_light(*POINT_LIGHT)]


def shader_fused(gbuffer, texture, camera):
    looked_up = tex.sample_texture_uv(texture, gbuffer[..., 1:3])
    bumped = shading.perturb_normals(gbuffer, looked_up[..., 3:6], normals=LAYOUT['normals'], tangents=TANGENTS)
    material = torch.tensor(MATERIAL, device=gbuffer.device).expand(tuple(gbuffer.shape[:-1]) + (2,))
    return shading.shade_gbuffer_pbr(bumped, lights(), colors=looked_up[..., :3], material=material, camera_position=camera,
                                     ambient=(0.05, 0.05, 0.05), background=(0., 0., 0.3), **LAYOUT)


def shader_torch(gbuffer, texture, camera):
    """the same with the frame in torch and a `torch.cat` back into the G-buffer: what `perturb_normals` replaces"""
    looked_up = tex.sample_texture_uv(texture, gbuffer[..., 1:3])
    n0 = LAYOUT['normals']
    normals = lighting.perturb_normals(gbuffer[..., n0:n0 + 3], gbuffer[..., TANGENTS:TANGENTS + 4], looked_up[..., 3:6])
    bumped = torch.cat([gbuffer[..., :n0], normals, gbuffer[..., n0 + 3:]], dim=-1)
    material = torch.tensor(MATERIAL, device=gbuffer.device).expand(tuple(gbuffer.shape[:-1]) + (2,))
    return shading.shade_gbuffer_pbr(bumped, lights(), colors=looked_up[..., :3], material=material, camera_position=camera,
                                     ambient=(0.05, 0.05, 0.05), background=(0., 0., 0.3), **LAYOUT)


def background_attributes(height, width, device):
    """What an uncovered pixel holds: mask 0, a unit normal (examples/fit_material_fused.py) and no tangent, which
    `perturb_normals` answers by leaving the normal as it is."""
    attributes = torch.zeros([height, width, CHANNELS], device=device)
    attributes[..., LAYOUT['normals'] + 2] = 1.
    return attributes


def render(vertices_object, uvs, topology, texture, width, height, fused=True):
    model, view_projection, camera = transforms(vertices_object.device)
    clip, attributes = attributes_fused(vertices_object, uvs, topology, model, view_projection)
    return dirt.rasterise_deferred(vertices=clip, vertex_attributes=attributes, faces=topology.faces,
                                   background_attributes=background_attributes(height, width, clip.device),
                                   shader_fn=shader_fused if fused else shader_torch, shader_additional_inputs=[texture, camera])


def scene(device):
    """-> (object-space vertices [V, 3], uvs [V, 2], the cube's MeshTopology, the true texture [64, 64, 6])"""
    vertices, uvs, faces = (torch.from_numpy(a).to(device) for a in textured.build_cube())
    return vertices, uvs, geom.MeshTopology(faces, int(vertices.shape[0])), torch.from_numpy(bumpy_texture()).to(device)


def fit(width=160, height=120, steps=40, rate=0.02, device=None):
    """-> (losses per step, |normal map - truth| before, after)"""
    dev = device or torch.device('cuda', 0)
    vertices, uvs, topology, truth = scene(dev)
    with torch.no_grad():
        target = render(vertices, uvs, topology, truth, width, height)
    bumps = torch.tensor([0.5, 0.5, 1.], device=dev).repeat(64, 64, 1).requires_grad_(True)
    before = float((bumps.detach() - truth[..., 3:]).norm())
    optimiser = torch.optim.Adam([bumps], lr=rate)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        texture = torch.cat([truth[..., :3], bumps], dim=-1)     # (of texels, once per step: not of pixels)
        loss = ((render(vertices, uvs, topology, texture, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        with torch.no_grad():
            bumps.clamp_(0., 1.)
        losses.append(float(loss.detach()))
    return losses, before, float((bumps.detach() - truth[..., 3:]).norm())


def main():
    losses, before, after = fit()
    print('loss %.3e -> %.3e in %d steps; |normal map - truth| %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))


if __name__ == '__main__':
    main()
