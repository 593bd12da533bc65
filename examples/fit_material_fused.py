#!/usr/bin/env python3
"""Recovers a metallic-roughness material from an image on dirt_amd (MI355X): the textured cube of examples/textured.py with
a 5-channel texture (albedo, roughness, metalness), lit by one directional and one point light through
`rasterise_deferred`.  The shader is two kernels forward and two backward: `sample_texture_uv` looks the five channels up, and
`shading.shade_gbuffer_pbr` reads `tex[..., :3]` as colours and `tex[..., 3:5]` as material in place (a 9-channel G-buffer:
mask, (u, v), normal, position).  A short descent on the texture and on the directional light's colour, started from a grey,
half-rough dielectric, brings the rendering back to the target.

    python examples/fit_material_fused.py
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, matrices, shading, texture as tex  # noqa: E402
import textured  # noqa: E402  (examples/textured.py: the cube and its checker texture)

LAYOUT = dict(mask=0, normals=3, positions=6)
LIGHT_DIRECTION = (0.5, -0.6, -0.6)
POINT_LIGHT = ((-1.5, 2.5, 2.), (0.5, 0.45, 0.4))
TRUE_COLOR = (0.9, 0.8, 0.7)


def material_texture(size=64):
    """[size, size, 5]: the checker albedo, a roughness ramp from 0.3 to 0.9, metal stripes"""
    y, x = np.mgrid[0:size, 0:size]
    albedo = textured.checker_texture(size) * 0.8 + 0.1
    roughness = 0.3 + 0.6 * (y / (size - 1.))
    metalness = ((x // 8) % 2).astype(np.float32) * 0.8 + 0.1
    return np.concatenate([albedo, roughness[..., None], metalness[..., None]], -1).astype(np.float32)


def geometry(vertices_object, uvs, faces):
    """-> (clip-space vertices [V, 4], vertex attributes [V, 9] = mask, (u, v), normal, world position, the camera's world position [3])"""
    dev = vertices_object.device
    v = torch.cat([vertices_object, torch.ones_like(vertices_object[:, -1:])], dim=1)
    world = v @ matrices.rodrigues(torch.tensor([0., 0.6, 0.], device=dev))
    normals = lighting.vertex_normals(world, faces)
    view = matrices.compose(matrices.translation(torch.tensor([0., -2., -3.2], device=dev)),
                            matrices.rodrigues(torch.tensor([-0.5, 0., 0.], device=dev)))
    clip = (world @ view) @ matrices.perspective_projection(near=0.1, far=20., right=0.1, aspect=0.75).to(dev)
    camera = -(view[3, :3] @ view[:3, :3].t())   # row vectors, a rigid view x R + t: the camera sits at -t R^T
    return clip, torch.cat([torch.ones_like(v[:, :1]), uvs, normals, world[:, :3]], dim=1), camera


def shader_fn(gbuffer, texture, light_color, camera):
    looked_up = tex.sample_texture_uv(texture, gbuffer[..., 1:3])
    lights = [shading.pbr_directional_light(LIGHT_DIRECTION, light_color), shading.pbr_point_light(*POINT_LIGHT)]
    return shading.shade_gbuffer_pbr(gbuffer, lights, colors=looked_up[..., :3], material=looked_up[..., 3:5], camera_position=camera,
                                     ambient=(0.05, 0.05, 0.05), background=(0., 0., 0.3), **LAYOUT)


def render(vertices_object, uvs, faces, texture, light_color, width, height):
    clip, attributes, camera = geometry(vertices_object, uvs, faces)
    return dirt.rasterise_deferred(vertices=clip, vertex_attributes=attributes, faces=faces,
                                   background_attributes=background_attributes(height, width, clip.device),
                                   shader_fn=shader_fn, shader_additional_inputs=[texture, light_color, camera])


def background_attributes(height, width, device):
    """What an uncovered pixel holds: mask 0 and a unit normal.  With a zero normal the model's D is a2 / 0 and the pixel inf * 0,
    in the fused shader as in `lighting.cook_torrance`, which the mask (a product) would not hide."""
    attributes = torch.zeros([height, width, 9], device=device)
    attributes[..., LAYOUT['normals'] + 2] = 1.
    return attributes


def fit(width=160, height=120, steps=40, rate=0.02, device=None):
    """-> (losses per step, |texture - truth| before, after)"""
    dev = device or torch.device('cuda', 0)
    vertices, uvs, faces = (torch.from_numpy(a).to(dev) for a in textured.build_cube())
    truth = torch.from_numpy(material_texture()).to(dev)
    with torch.no_grad():
        target = render(vertices, uvs, faces, truth, torch.tensor(TRUE_COLOR, device=dev), width, height)
    texture = torch.tensor([0.5, 0.5, 0.5, 0.6, 0.3], device=dev).repeat(64, 64, 1).requires_grad_(True)
    color = torch.full((3,), 0.6, device=dev, requires_grad=True)
    before = float((texture.detach() - truth).norm())
    optimiser = torch.optim.Adam([texture, color], lr=rate)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(vertices, uvs, faces, texture, color, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        with torch.no_grad():
            texture.clamp_(0., 1.)
        losses.append(float(loss.detach()))
    return losses, before, float((texture.detach() - truth).norm())


def main():
    losses, before, after = fit()
    print('loss %.3e -> %.3e in %d steps; |texture - truth| %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))


if __name__ == '__main__':
    main()
