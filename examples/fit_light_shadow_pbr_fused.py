#!/usr/bin/env python3
"""Recovers the direction of a light from an image with a cast shadow on dirt_amd (MI355X), with the Cook-Torrance material:
the scene of fit_light_shadow_fused.py (a box above a floor under one directional light), its G-buffer two channels wider
(roughness, metalness), lit by one shader call -- `shading.shade_gbuffer_pbr(..., visibility=shading.shadow_visibility(...))`:
the shadowed light, the ambient term, the background and the clamp in one kernel forward and one backward.  A short descent on
the direction brings the rendering back to the target; the gradient reaches the direction through the light's term, through
the look-up (the light's matrix) and through the map that is drawn again in every step.

    python examples/fit_light_shadow_pbr_fused.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import matrices, shading  # noqa: E402
import fit_light_shadow_fused as shadow  # noqa: E402

LAYOUT = dict(mask=0, colors=1, normals=4, positions=7, material=10)
ROUGHNESS, METALNESS = 0.6, 0.
LIGHT_COLOR = (2.4, 2.4, 2.25)      # the diffuse lobe is albedo / pi: three times the Lambertian example's colour


def camera(width, height, device):
    """-> (world -> clip [4, 4], the camera's position in the world [3]): the view of fit_light_shadow_fused.py"""
    view = matrices.compose(matrices.rodrigues(torch.tensor([0., 0.5, 0.])), matrices.rodrigues(torch.tensor([-0.6, 0., 0.])),
                            matrices.translation(torch.tensor([0., -0.3, -7.])))
    position = torch.linalg.inv(view)[3, :3]     # row vectors: the origin of camera space, in the world
    return shadow.camera_matrix(width, height, device), position.to(device)


def render(direction, scene, width, height):
    vertices, faces, normals, colors = scene
    dev = vertices.device
    one = torch.ones_like(vertices[:, :1])
    projection, position = camera(width, height, dev)
    clip = torch.cat([vertices, one], dim=1) @ projection
    attributes = torch.cat([one, colors, normals, vertices, ROUGHNESS * one, METALNESS * one], dim=1)
    matrix = shadow.light_matrix(direction)
    shadow_map = shading.render_shadow_map(vertices, faces, matrix, shadow.MAP_SIZE, far=1.)
    background = torch.zeros([height, width, 12], device=dev)
    background[..., LAYOUT['normals'] + 2] = 1.      # a unit normal for the uncovered pixels (shade_gbuffer_pbr's docstring)

    def shader_fn(gbuffer, direction, shadow_map, matrix):
        visibility = shading.shadow_visibility(gbuffer, shadow_map[None], matrix[None], positions=LAYOUT['positions'], normals=LAYOUT['normals'],
                                               mask=LAYOUT['mask'], kernel=3, bias=shadow.BIAS, softness=shadow.SOFTNESS,
                                               normal_offset=shadow.NORMAL_OFFSET)
        return shading.shade_gbuffer_pbr(gbuffer, [shading.pbr_directional_light(direction, LIGHT_COLOR)], camera_position=position,
                                         ambient=shadow.AMBIENT, background=shadow.BACKGROUND, visibility=visibility, **LAYOUT)

    return dirt.rasterise_deferred(background_attributes=background, vertices=clip, vertex_attributes=attributes, faces=faces,
                                   shader_fn=shader_fn, shader_additional_inputs=[direction, shadow_map, matrix])


def fit(width=160, height=120, steps=60, rate=0.03, device=None):
    """-> (losses per step, the angle in degrees between the direction and the truth before, and after)"""
    dev = device or torch.device('cuda', 0)
    scene = tuple(torch.from_numpy(a).to(dev) for a in shadow.build_scene())
    truth = torch.tensor([0.45, -0.8, -0.35], device=dev)
    target = render(truth, scene, width, height).detach()
    direction = torch.tensor([0.15, -0.9, -0.1], device=dev, requires_grad=True)
    before = shadow.angle_between(direction.detach(), truth)
    optimiser = torch.optim.Adam([direction], lr=rate)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(direction, scene, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    return losses, before, shadow.angle_between(direction.detach(), truth)


def main():
    losses, before, after = fit()
    print('loss %.3e -> %.3e in %d steps; direction error %.1f -> %.1f degrees' % (losses[0], losses[-1], len(losses), before, after))


if __name__ == '__main__':
    main()
