#!/usr/bin/env python3
"""Recovers an environment map from the image of a glossy sphere whose roughness varies over its surface, on dirt_amd (MI355X):
the sphere of fit_environment_fused.py, but the blur of a rough reflection is the GGX lobe of its roughness rather than a box
filter.  Every step `texture.prefilter_cube` turns the learnable cube into a pyramid whose level k is the environment convolved
with a GGX lobe of roughness k / (L - 1) (the specular half of split-sum image-based lighting), and the shader looks the
reflection up with `texture.sample_cube_pyramid(pyramid, reflected, roughness * (L - 1))`, per pixel.  The gradient reaches the
cube through the look-up, the transposed convolutions and the pyramid's collapse.

    python examples/fit_environment_prefiltered.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, matrices, texture  # noqa: E402
from fit_environment_fused import CAMERA, SIZE, build_sphere, true_environment  # noqa: E402


def render(environment, vertices, faces, width, height):
    dev = vertices.device
    view = matrices.translation(torch.tensor([-x for x in CAMERA], device=dev))
    projection = matrices.perspective_projection(near=0.1, far=20., right=0.05, aspect=float(height) / width).to(dev)
    v4 = torch.cat([vertices, torch.ones_like(vertices[:, :1])], dim=1)
    clip = (v4 @ view) @ projection
    attributes = torch.cat([torch.ones_like(vertices[:, :1]), lighting.vertex_normals(vertices, faces), vertices], dim=1)

    def shader_fn(gbuffer, env):
        mask, normals, positions = gbuffer[..., :1], torch.nn.functional.normalize(gbuffer[..., 1:4], dim=-1), gbuffer[..., 4:7]
        incident = positions - torch.tensor(CAMERA, device=dev)
        reflected = incident - 2. * (incident * normals).sum(-1, keepdim=True) * normals
        pyramid = texture.prefilter_cube(env)
        roughness = (0.35 + 0.3 * positions[..., 1]).clamp(0., 1.)       # polished at the bottom of the sphere, rough at its top
        # the background (mask 0) gets the direction (0, 0, 0): not a valid direction, so black, with no gradient
        return texture.sample_cube_pyramid(pyramid, reflected * mask, roughness * (pyramid.levels - 1))

    return dirt.rasterise_deferred(background_attributes=torch.zeros([height, width, 7], device=dev), vertices=clip,
                                   vertex_attributes=attributes, faces=faces, shader_fn=shader_fn, shader_additional_inputs=[environment])


def fit(width=160, height=120, steps=60, rate=0.05, device=None):
    """-> (losses per step, mean |environment - truth| over the texels, before and after)"""
    dev = device or torch.device('cuda', 0)
    vertices, faces = (torch.from_numpy(a).to(dev) for a in build_sphere())
    truth = true_environment(SIZE, dev)
    target = render(truth, vertices, faces, width, height).detach()
    environment = torch.full_like(truth, 0.5).requires_grad_(True)
    optimiser = torch.optim.Adam([environment], lr=rate)
    before = float((environment.detach() - truth).abs().mean())
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(environment, vertices, faces, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    return losses, before, float((environment.detach() - truth).abs().mean())


def main():
    losses, before, after = fit()
    print('losses: ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; mean |environment - truth| %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))


if __name__ == '__main__':
    main()
