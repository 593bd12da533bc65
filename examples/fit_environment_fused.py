#!/usr/bin/env python3
"""Recovers an environment map from the image of a mirror-like sphere on dirt_amd (MI355X): the sphere is rendered through
`rasterise_deferred` into a 7-channel G-buffer (mask, normal, position); the shader reflects the view vector about the normal
in torch and looks the reflection up in a cube map with `texture.sample_texture_cube(..., filter='trilinear',
lod=roughness * (L - 1))`, so a rougher surface reads a blurrier level.  A short gradient descent on the cube's texels,
started from grey, brings the rendering back to that of a target environment.

    python examples/fit_environment_fused.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, matrices, texture  # noqa: E402

CAMERA = (0., 0., 3.)
SIZE = 16          # texels along a face's edge
LEVELS = 5         # of its mip pyramid: 16, 8, 4, 2, 1


def build_sphere(rings=16, segments=32):
    """A unit UV sphere -> (vertices [V, 3], faces [F, 3])"""
    vertices = []
    for r in range(rings + 1):
        theta = math.pi * r / rings
        for s in range(segments):
            phi = 2. * math.pi * s / segments
            vertices.append([math.sin(theta) * math.cos(phi), math.cos(theta), math.sin(theta) * math.sin(phi)])
    faces = []
    for r in range(rings):
        for s in range(segments):
            a, b = r * segments + s, r * segments + (s + 1) % segments
            c, d = a + segments, b + segments
            faces += [[a, b, d], [d, c, a]]
    return np.asarray(vertices, np.float32), np.asarray(faces, np.int32)


def texel_directions(size):
    """The direction of every texel centre of a cube [6, size, size, 3], faces in OpenGL order (the table of DESIGN.md §7)."""
    c = (torch.arange(size, dtype=torch.float32) + 0.5) * 2. / size - 1.
    tc, sc = torch.meshgrid(c, c, indexing='ij')
    one = torch.ones_like(sc)
    faces = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)]
    return torch.stack([torch.stack(f, -1) for f in faces])


def true_environment(size, device):
    """A sky: blue above, brown below, a warm sun towards (+1, +1, +1)."""
    d = torch.nn.functional.normalize(texel_directions(size), dim=-1)
    up = d[..., 1:2].clamp(-1., 1.)
    sky = torch.tensor([0.3, 0.5, 0.9]) * (0.5 + 0.5 * up) + torch.tensor([0.35, 0.25, 0.15]) * (0.5 - 0.5 * up)
    sun = (d @ torch.nn.functional.normalize(torch.tensor([1., 1., 1.]), dim=0)).clamp(min=0.)[..., None] ** 8
    return (sky + sun * torch.tensor([1.0, 0.8, 0.5])).to(device)


def render(environment, roughness, vertices, faces, width, height):
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
        lod = torch.full_like(mask[..., 0], roughness * (LEVELS - 1))
        # the background (mask 0) gets the direction (0, 0, 0): not a valid direction, so black, with no gradient
        return texture.sample_texture_cube(env, reflected * mask, filter='trilinear', lod=lod)

    return dirt.rasterise_deferred(background_attributes=torch.zeros([height, width, 7], device=dev), vertices=clip,
                                   vertex_attributes=attributes, faces=faces, shader_fn=shader_fn, shader_additional_inputs=[environment])


def fit(width=160, height=120, steps=60, rate=0.05, roughness=0.25, device=None):
    """-> (losses per step, mean |environment - truth| over the texels the sphere reflects, before and after)"""
    dev = device or torch.device('cuda', 0)
    vertices, faces = (torch.from_numpy(a).to(dev) for a in build_sphere())
    truth = true_environment(SIZE, dev)
    target = render(truth, roughness, vertices, faces, width, height).detach()
    environment = torch.full_like(truth, 0.5).requires_grad_(True)
    optimiser = torch.optim.Adam([environment], lr=rate)
    losses, seen = [], torch.zeros_like(truth, dtype=torch.bool)
    before = None
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(environment, roughness, vertices, faces, width, height) - target) ** 2).mean()
        loss.backward()
        seen |= environment.grad != 0
        if before is None:
            before = float((environment.detach() - truth).abs()[seen].mean())
        optimiser.step()
        losses.append(float(loss.detach()))
    return losses, before, float((environment.detach() - truth).abs()[seen].mean())


def main():
    losses, before, after = fit()
    print('losses: ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; |environment - truth| over the reflected texels %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))


if __name__ == '__main__':
    main()
