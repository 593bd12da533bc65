#!/usr/bin/env python3
"""Recovers spherical-harmonic lighting from an image on dirt_amd (MI355X): a sphere with a striped albedo is rendered under
known second-order SH coefficients through `rasterise_deferred` with `shading.shade_gbuffer_sh` as the shader (a 7-channel
G-buffer: mask, colour, normal), and a short gradient descent on the 27 coefficients, started from a grey ambient light,
brings the rendering back to the target.

    python examples/fit_sh_lighting_fused.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, matrices, shading  # noqa: E402

LAYOUT = dict(mask=0, colors=1, normals=4)
BACKGROUND = (0.1, 0.1, 0.2)


def build_sphere(rings=12, segments=24):
    """A unit UV sphere -> (vertices [V, 3], faces [F, 3], colours [V, 3]: stripes along the latitude)"""
    vertices, colors = [], []
    for r in range(rings + 1):
        theta = math.pi * r / rings
        for s in range(segments):
            phi = 2. * math.pi * s / segments
            vertices.append([math.sin(theta) * math.cos(phi), math.cos(theta), math.sin(theta) * math.sin(phi)])
            colors.append([0.9, 0.6, 0.4] if (r // 2) % 2 else [0.5, 0.7, 0.9])
    faces = []
    for r in range(rings):
        for s in range(segments):
            a, b = r * segments + s, r * segments + (s + 1) % segments
            c, d = a + segments, b + segments
            faces += [[a, b, d], [d, c, a]]
    return np.asarray(vertices, np.float32), np.asarray(faces, np.int32), np.asarray(colors, np.float32)


def true_coefficients(device):
    """A sky-like light: bright from above, a warm tint from one side."""
    L = torch.zeros(9, 3)
    L[0] = torch.tensor([0.9, 0.9, 1.0]) / lighting.SH_C0 * 0.5
    L[1] = torch.tensor([0.5, 0.5, 0.6])     # y: from above
    L[3] = torch.tensor([0.4, 0.2, 0.1])     # x: warm from the right
    L[6] = torch.tensor([-0.2, -0.2, -0.1])
    L[8] = torch.tensor([0.15, 0.1, 0.1])
    return L.to(device)


def render(coefficients, vertices, faces, colors, width, height):
    dev = vertices.device
    view = matrices.translation(torch.tensor([0., 0., -3.], device=dev))
    projection = matrices.perspective_projection(near=0.1, far=20., right=0.05, aspect=float(height) / width).to(dev)
    v4 = torch.cat([vertices, torch.ones_like(vertices[:, :1])], dim=1)
    clip = (v4 @ view) @ projection
    normals = lighting.vertex_normals(vertices, faces)
    attributes = torch.cat([torch.ones_like(vertices[:, :1]), colors, normals], dim=1)

    def shader_fn(gbuffer, table):
        return shading.shade_gbuffer_sh(gbuffer, table, background=BACKGROUND, **LAYOUT)

    return dirt.rasterise_deferred(background_attributes=torch.zeros([height, width, 7], device=dev), vertices=clip,
                                   vertex_attributes=attributes, faces=faces, shader_fn=shader_fn, shader_additional_inputs=[coefficients])


def fit(width=160, height=120, steps=60, rate=0.05, device=None):
    """-> (losses per step, |L - truth| before, |L - truth| after)"""
    dev = device or torch.device('cuda', 0)
    vertices, faces, colors = (torch.from_numpy(a).to(dev) for a in build_sphere())
    truth = true_coefficients(dev)
    target = render(truth, vertices, faces, colors, width, height).detach()
    table = torch.zeros(9, 3, device=dev)
    table[0] = 0.5 / lighting.SH_C0 * 0.5
    table.requires_grad_(True)
    before = float((table.detach() - truth).norm())
    optimiser = torch.optim.Adam([table], lr=rate)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(table, vertices, faces, colors, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    return losses, before, float((table.detach() - truth).norm())


def main():
    losses, before, after = fit()
    print('loss %.3e -> %.3e in %d steps; |L - truth| %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))


if __name__ == '__main__':
    main()
