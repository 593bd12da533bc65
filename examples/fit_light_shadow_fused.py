#!/usr/bin/env python3
"""Recovers the direction of a light from an image with a cast shadow on dirt_amd (MI355X): a box above a floor under one
directional light.  The light's orthographic shadow map is drawn by `shading.render_shadow_map`, the camera's 10-channel G-buffer
(mask, colour, normal, world position) goes through `rasterise_deferred`, and the shader multiplies the light's diffuse term
(`shading.shade_gbuffer`) by `shading.shadow_visibility` before it adds the ambient term and clamps once.  A short descent on the
direction, started some twenty degrees off, brings the rendering back to the target; the gradient reaches the direction
through the diffuse term, through the look-up (the light's matrix) and through the map that is drawn again in every step.

    python examples/fit_light_shadow_fused.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import matrices, shading  # noqa: E402

LAYOUT = dict(mask=0, colors=1, normals=4, positions=7)
AMBIENT, LIGHT_COLOR, BACKGROUND = (0.25, 0.25, 0.3), (0.8, 0.8, 0.75), (0.05, 0.05, 0.1)
MAP_SIZE = 128
# the light's box: 8 x 8 world units across, from 1 to 13 units in front of the light: one unit of depth is 1 / 6 of clip z
NEAR, FAR, RIGHT, DISTANCE = 1., 13., 4., 7.
# in clip z: the comparison turns from shadow to light over SOFTNESS; BIAS lifts the map by a quarter of a world unit, more than
# the depth a 3 x 3 window of texels (8 / 128 world units each) spans on a surface the light meets at 30 degrees
SOFTNESS, BIAS, NORMAL_OFFSET = 0.02, 0.04, 0.05


def quad(corners, normal, color):
    return np.asarray(corners, np.float32), np.tile(np.asarray(normal, np.float32), (4, 1)), np.tile(np.asarray(color, np.float32), (4, 1))


def build_scene():
    """A floor (y = 0, 7 x 7) and a box (1.2 x 1 x 1.2, its base 0.6 above the floor), every side with vertices and a normal of its
    own -> (vertices [V, 3], faces [F, 3], normals [V, 3], colours [V, 3])"""
    parts = [quad([[-3.5, 0, -3.5], [-3.5, 0, 3.5], [3.5, 0, 3.5], [3.5, 0, -3.5]], [0, 1, 0], [0.8, 0.8, 0.8])]
    lo, hi = np.array([-0.6, 0.6, -0.6]), np.array([0.6, 1.6, 0.6])
    for axis in range(3):
        for sign in (-1., 1.):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            corners = []
            for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)) if sign > 0 else ((0, 0), (0, 1), (1, 1), (1, 0)):
                p = np.zeros(3)
                p[axis] = hi[axis] if sign > 0 else lo[axis]
                p[u] = hi[u] if cu else lo[u]
                p[v] = hi[v] if cv else lo[v]
                corners.append(p)
            parts.append(quad(corners, np.eye(3)[axis] * sign, [0.9, 0.5, 0.3]))
    vertices, normals, colors = (np.concatenate([p[k] for p in parts]) for k in range(3))
    faces = np.concatenate([[[4 * q, 4 * q + 1, 4 * q + 2], [4 * q, 4 * q + 2, 4 * q + 3]] for q in range(len(parts))]).astype(np.int32)
    return vertices, faces, normals, colors


def light_matrix(direction):
    """world -> the clip space of a directional light that shines along `direction` [3] (row vectors), differentiably: an
    orthographic camera DISTANCE in front of the scene's centre that looks along the direction"""
    dev = direction.device
    d = direction / direction.norm()
    z_axis = -d                                            # a camera looks down its -z
    x_axis = torch.linalg.cross(torch.tensor([0., 0., 1.], device=dev), z_axis)
    x_axis = x_axis / x_axis.norm()
    y_axis = torch.linalg.cross(z_axis, x_axis)
    eye = torch.tensor([0., 0.8, 0.], device=dev) - DISTANCE * d
    view = matrices.compose(matrices.translation(-eye), matrices.pad_3x3_to_4x4(torch.stack([x_axis, y_axis, z_axis], dim=1)))
    return matrices.compose(view, matrices.orthographic_projection(NEAR, FAR, RIGHT, 1.).to(dev))


def camera_matrix(width, height, device):
    # the scene turned about y, tipped towards the camera (the floor is seen from above), then moved 7 units down the camera's -z
    view = matrices.compose(matrices.rodrigues(torch.tensor([0., 0.5, 0.])), matrices.rodrigues(torch.tensor([-0.6, 0., 0.])),
                            matrices.translation(torch.tensor([0., -0.3, -7.])))
    return matrices.compose(view, matrices.perspective_projection(near=0.1, far=30., right=0.05, aspect=float(height) / width)).to(device)


def render(direction, scene, width, height, shadows=True):
    vertices, faces, normals, colors = scene
    dev = vertices.device
    v4 = torch.cat([vertices, torch.ones_like(vertices[:, :1])], dim=1)
    clip = v4 @ camera_matrix(width, height, dev)
    attributes = torch.cat([torch.ones_like(vertices[:, :1]), colors, normals, vertices], dim=1)
    matrix = light_matrix(direction)
    shadow_map = shading.render_shadow_map(vertices, faces, matrix, MAP_SIZE, far=1.)

    def shader_fn(gbuffer, direction, shadow_map, matrix):
        direct = shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(direction / direction.norm(), LIGHT_COLOR, double_sided=False)],
                                       colors=LAYOUT['colors'], normals=LAYOUT['normals'], mask=LAYOUT['mask'], clamp=None)
        if shadows:
            direct = direct * shading.shadow_visibility(gbuffer, shadow_map[None], matrix[None], positions=LAYOUT['positions'],
                                                        normals=LAYOUT['normals'], mask=LAYOUT['mask'], kernel=3, bias=BIAS, softness=SOFTNESS,
                                                        normal_offset=NORMAL_OFFSET)
        rest = shading.shade_gbuffer(gbuffer, [], colors=LAYOUT['colors'], normals=LAYOUT['normals'], mask=LAYOUT['mask'], ambient=AMBIENT,
                                     background=BACKGROUND, clamp=None)
        return torch.clamp(direct + rest, 0., 1.)

    return dirt.rasterise_deferred(background_attributes=torch.zeros([height, width, 10], device=dev), vertices=clip, vertex_attributes=attributes,
                                   faces=faces, shader_fn=shader_fn, shader_additional_inputs=[direction, shadow_map, matrix])


def angle_between(a, b):
    return math.degrees(math.acos(max(-1., min(1., float(torch.dot(a / a.norm(), b / b.norm()))))))


def fit(width=160, height=120, steps=60, rate=0.03, device=None):
    """-> (losses per step, the angle in degrees between the direction and the truth before, and after)"""
    dev = device or torch.device('cuda', 0)
    scene = tuple(torch.from_numpy(a).to(dev) for a in build_scene())
    truth = torch.tensor([0.45, -0.8, -0.35], device=dev)
    target = render(truth, scene, width, height).detach()
    direction = torch.tensor([0.15, -0.9, -0.1], device=dev, requires_grad=True)
    before = angle_between(direction.detach(), truth)
    optimiser = torch.optim.Adam([direction], lr=rate)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(direction, scene, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    return losses, before, angle_between(direction.detach(), truth)


def main():
    losses, before, after = fit()
    print('loss %.3e -> %.3e in %d steps; direction error %.1f -> %.1f degrees' % (losses[0], losses[-1], len(losses), before, after))


if __name__ == '__main__':
    main()
