#!/usr/bin/env python3
"""B views of examples/textured.py's textured cube, each with a texture of its own, rendered in one
`rasterise_batch_deferred` call whose shader looks all B textures up in one launch: `sample_texture_uv_batch` with the
trilinear filter, (u, v) and the mask read in place from the batched G-buffer.  A short gradient descent on the B
textures toward B target images (the same views rendered with B target textures) prints the loss per step.

    python examples/textured_batch.py
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, matrices, texture as tex  # noqa: E402
import textured  # noqa: E402  (examples/textured.py: the cube and its checker texture)


def target_textures(scenes, size=128):
    """The checker of examples/textured.py, its channels rolled and its squares shifted per scene."""
    base = textured.checker_texture(size)
    return np.stack([np.roll(np.roll(base, 5 * b, axis=1), b, axis=2) for b in range(scenes)]).astype(np.float32)


def shader_fn(gbuffer, textures, light_direction):
    """gbuffer [B, H, W, 6] = mask, (u, v), normal; textures [B, Ht, Wt, 3]: scene b's pixels read textures[b]."""
    mask, normals = gbuffer[..., :1], gbuffer[..., 3:]
    unlit = tex.sample_texture_uv_batch(textures, gbuffer[..., 1:3], filter='trilinear', mask=gbuffer[..., 0])
    diffuse = lighting.diffuse_directional(normals.reshape(-1, 3), unlit.reshape(-1, 3), light_direction,
                                           light_color=torch.full((3,), 0.6, device=gbuffer.device), double_sided=True)
    background = torch.tensor([0., 0., 0.3], device=gbuffer.device)
    return (diffuse.reshape(unlit.shape) + unlit * 0.4) * mask + background * (1. - mask)


def geometry(vertices_object, uvs, faces, angles, height, width):
    """One view per angle (the cube turned about y) -> clip-space vertices [B, V, 4], attributes [B, V, 6], faces [B, F, 3]."""
    device = vertices_object.device
    v = torch.cat([vertices_object, torch.ones_like(vertices_object[:, -1:])], dim=1)
    view = matrices.compose(matrices.translation(torch.tensor([0., -2., -3.2], device=device)),
                            matrices.rodrigues(torch.tensor([-0.5, 0., 0.], device=device)))
    projection = matrices.perspective_projection(near=0.1, far=20., right=0.1, aspect=float(height) / width).to(device)
    clips, attributes = [], []
    for angle in angles:
        world = v @ matrices.rodrigues(torch.tensor([0., angle, 0.], device=device))
        clips.append((world @ view) @ projection)
        attributes.append(torch.cat([torch.ones_like(v[:, :1]), uvs, lighting.vertex_normals(world, faces)], dim=1))
    return torch.stack(clips), torch.stack(attributes), faces[None].expand(len(angles), -1, -1).contiguous()


def render(clip, attributes, faces, textures, light_direction, height, width):
    return dirt.rasterise_batch_deferred(
        vertices=clip, vertex_attributes=attributes, faces=faces,
        background_attributes=torch.zeros([clip.shape[0], height, width, 6], device=clip.device),
        shader_fn=shader_fn, shader_additional_inputs=[textures, light_direction])


def main(scenes=4, height=480, width=640, steps=8, rate=None, device=None, quiet=False):
    """-> [steps, scenes] losses (mean squared error of each scene's image against its target).  The image is linear in the
    textures, so the loss is quadratic; a texel seen by k pixels has curvature of about 2 k / (3 height width), and the default
    rate of 0.05 height width keeps a step stable up to k = 60."""
    rate = 0.05 * height * width if rate is None else rate
    device = device or torch.device('cuda', 0)
    vertices, uvs, faces = (torch.from_numpy(a).to(device) for a in textured.build_cube())
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=device), dim=0)
    clip, attributes, faces = geometry(vertices, uvs, faces, [0.6 + 0.5 * b for b in range(scenes)], height, width)
    with torch.no_grad():
        targets = render(clip, attributes, faces, torch.from_numpy(target_textures(scenes)).to(device), light, height, width)
    textures = torch.full((scenes, 128, 128, 3), 0.5, device=device, requires_grad=True)
    losses = []
    for step in range(steps):
        pixels = render(clip, attributes, faces, textures, light, height, width)
        per_scene = ((pixels - targets) ** 2).mean(dim=(1, 2, 3))
        grad, = torch.autograd.grad(per_scene.sum(), [textures])
        with torch.no_grad():
            textures -= rate * grad
        losses.append(per_scene.detach().cpu().numpy())
        if not quiet:
            print('step %2d  loss %.6f  per scene %s' % (step, losses[-1].mean(), np.round(losses[-1], 6)))
    return np.stack(losses)


if __name__ == '__main__':
    main()
