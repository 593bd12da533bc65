#!/usr/bin/env python3
"""The textured cube of examples/textured.py with both halves of its shader fused: the texture look-up
(`sample_texture_uv`) hands its colours to the fused lighting (`shade_gbuffer(..., colors=<tensor>)`), which reads them
beside the G-buffer and writes their gradient for the look-up's backward.  The shader is the reference's
samples/textured.py one exactly, (diffuse + 0.4 * unlit) * mask + background * (1 - mask), in two kernels forward and two
backward instead of a chain of frame-sized elementwise ones.  Renders the image, then fits the texture to it from a grey
start by a few descent steps and prints the loss per step.  Writes textured_fused.png next to this file when Pillow is
available.

    python examples/textured_fused.py
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import shading, texture as tex  # noqa: E402
import textured  # noqa: E402  (examples/textured.py: the cube, its checker texture and its geometry)


def shader_fn(gbuffer, texture, light_direction):
    """gbuffer [H, W, 6] = mask, (u, v), normal"""
    unlit = tex.sample_texture_uv(texture, gbuffer[..., 1:3])
    return shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(light_direction, (.6, .6, .6), True)],
                                 colors=unlit, normals=3, mask=0, ambient=(.4, .4, .4), background=(0., 0., .3), clamp=None)


def render(vertices_object, uvs, faces, texture, light_direction):
    clip, attributes = textured.geometry(vertices_object, uvs, faces)
    return dirt.rasterise_deferred(
        vertices=clip, vertex_attributes=attributes, faces=faces,
        background_attributes=torch.zeros([textured.frame_height, textured.frame_width, 6], device=clip.device),
        shader_fn=shader_fn, shader_additional_inputs=[texture, light_direction])


def main(steps=6, rate=None, device=None, quiet=False):
    """-> (the image under the checker texture [H, W, 3], [steps] losses of the descent on the texture).  The image is linear
    in the texture, so the loss is quadratic; the rate is that of examples/textured_batch.py."""
    device = device or torch.device('cuda', 0)
    rate = 0.05 * textured.frame_height * textured.frame_width if rate is None else rate
    vertices, uvs, faces = (torch.from_numpy(a).to(device) for a in textured.build_cube())
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=device), dim=0)
    with torch.no_grad():
        target = render(vertices, uvs, faces, torch.from_numpy(textured.checker_texture()).to(device), light)
    if not quiet:
        print('pixels', tuple(target.shape), 'mean %.4f' % target.mean().item())
    texture = torch.full((128, 128, 3), 0.5, device=device, requires_grad=True)
    losses = []
    for step in range(steps):
        loss = ((render(vertices, uvs, faces, texture, light) - target) ** 2).mean()
        grad, = torch.autograd.grad(loss, [texture])
        with torch.no_grad():
            texture -= rate * grad
        losses.append(loss.item())
        if not quiet:
            print('step %2d  loss %.6f' % (step, losses[-1]))
    try:
        from PIL import Image
        Image.fromarray((target.clamp(0, 1) * 255).byte().cpu().numpy()).save(os.path.join(_HERE, 'textured_fused.png'))
    except ImportError:
        pass
    return target, np.asarray(losses)


if __name__ == '__main__':
    main()
