#!/usr/bin/env python3
"""examples/textured.py's textured, deferred-shaded cube with a large (2048 x 2048) checker texture, minified several times
over, shaded with the trilinear look-up: the level of detail comes from the footprint of the G-buffer's (u, v), and the
G-buffer's mask channel marks which pixels are surface.  Back-propagates an image loss to the texture, the light direction
and the vertices, and reports how many texels receive gradient with 'bilinear' and with 'trilinear'.  Writes
textured_mip.png next to this file when Pillow is available.

    python examples/textured_mip.py
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, texture as tex  # noqa: E402
import textured  # noqa: E402  (examples/textured.py: the cube, its camera and frame size)


def checker_texture(size=2048, squares=64):
    y, x = np.mgrid[0:size, 0:size]
    step = size // squares
    c = ((x // step + y // step) % 2).astype(np.float32)
    return np.stack([0.2 + 0.8 * c, 0.3 + 0.5 * (x / size), 0.9 - 0.6 * c], -1).astype(np.float32)


def make_shader(filter):
    def shader_fn(gbuffer, texture, light_direction):
        mask, uvs, normals = gbuffer[..., :1], gbuffer[..., 1:3], gbuffer[..., 3:]
        if filter == 'trilinear':   # level of detail from the (u, v) footprint; background pixels are not neighbours
            unlit = tex.sample_texture_uv(texture, uvs, filter='trilinear', mask=gbuffer[..., 0])
        else:
            unlit = tex.sample_texture_uv(texture, uvs, filter=filter)
        ambient = unlit * 0.4
        diffuse = lighting.diffuse_directional(normals.reshape(-1, 3), unlit.reshape(-1, 3), light_direction,
                                               light_color=torch.full((3,), 0.6, device=gbuffer.device), double_sided=True)
        background = torch.tensor([0., 0., 0.3], device=gbuffer.device)
        return (diffuse.reshape(unlit.shape) + ambient) * mask + background * (1. - mask)
    return shader_fn


def render(vertices_object, uvs, faces, texture, light_direction, filter='trilinear'):
    clip, attributes = textured.geometry(vertices_object, uvs, faces)
    return dirt.rasterise_deferred(
        vertices=clip, vertex_attributes=attributes, faces=faces,
        background_attributes=torch.zeros([textured.frame_height, textured.frame_width, 6], device=clip.device),
        shader_fn=make_shader(filter), shader_additional_inputs=[texture, light_direction])


def run(device, filter='trilinear'):
    """One forward + backward -> (pixels, texture, light, vertices), the three inputs carrying their gradients."""
    vertices, uvs, faces = (torch.from_numpy(a).to(device) for a in textured.build_cube())
    texture = torch.from_numpy(checker_texture()).to(device).requires_grad_(True)
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=device), dim=0).requires_grad_(True)
    vertices.requires_grad_(True)
    pixels = render(vertices, uvs, faces, texture, light, filter)
    (pixels ** 2).mean().backward()
    return pixels, texture, light, vertices


def main():
    device = torch.device('cuda', 0)
    for filter in ('bilinear', 'trilinear'):
        pixels, texture, light, vertices = run(device, filter)
        touched = (texture.grad.abs().sum(-1) != 0).float().mean().item()
        print('%-9s pixels mean %.4f; texels with gradient %.1f %%; |d loss / d light| %s, |d loss / d vertices| max %.3e'
              % (filter, pixels.mean().item(), 100 * touched, light.grad.abs().cpu().numpy().round(5), vertices.grad.abs().max().item()))
    try:
        from PIL import Image
        Image.fromarray((pixels.detach().clamp(0, 1) * 255).byte().cpu().numpy()).save(os.path.join(_HERE, 'textured_mip.png'))
    except ImportError:
        pass


if __name__ == '__main__':
    main()
