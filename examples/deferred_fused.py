#!/usr/bin/env python3
"""examples/deferred.py with its torch `shader_fn` replaced by one `dirt_amd.shading.shade_gbuffer` call: the same
deferred-shaded cube (samples/deferred.py:58-117: ambient + red diffuse + white Phong specular over a blue background), the
lighting of the G-buffer and its gradient now one HIP kernel each instead of some eighty elementwise torch kernels.

    python examples/deferred_fused.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import matrices, shading  # noqa: E402
from examples import deferred  # noqa: E402  (the cube, its geometry and the frame size)


def shader_fn(gbuffer, view_matrix, light_direction):
    """samples/deferred.py:58-96 in one call; G-buffer channels: mask, world position [1:4], colour [4:7], normal [7:10]."""
    return shading.shade_gbuffer(
        gbuffer,
        [shading.diffuse_directional_light(light_direction, (1., 0., 0.), double_sided=False),
         shading.specular_directional_light(light_direction, (1., 1., 1.), shininess=6., double_sided=False)],
        colors=4, normals=7, positions=1, mask=0, ambient=(0.2, 0.2, 0.2), background=(0., 0., 0.3),
        camera_position=torch.linalg.inv(view_matrix)[3, :3], clamp=(0., 1.))


def render(vertices_object, faces, view_matrix, light_direction):
    clip, faces, attributes = deferred.geometry(vertices_object, faces, view_matrix)
    return dirt.rasterise_deferred(
        vertices=clip, vertex_attributes=attributes, faces=faces,
        background_attributes=torch.zeros([deferred.frame_height, deferred.frame_width, 10], device=clip.device),
        shader_fn=shader_fn, shader_additional_inputs=[view_matrix, light_direction])


def main():
    dev = torch.device('cuda', 0)
    vertices, faces = (torch.from_numpy(a).to(dev) for a in deferred.build_cube())
    vertices.requires_grad_(True)
    view_matrix = matrices.compose(matrices.translation(torch.tensor([0., -1.5, -3.5], device=dev)),
                                   matrices.rodrigues(torch.tensor([-0.3, 0., 0.], device=dev))).requires_grad_(True)
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=dev), dim=0).requires_grad_(True)
    pixels = render(vertices, faces, view_matrix, light)
    (pixels ** 2).mean().backward()
    print('pixels', tuple(pixels.shape), 'mean %.4f' % pixels.mean().item())
    print('|d loss / d vertices| max %.3e, |d loss / d view| max %.3e, d loss / d light %s'
          % (vertices.grad.abs().max().item(), view_matrix.grad.abs().max().item(), light.grad.cpu().numpy().round(5)))
    return pixels


if __name__ == '__main__':
    main()
