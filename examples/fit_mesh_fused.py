#!/usr/bin/env python3
"""A small mesh-fitting loop on the fused vertex stage: gradient descent moves the vertices of a shared-vertex mesh (a
bumpy sheet) until its deferred-shaded image matches that of a target sheet.  Every step is

    vertex_stage (transforms + vertex normals, one HIP kernel) -> rasterise_deferred with shade_gbuffer -> loss -> backward

-- the geometry and lighting steps of the reference's samples/deferred.py:40-51,58-98 with no torch composition left
between the vertices and the pixels.  Prints the loss and the gradient norms as it goes.

    python examples/fit_mesh_fused.py [steps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import geometry, matrices, shading  # noqa: E402

frame_width, frame_height = 320, 240


def build_sheet(n, bump, device):
    """(n + 1)^2 shared vertices over [-1, 1]^2, z = bump * a smooth hill; two triangles per cell"""
    u = torch.linspace(-1., 1., n + 1, device=device)
    y, x = torch.meshgrid(u, u, indexing='ij')
    z = bump * torch.exp(-3. * (x ** 2 + y ** 2))
    idx = torch.arange((n + 1) ** 2, device=device).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, 1:].reshape(-1), idx[1:, :-1].reshape(-1)
    faces = torch.cat([torch.stack([a, b, c], 1), torch.stack([a, c, d], 1)]).to(torch.int32)
    return torch.stack([x, y, z], -1).reshape(-1, 3), faces


def shader_fn(gbuffer, light_direction):
    return shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(light_direction, (0.9, 0.8, 0.7), double_sided=False)],
                                 colors=4, normals=7, positions=1, mask=0, ambient=(0.15, 0.15, 0.15), background=(0., 0., 0.2))


def render(vertices, topology, model, view_projection, light):
    clip, world, normals = geometry.vertex_stage(vertices, topology, model, view_projection)
    attributes = torch.cat([torch.ones_like(world[:, :1]), world[:, :3], torch.ones_like(normals), normals], dim=1)
    return dirt.rasterise_deferred(vertices=clip, vertex_attributes=attributes, faces=topology.faces,
                                   background_attributes=torch.zeros([frame_height, frame_width, 10], device=clip.device),
                                   shader_fn=shader_fn, shader_additional_inputs=[light])


def main(steps=40):
    dev = torch.device('cuda', 0)
    target_vertices, faces = build_sheet(24, 0.5, dev)
    vertices = build_sheet(24, 0.1, dev)[0].requires_grad_(True)
    topology = geometry.MeshTopology(faces, vertices.shape[0])   # once: the topology does not change while the vertices move
    model = matrices.rodrigues(torch.tensor([-0.9, 0., 0.], device=dev))
    view_projection = matrices.translation(torch.tensor([0., 0., -3.], device=dev)) @ \
        matrices.perspective_projection(near=0.1, far=20., right=0.06, aspect=float(frame_height) / frame_width).to(dev)
    light = torch.nn.functional.normalize(torch.tensor([0.4, -0.3, -1.], device=dev), dim=0)
    with torch.no_grad():
        target = render(target_vertices, topology, model, view_projection, light)
    losses = []
    for it in range(steps):
        loss = ((render(vertices, topology, model, view_projection, light) - target) ** 2).mean()
        (grad,) = torch.autograd.grad(loss, vertices)
        with torch.no_grad():
            vertices -= 2.0 * grad
        losses.append(loss.item())
        if it % 5 == 0 or it == steps - 1:
            print('step %3d  loss %.6f  |d loss / d vertices| %.3e (max %.3e)' % (it, losses[-1], grad.norm().item(), grad.abs().max().item()))
    return losses


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 40)
