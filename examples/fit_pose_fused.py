#!/usr/bin/env python3
"""A small pose-fitting loop on the fused skinning stage: gradient descent turns the three bones of a tube until its
deferred-shaded image matches that of a target pose.  Every step is

    bone rotations -> bone transforms (matrices.rodrigues / compose: the forward kinematics of a three-bone chain, in torch)
    skin_vertices (linear-blend skinning, one HIP kernel) -> vertex_stage (transforms + vertex normals, one HIP kernel)
    -> rasterise_deferred with shade_gbuffer -> loss -> backward

-- where the reference's samples/deferred.py:40-41 moves its mesh with one matrix, every vertex here follows a blend of
two bone matrices, the weights blended along the tube's axis.  Prints the loss and the gradient norm as it goes.

    python examples/fit_pose_fused.py [steps]
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import geometry, matrices, shading, skinning  # noqa: E402

frame_width, frame_height = 320, 240
JOINTS = (-0.6, -0.2, 0.2)   # the height of each bone's pivot on the tube's axis (the tube spans y in [-0.6, 0.6])


def build_tube(rings, segments, radius, device):
    """`rings` rings of `segments` shared vertices around the y axis from y = -0.6 to 0.6, two triangles per quad, and a fan
    over each end.  -> (vertices [V, 3], faces [F, 3] int32)"""
    y = torch.linspace(-0.6, 0.6, rings, device=device)
    ang = torch.arange(segments, device=device) * (2. * math.pi / segments)
    ring = torch.stack([radius * torch.cos(ang), torch.zeros_like(ang), radius * torch.sin(ang)], 1)
    vertices = torch.cat([(ring[None] + torch.stack([torch.zeros_like(y), y, torch.zeros_like(y)], 1)[:, None]).reshape(-1, 3),
                          torch.tensor([[0., -0.65, 0.], [0., 0.65, 0.]], device=device)])
    r, q = torch.meshgrid(torch.arange(rings - 1, device=device), torch.arange(segments, device=device), indexing='ij')
    a, b = (r * segments + q).reshape(-1), (r * segments + (q + 1) % segments).reshape(-1)
    q1 = torch.arange(segments, device=device)
    low, high, top = rings * segments, rings * segments + 1, (rings - 1) * segments
    faces = torch.cat([torch.stack([a, a + segments, b], 1), torch.stack([a + segments, b + segments, b], 1),
                       torch.stack([torch.full_like(q1, low), q1, (q1 + 1) % segments], 1),
                       torch.stack([torch.full_like(q1, high), top + (q1 + 1) % segments, top + q1], 1)])
    return vertices, faces.to(torch.int32)


def tube_weights(vertices):
    """Two influences per vertex, blended along the axis: bone j owns the tube at the middle of its segment and hands over
    linearly to the next.  -> (bone_indices [V, 2], bone_weights [V, 2])"""
    centres = torch.tensor([-0.4, 0., 0.4], device=vertices.device)
    t = ((vertices[:, 1] - centres[0]) / (centres[1] - centres[0])).clamp(0., 2.)   # 0 at the first centre, 2 at the last
    lower = t.floor().clamp(max=1.)
    upper_weight = t - lower
    return torch.stack([lower, lower + 1.], 1).to(torch.int32), torch.stack([1. - upper_weight, upper_weight], 1)


def bone_transforms(rotations):
    """The chain's forward kinematics: bone j turns by rotations[j] about its pivot (0, JOINTS[j], 0) in the frame of bone
    j - 1.  [3, 3] angle-axis vectors -> [3, 4, 4] transforms, row-vector convention."""
    out, parent = [], None
    for j, height in enumerate(JOINTS):
        pivot = torch.tensor([0., height, 0.], device=rotations.device)
        local = matrices.compose(matrices.translation(-pivot), matrices.rodrigues(rotations[j]), matrices.translation(pivot))
        parent = local if parent is None else matrices.compose(local, parent)
        out.append(parent)
    return torch.stack(out)


def shader_fn(gbuffer, light_direction):
    return shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(light_direction, (0.9, 0.8, 0.7), double_sided=False)],
                                 colors=4, normals=7, positions=1, mask=0, ambient=(0.15, 0.15, 0.15), background=(0., 0., 0.2))


def render(rest, skin, topology, rotations, view_projection, light):
    posed = skinning.skin_vertices(rest, skin, bone_transforms(rotations))
    clip, world, normals = geometry.vertex_stage(posed, topology, None, view_projection)
    attributes = torch.cat([torch.ones_like(world[:, :1]), world[:, :3], torch.ones_like(normals), normals], dim=1)
    return dirt.rasterise_deferred(vertices=clip, vertex_attributes=attributes, faces=topology.faces,
                                   background_attributes=torch.zeros([frame_height, frame_width, 10], device=clip.device),
                                   shader_fn=shader_fn, shader_additional_inputs=[light])


def main(steps=40, rate=0.2):
    """-> the losses.  `rate` by trial on an MI355X, 40 steps from a loss of 0.00425 (first gradient norm 0.110): rates 0.05,
    0.1 and 0.2 descend at every step, to 0.00167, 0.00149 and 0.00114; 0.4 descends with a zigzag (0.00081); 0.8 and 2.0
    overshoot at once (0.0058 and 0.0203 after one step) and oscillate above where they began.  0.2 is the largest tried
    that descends at every step."""
    dev = torch.device('cuda', 0)
    rest, faces = build_tube(25, 24, 0.12, dev)
    topology = geometry.MeshTopology(faces, rest.shape[0])              # once: neither the topology
    skin = skinning.SkinWeights(*tube_weights(rest), num_bones=3)       # nor the weights change while the pose moves
    view_projection = matrices.translation(torch.tensor([0., 0., -2.5], device=dev)) @ \
        matrices.perspective_projection(near=0.1, far=20., right=0.06, aspect=float(frame_height) / frame_width).to(dev)
    light = torch.nn.functional.normalize(torch.tensor([0.4, -0.3, -1.], device=dev), dim=0)
    target_rotations = torch.tensor([[0., 0., 0.25], [0., 0., -0.6], [0.3, 0., 0.5]], device=dev)
    rotations = (target_rotations + torch.tensor([[0., 0., -0.12], [0., 0., 0.2], [-0.1, 0., -0.15]], device=dev)).requires_grad_(True)
    with torch.no_grad():
        target = render(rest, skin, topology, target_rotations, view_projection, light)
    losses = []
    for it in range(steps):
        loss = ((render(rest, skin, topology, rotations, view_projection, light) - target) ** 2).mean()
        (grad,) = torch.autograd.grad(loss, rotations)
        with torch.no_grad():
            rotations -= rate * grad
        losses.append(loss.item())
        if it % 5 == 0 or it == steps - 1:
            print('step %3d  loss %.6f  |d loss / d rotations| %.3e  pose error %.4f' % (it, losses[-1], grad.norm().item(),
                                                                                         (rotations - target_rotations).abs().max().item()))
    return losses


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 40)
