#!/usr/bin/env python3
"""A pose-fitting loop on the whole fused pose -> pixels path: gradient descent turns the eight joints of a small articulated
figure -- a trunk of three links, a head and two arms of two links each -- until its deferred-shaded image and its projected
joint positions match those of a target pose.  Every step is

    joint rotations -> pose_skeleton (the forward kinematics of the tree, one HIP kernel: bone transforms and posed joints)
    -> skin_vertices (linear-blend skinning, one HIP kernel) -> vertex_stage (transforms + vertex normals, one HIP kernel)
    -> rasterise_deferred with shade_gbuffer -> image loss + key-point loss -> backward

-- examples/fit_pose_fused.py composes the transforms of its three-bone chain with matrices.rodrigues / compose in torch;
here the skeleton branches, and the posed joints the kernel returns beside the transforms are projected with the same
view_projection for the key-point term that pose fitting pairs with an image loss.  Prints the losses as it goes.

    python examples/fit_body_pose_fused.py [steps]
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import geometry, kinematics, matrices, shading, skinning  # noqa: E402

frame_width, frame_height = 320, 240
# joint: (parent, position, where its link ends, the link's radius)
FIGURE = (
    (-1, (0., -0.55, 0.), (0., -0.25, 0.), 0.11),       # 0 pelvis
    (0, (0., -0.25, 0.), (0., 0.05, 0.), 0.11),         # 1 spine
    (1, (0., 0.05, 0.), (0., 0.35, 0.), 0.11),          # 2 chest
    (2, (0., 0.35, 0.), (0., 0.6, 0.), 0.08),           # 3 head
    (2, (0.11, 0.27, 0.), (0.4, 0.27, 0.), 0.05),       # 4 left shoulder
    (4, (0.4, 0.27, 0.), (0.68, 0.27, 0.), 0.045),      # 5 left elbow
    (2, (-0.11, 0.27, 0.), (-0.4, 0.27, 0.), 0.05),     # 6 right shoulder
    (6, (-0.4, 0.27, 0.), (-0.68, 0.27, 0.), 0.045),    # 7 right elbow
)
PARENTS = [f[0] for f in FIGURE]
KEY_POINT_WEIGHT = 5.


def build_link(start, end, radius, rings, segments, first_vertex, device):
    """A tube of `rings` rings of `segments` vertices from `start` to `end` with a fan over each end.
    -> (vertices [n, 3], faces [f, 3] numbered from first_vertex, the position of every vertex along the link in [0, 1])"""
    a, b = torch.tensor(start, device=device), torch.tensor(end, device=device)
    axis = torch.nn.functional.normalize(b - a, dim=0)
    u = torch.nn.functional.normalize(torch.linalg.cross(axis, torch.tensor([0., 0., 1.], device=device)), dim=0)   # (no link runs along z)
    w = torch.linalg.cross(u, axis)
    s = torch.linspace(0., 1., rings, device=device)
    ang = torch.arange(segments, device=device) * (2. * math.pi / segments)
    ring = radius * (torch.cos(ang)[:, None] * u + torch.sin(ang)[:, None] * w)
    vertices = torch.cat([(ring[None] + (a + s[:, None] * (b - a))[:, None]).reshape(-1, 3), (a - 0.3 * radius * axis)[None], (b + 0.3 * radius * axis)[None]])
    along = torch.cat([s[:, None].expand(rings, segments).reshape(-1), torch.tensor([0., 1.], device=device)])
    r, q = torch.meshgrid(torch.arange(rings - 1, device=device), torch.arange(segments, device=device), indexing='ij')
    p0, p1 = (r * segments + q).reshape(-1), (r * segments + (q + 1) % segments).reshape(-1)
    q1 = torch.arange(segments, device=device)
    low, high, top = rings * segments, rings * segments + 1, (rings - 1) * segments
    faces = torch.cat([torch.stack([p0, p0 + segments, p1], 1), torch.stack([p0 + segments, p1 + segments, p1], 1),
                       torch.stack([torch.full_like(q1, low), q1, (q1 + 1) % segments], 1),
                       torch.stack([torch.full_like(q1, high), top + (q1 + 1) % segments, top + q1], 1)])
    return vertices, (faces + first_vertex).to(torch.int32), along


def build_figure(device, rings=9, segments=16):
    """One link per joint.  Every vertex follows its own joint and that joint's parent: the parent's share falls linearly from
    a half where the link begins to nothing a quarter of the way along (a root link follows its joint alone).
    -> (vertices [V, 3], faces [F, 3] int32, bone_indices [V, 2] int32, bone_weights [V, 2], joints [J, 3])"""
    vertices, faces, indices, weights = [], [], [], []
    count = 0
    for j, (parent, start, end, radius) in enumerate(FIGURE):
        v, f, along = build_link(start, end, radius, rings, segments, count, device)
        share = (0.5 - 2. * along).clamp(min=0.) if parent >= 0 else torch.zeros_like(along)
        vertices.append(v)
        faces.append(f)
        indices.append(torch.tensor([j, max(parent, 0)], dtype=torch.int32, device=device).expand(v.shape[0], 2))
        weights.append(torch.stack([1. - share, share], 1))
        count += v.shape[0]
    return torch.cat(vertices), torch.cat(faces), torch.cat(indices).contiguous(), torch.cat(weights), torch.tensor([f[1] for f in FIGURE], device=device)


def shader_fn(gbuffer, light_direction):
    return shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(light_direction, (0.9, 0.8, 0.7), double_sided=False)],
                                 colors=4, normals=7, positions=1, mask=0, ambient=(0.15, 0.15, 0.15), background=(0., 0., 0.2))


def render(rest, skin, topology, skeleton, joints, rotations, view_projection, light):
    """-> (the image [H, W, 3], the posed joints projected to normalised device coordinates [J, 2])"""
    transforms, posed_joints = kinematics.pose_skeleton(rotations, joints, skeleton)
    posed = skinning.skin_vertices(rest, skin, transforms)
    clip, world, normals = geometry.vertex_stage(posed, topology, None, view_projection)
    attributes = torch.cat([torch.ones_like(world[:, :1]), world[:, :3], torch.ones_like(normals), normals], dim=1)
    image = dirt.rasterise_deferred(vertices=clip, vertex_attributes=attributes, faces=topology.faces,
                                    background_attributes=torch.zeros([frame_height, frame_width, 10], device=clip.device),
                                    shader_fn=shader_fn, shader_additional_inputs=[light])
    joints_clip = torch.cat([posed_joints, torch.ones_like(posed_joints[:, :1])], 1) @ view_projection
    return image, joints_clip[:, :2] / joints_clip[:, 3:]


def main(steps=40, rate=0.1):
    """-> the losses (image term + KEY_POINT_WEIGHT x key-point term).  `rate` is half that of examples/fit_pose_fused.py, whose
    trials it rests on: the figure covers more of the frame than that tube, and the key-point term adds its own curvature.  On an
    MI355X twelve steps take the loss from 0.01311 to 0.01147 (image term 0.01062 -> 0.00970, key points 0.000498 -> 0.000353,
    first gradient norm 0.038), lower at every printed step; larger rates were not tried."""
    dev = torch.device('cuda', 0)
    rest, faces, bone_indices, bone_weights, joints = build_figure(dev)
    topology = geometry.MeshTopology(faces, rest.shape[0])                  # once: neither the topology,
    skin = skinning.SkinWeights(bone_indices, bone_weights, len(FIGURE))    # nor the weights,
    skeleton = kinematics.Skeleton(PARENTS, device=dev)                     # nor the tree change while the pose moves
    view_projection = matrices.translation(torch.tensor([0., 0., -2.5], device=dev)) @ \
        matrices.perspective_projection(near=0.1, far=20., right=0.06, aspect=float(frame_height) / frame_width).to(dev)
    light = torch.nn.functional.normalize(torch.tensor([0.4, -0.3, -1.], device=dev), dim=0)
    target_rotations = torch.tensor([[0., 0.2, 0.1], [0., 0., -0.15], [0.1, 0., -0.1], [0., 0.3, 0.2],
                                     [0., 0.2, 0.5], [0., 0., 0.7], [0., -0.2, -0.4], [0., 0.3, -0.6]], device=dev)
    offsets = torch.tensor([[0., -0.1, -0.08], [0., 0., 0.1], [-0.05, 0., 0.08], [0., -0.15, -0.1],
                            [0., -0.1, -0.2], [0., 0.1, -0.25], [0., 0.1, 0.2], [0., -0.1, 0.25]], device=dev)
    rotations = (target_rotations + offsets).requires_grad_(True)
    with torch.no_grad():
        target_image, target_points = render(rest, skin, topology, skeleton, joints, target_rotations, view_projection, light)
    losses = []
    for it in range(steps):
        image, points = render(rest, skin, topology, skeleton, joints, rotations, view_projection, light)
        image_loss, point_loss = ((image - target_image) ** 2).mean(), ((points - target_points) ** 2).mean()
        loss = image_loss + KEY_POINT_WEIGHT * point_loss
        (grad,) = torch.autograd.grad(loss, rotations)
        with torch.no_grad():
            rotations -= rate * grad
        losses.append(loss.item())
        if it % 5 == 0 or it == steps - 1:
            print('step %3d  loss %.6f  (image %.6f, key points %.6f)  |d loss / d rotations| %.3e  pose error %.4f'
                  % (it, losses[-1], image_loss.item(), point_loss.item(), grad.norm().item(), (rotations - target_rotations).abs().max().item()))
    return losses


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 40)
