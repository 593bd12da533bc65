#!/usr/bin/env python3
"""A shape-and-pose fitting loop on the whole fused coefficients -> pixels path: gradient descent moves five shape
coefficients and the eight joint rotations of the articulated figure of examples/fit_body_pose_fused.py together until its
deferred-shaded image and its projected joint positions match those of a target body in a target pose.  Every step is

    shape coefficients + pose_corrective_features(rotations) -> blend_shapes (template + directions, joints regressed from the
    shaped mesh: one HIP kernel) -> pose_skeleton -> skin_vertices -> vertex_stage -> rasterise_deferred with shade_gbuffer
    -> image loss + key-point loss -> backward

-- examples/fit_body_pose_fused.py stops short of shape: its rest mesh and rest joints are constants.  Here they come from a
small procedural model in SMPL's form: five shape directions (trunk length, arm length, trunk radius, arm radius and one
asymmetric direction: the left arm alone), 9 (J - 1) = 63 pose-corrective directions that bulge every link where it meets
its parent, and a regressor that puts every joint at the mean of the first ring of its link.  Only the shape directions move
the joints (joint_shapes = 5 < K = 68).  Prints the losses as it goes.

    python examples/fit_body_shape_fused.py [steps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import fit_body_pose_fused as body  # noqa: E402  (the figure, its skinning weights and the renderer: imported, not copied)
from dirt_amd import blendshapes, geometry, kinematics, matrices, skinning  # noqa: E402

SHAPE_NAMES = ('trunk length', 'arm length', 'trunk radius', 'arm radius', 'left arm length')
TRUNK, ARMS, LEFT_ARM = (0, 1, 2, 3), (4, 5, 6, 7), (4, 5)
RINGS, SEGMENTS = 9, 16


def build_model(template, device):
    """-> (directions [68, V, 3], regressor [J, V]) for the figure's template: link j owns vertices j n .. (j + 1) n, n = rings x
    segments + 2, ring by ring (body.build_link)."""
    J = len(body.FIGURE)
    n = RINGS * SEGMENTS + 2
    V = template.shape[0]
    assert V == J * n
    link = torch.arange(V, device=device) // n
    start = torch.tensor([f[1] for f in body.FIGURE], device=device)[link]
    end = torch.tensor([f[2] for f in body.FIGURE], device=device)[link]
    axis = torch.nn.functional.normalize(end - start, dim=1)
    along = ((template - start) * axis).sum(1, keepdim=True)
    radial = template - start - along * axis                                   # from the link's axis to the vertex
    member = lambda links: torch.isin(link, torch.tensor(links, device=device))[:, None].float()   # noqa: E731
    up, out = torch.tensor([0., 1., 0.], device=device), torch.sign(template[:, :1]) * torch.tensor([1., 0., 0.], device=device)
    shoulder_height = body.FIGURE[4][1][1] - body.FIGURE[0][1][1]
    shape = [
        # the trunk and head stretch upwards from the pelvis; the arms ride on the chest
        member(TRUNK) * (template[:, 1:2] - body.FIGURE[0][1][1]) * up + member(ARMS) * shoulder_height * up,
        member(ARMS) * (template[:, :1].abs() - abs(body.FIGURE[4][1][0])) * out,          # both arms stretch outwards from the shoulders
        member(TRUNK) * radial, member(ARMS) * radial,                                     # thicker trunk, thicker arms
        member(LEFT_ARM) * (template[:, :1].abs() - abs(body.FIGURE[4][1][0])) * out,      # the asymmetric one
    ]
    # pose correctives: feature i of joint j (an entry of R_j - I) pushes the quarter of link j next to its joint along axis
    # i // 3, in proportion to component i % 3 of the vertex's offset from the link's axis
    near = (0.5 - 2. * along / (end - start).norm(dim=1, keepdim=True)).clamp(min=0.)
    eye = torch.eye(3, device=device)
    correctives = [0.5 * member((j,)) * near * radial[:, i % 3:i % 3 + 1] * eye[i // 3] for j in range(1, J) for i in range(9)]
    regressor = torch.zeros(J, V, device=device)
    for j in range(J):
        regressor[j, j * n:j * n + SEGMENTS] = 1. / SEGMENTS                   # the mean of the link's first ring: where the link begins
    return torch.stack(shape + correctives).contiguous(), regressor


def render(template, shapes, betas, skin, topology, skeleton, rotations, view_projection, light):
    coefficients = torch.cat([betas, blendshapes.pose_corrective_features(rotations)])
    rest, joints = blendshapes.blend_shapes(template, coefficients, shapes)
    return body.render(rest, skin, topology, skeleton, joints, rotations, view_projection, light)


def main(steps=40, rate=0.1):
    """-> the losses (image term + body.KEY_POINT_WEIGHT x key-point term).  One rate for the shape coefficients and the
    rotations: that of examples/fit_body_pose_fused.py, whose trials it rests on.  On an MI355X twelve steps take the loss from
    0.08197 to 0.01140 (image term 0.02657 -> 0.01051, key points 0.011079 -> 0.000177; first gradient norms 0.504 to the shape
    coefficients, 0.073 to the rotations) and forty to 0.00882, lower at every printed step.  The key points pull the two
    length coefficients in within ten steps; the radii and the asymmetric arm, which only the image term sees, move slowly
    at this rate (the largest shape error is still 0.49 of 0.5 after forty steps); larger rates were not tried."""
    dev = torch.device('cuda', 0)
    template, faces, bone_indices, bone_weights, joints = body.build_figure(dev, rings=RINGS, segments=SEGMENTS)
    directions, regressor = build_model(template, dev)
    shapes = blendshapes.BlendShapes(directions, regressor, joint_shapes=len(SHAPE_NAMES))    # once: the table, the regressor's indices,
    topology = geometry.MeshTopology(faces, template.shape[0])                                # the topology,
    skin = skinning.SkinWeights(bone_indices, bone_weights, len(body.FIGURE))                 # the weights
    skeleton = kinematics.Skeleton(body.PARENTS, device=dev)                                  # and the tree stay as they are
    assert torch.allclose(regressor @ template, joints, atol=1e-6)                            # the regressor finds the figure's own joints
    view_projection = matrices.translation(torch.tensor([0., 0., -2.5], device=dev)) @ \
        matrices.perspective_projection(near=0.1, far=20., right=0.06, aspect=float(body.frame_height) / body.frame_width).to(dev)
    light = torch.nn.functional.normalize(torch.tensor([0.4, -0.3, -1.], device=dev), dim=0)
    target_betas = torch.tensor([0.25, -0.2, 0.4, 0.5, 0.3], device=dev)
    target_rotations = torch.tensor([[0., 0.2, 0.1], [0., 0., -0.15], [0.1, 0., -0.1], [0., 0.3, 0.2],
                                     [0., 0.2, 0.5], [0., 0., 0.7], [0., -0.2, -0.4], [0., 0.3, -0.6]], device=dev)
    offsets = torch.tensor([[0., -0.1, -0.08], [0., 0., 0.1], [-0.05, 0., 0.08], [0., -0.15, -0.1],
                            [0., -0.1, -0.2], [0., 0.1, -0.25], [0., 0.1, 0.2], [0., -0.1, 0.25]], device=dev)
    betas = torch.zeros(len(SHAPE_NAMES), device=dev, requires_grad=True)
    rotations = (target_rotations + 0.5 * offsets).requires_grad_(True)
    fixed = (skin, topology, skeleton)
    with torch.no_grad():
        target_image, target_points = render(template, shapes, target_betas, *fixed, target_rotations, view_projection, light)
    losses = []
    for it in range(steps):
        image, points = render(template, shapes, betas, *fixed, rotations, view_projection, light)
        image_loss, point_loss = ((image - target_image) ** 2).mean(), ((points - target_points) ** 2).mean()
        loss = image_loss + body.KEY_POINT_WEIGHT * point_loss
        grad_betas, grad_rotations = torch.autograd.grad(loss, [betas, rotations])
        with torch.no_grad():
            betas -= rate * grad_betas
            rotations -= rate * grad_rotations
        losses.append(loss.item())
        if it % 5 == 0 or it == steps - 1:
            print('step %3d  loss %.6f  (image %.6f, key points %.6f)  |d loss / d betas| %.3e  |d loss / d rotations| %.3e  shape error %.4f'
                  % (it, losses[-1], image_loss.item(), point_loss.item(), grad_betas.norm().item(), grad_rotations.norm().item(),
                     (betas - target_betas).abs().max().item()))
    return losses


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 40)
