"""`blend_shapes` -> `pose_skeleton` -> `skin_vertices` -> `vertex_stage` in one autograd graph.  What every stage computes is
pinned by its own test file; this pins the wiring at the head of the chain, as tests/test_stage_chain.py does for the later
stages: the gradients skinning returns for its vertices and kinematics for its joints are the two that blend_shapes'
backward receives, unchanged, so every gradient of the chain has the bits of the stages run apart with the gradients
handed across."""
import numpy as np
import pytest
import torch

from tests import geometry_reference as G
from tests import kinematics_reference as KR
from tests import skin_reference as S
from tests import blend_reference as BR

V, J, K, KS, INFLUENCES = 257, 24, 13, 5, 4


def inputs(scenes):
    """A grid mesh of 257 vertices with 13 directions (5 of them move the joints), the 24-joint SMPL tree, four influences per
    vertex; scenes: None, or the count of per-scene coefficients and rotations (the template is shared; everything
    downstream is per scene; the model matrix per scene, the view-projection shared)"""
    rng = np.random.default_rng(9400 + (scenes or 0))
    template, faces = G.grid_mesh(rng, V)
    idx, weights = S.random_weights(rng, V, INFLUENCES, J)
    lead = (scenes,) if scenes else ()
    cotangents = [rng.standard_normal(lead + (V, n)).astype(np.float32) for n in (4, 4, 3)] + [rng.standard_normal(lead + (J, 3)).astype(np.float32)]
    return dict(template=np.asarray(template[..., :3], np.float32), faces=faces, bone_indices=idx, bone_weights=weights,
                directions=(0.05 * rng.standard_normal((K, V, 3))).astype(np.float32), regressor=BR.random_regressor(rng, J, V),
                coefficients=rng.standard_normal(lead + (K,)).astype(np.float32), rotations=(0.3 * rng.standard_normal(lead + (J, 3))).astype(np.float32),
                model=G.random_model(rng, scenes), view_projection=G.random_view_projection(rng)), cotangents


@pytest.mark.gpu
@pytest.mark.parametrize('scenes', [None, 3], ids=['unbatched', 'b3_per_scene_coefficients'])
def test_the_chain_has_the_gradients_of_its_stages_run_apart(gpu, scenes):
    from dirt_amd import blendshapes, geometry, kinematics, skinning
    x, cotangents = inputs(scenes)
    shapes = blendshapes.BlendShapes(torch.from_numpy(x['directions']).to(gpu), torch.from_numpy(x['regressor']).to(gpu), KS)
    skeleton = kinematics.Skeleton(KR.SMPL_PARENTS, device=gpu)
    skin = skinning.SkinWeights(torch.from_numpy(x['bone_indices']).to(gpu), torch.from_numpy(x['bone_weights']).to(gpu), J)
    topology = geometry.MeshTopology(torch.from_numpy(x['faces']).to(gpu), V)
    cotangents = [torch.from_numpy(c).to(gpu) for c in cotangents]
    names = ('template', 'coefficients', 'rotations', 'model', 'view_projection')

    def leaves():
        return [torch.from_numpy(x[k]).to(gpu).requires_grad_(True) for k in names]

    def tail(rest, joints, r, m, p):
        transforms, posed_joints = kinematics.pose_skeleton(r, joints, skeleton)
        posed = skinning.skin_vertices(rest, skin, transforms)
        outs = tuple(geometry.vertex_stage(posed, topology, m, p)) + (posed_joints,)
        return sum((o * c).sum() for o, c in zip(outs, cotangents))

    t, c, r, m, p = chained = leaves()
    rest, joints = blendshapes.blend_shapes(t, c, shapes)
    loss = tail(rest, joints, r, m, p)
    loss.backward()

    t, c, r, m, p = apart = leaves()
    rest_apart, joints_apart = blendshapes.blend_shapes(t, c, shapes)
    handed = [o.detach().requires_grad_(True) for o in (rest_apart, joints_apart)]
    loss_apart = tail(handed[0], handed[1], r, m, p)
    loss_apart.backward()
    assert t.grad is None and c.grad is None and all(h.grad.shape == o.shape for h, o in zip(handed, (rest_apart, joints_apart)))
    torch.autograd.backward([rest_apart, joints_apart], [h.grad for h in handed])

    lead = (scenes,) if scenes else ()
    assert rest.shape == lead + (V, 3) and joints.shape == lead + (J, 3)
    assert torch.equal(rest, rest_apart) and torch.equal(joints, joints_apart) and torch.equal(loss, loss_apart)
    for k, a, b in zip(names, chained, apart):
        assert a.grad.shape == a.shape and torch.equal(a.grad, b.grad) and bool(a.grad.abs().max() > 0), k
