"""`skin_vertices` -> `vertex_stage` in one autograd graph.  What either stage computes is pinned by tests/test_skinning.py and
tests/test_geometry.py; this pins the wiring between them: the gradient the vertex stage returns for its vertices is the one
skinning's backward receives, unchanged, so every gradient of the chain has the bits of the two stages run apart."""
import numpy as np
import pytest
import torch

from tests import geometry_reference as G
from tests import skin_reference as S

V, J, K = 257, 24, 4


def inputs(scenes):
    """A grid mesh of 257 vertices skinned to 24 bones; scenes: None, or the count of per-scene transforms (the rest mesh is
    shared, the posed vertices and every output of the stage are per scene; the model matrix per scene, the
    view-projection shared)"""
    rng = np.random.default_rng(9300 + (scenes or 0))
    vertices, faces = G.grid_mesh(rng, V)
    idx, weights = S.random_weights(rng, V, K, J)
    lead = (scenes,) if scenes else ()
    cotangents = [rng.standard_normal(lead + (V, n)).astype(np.float32) for n in (4, 4, 3)]
    return dict(vertices=vertices, faces=faces, bone_indices=idx, bone_weights=weights, transforms=S.random_transforms(rng, J, scenes),
                model=G.random_model(rng, scenes), view_projection=G.random_view_projection(rng)), cotangents


@pytest.mark.gpu
@pytest.mark.parametrize('scenes', [None, 3], ids=['unbatched', 'b3_per_scene_transforms'])
def test_the_chain_has_the_gradients_of_its_two_stages_run_apart(gpu, scenes):
    from dirt_amd import geometry, skinning
    x, cotangents = inputs(scenes)
    skin = skinning.SkinWeights(torch.from_numpy(x['bone_indices']).to(gpu), torch.from_numpy(x['bone_weights']).to(gpu), J)
    topology = geometry.MeshTopology(torch.from_numpy(x['faces']).to(gpu), V)
    cotangents = [torch.from_numpy(c).to(gpu) for c in cotangents]
    names = ('vertices', 'transforms', 'bone_weights', 'model', 'view_projection')

    def leaves():
        return [torch.from_numpy(x[k]).to(gpu).requires_grad_(True) for k in names]

    def loss_of(outs):
        return sum((o * c).sum() for o, c in zip(outs, cotangents))

    v, T, w, m, p = chained = leaves()
    posed = skinning.skin_vertices(v, skin, T, weights=w)
    loss = loss_of(geometry.vertex_stage(posed, topology, m, p))
    loss.backward()

    v, T, w, m, p = apart = leaves()
    posed_apart = skinning.skin_vertices(v, skin, T, weights=w)
    handed = posed_apart.detach().requires_grad_(True)
    loss_apart = loss_of(geometry.vertex_stage(handed, topology, m, p))
    loss_apart.backward()
    assert all(t.grad is None for t in (v, T, w)) and handed.grad.shape == posed_apart.shape
    posed_apart.backward(handed.grad)

    assert posed.shape == ((scenes, V, 3) if scenes else (V, 3)) and torch.equal(posed, posed_apart) and torch.equal(loss, loss_apart)
    for k, a, b in zip(names, chained, apart):
        assert a.grad.shape == a.shape and torch.equal(a.grad, b.grad) and bool(a.grad.abs().max() > 0), k
