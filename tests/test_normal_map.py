"""Tangent-space normal mapping -- `dirt_amd.geometry.vertex_tangents` (dirt_tangent.hip), `dirt_amd.shading.perturb_normals`
(dirt_normal_map.hip) and their torch forms `dirt_amd.lighting.vertex_tangents` / `perturb_normals` -- against the float64
restatement of tests/normal_map_reference.py.  Every comparison is per element, |got - ref64| <= tol * (L1 mass of the element's
terms); an element of zero mass must equal the reference exactly; the channels `perturb_normals` does not touch must keep
their bits.

The tolerances are measured, not chosen: the float32 torch composition (`lighting.*` plus `torch.cat`) is run on
`tolerance_cases()`, the random inputs of the tests below, and its worst |f32 - ref64| / mass per kind of result is F32; the
kernels, which order a vertex's sums differently, get 4 x that.  Produced by

    python -m tests.normal_map_reference
"""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import normal_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# worst |f32 - ref64| / mass of the float32 composition on tolerance_cases(), per kind of result (python -m tests.normal_map_reference),
# rounded up.  Measured again with the tori among the cases: 8.759e-8, 5.310e-8, 1.487e-7, 3.384e-8, 3.975e-8, 2.218e-8, the same
# figures, set by the strips (the tori alone: 7.12e-8, 4.50e-8, 6.53e-8)
F32 ={'tangents': 8.76e-8, 'd_vertices': 5.32e-8, 'd_normals': 1.49e-7, 'out': 3.39e-8, 'd_gbuffer': 3.98e-8, 'd_normal_map': 2.22e-8}
KERNEL = 4     # the kernels' allowance over the float32 composition


def kernel_constants():
    text = lambda name: open(os.path.join(ROOT, 'dirt_amd', 'csrc', name)).read()   # noqa: E731
    find = lambda source, name: int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1))   # noqa: E731
    return find(text('dirt_tangent.hip'), 'TG_BLOCK'), find(text('dirt_normal_map.hip'), 'NM_BLOCK'), find(text('dirt_normal_map.hip'), 'NM_ITER')


TG_BLOCK, NM_BLOCK, NM_ITER = kernel_constants()
SPAN = NM_BLOCK * NM_ITER      # pixels of one workgroup, forward and backward
FLAT = SPAN + 3                # one full workgroup and a second with three pixels
LAYOUTS = {   # name -> (Cg, first normal channel, first tangent channel); every other channel holds noise
    'c7': (7, 0, 3),
    'c7r': (7, 4, 0),          # the normals after the tangents
    'c11': (11, 2, 6),
    'c12': (12, 3, 8),
    'c257': (257, 254, 100),   # the normals in the last three channels, past channel 256
}


class Mesh:
    """One mesh comparison: `scenes` draws of a sheet over a strip or a fan, of a torus or of the cube, grad_out [.., V, 4]."""

    def __init__(self, seed, kind, size=0, components=3, scenes=None, mirrored=False):
        rng = np.random.default_rng(seed)
        self.seed, self.components, self.scenes = seed, components, scenes
        if kind == 'cube':
            pos, nrm, uv, self.faces = R.cube_mesh()
            v = (pos + rng.normal(0., 0.05, pos.shape)).astype(np.float32)
            self.v, self.n, self.uv, self.share = v[None], nrm.astype(np.float32)[None], uv.astype(np.float32), 0.
        else:
            if kind == 'torus':     # size = (nu, nv); mirrored: False, True, or 'both' for the two as disconnected components of one mesh
                parts = [R.draw_torus(rng, *size, mirrored=m, components=components) for m in ((False, True) if mirrored == 'both' else (mirrored,))]
                v, n, uv = (np.concatenate([p[k] for p in parts]) for k in range(3))
                self.faces = np.concatenate([p[3] + i * len(parts[0][0]) for i, p in enumerate(parts)])     # the second component's indices offset
                share = max(p[4] for p in parts)
            else:
                xy, self.faces = R.strip_mesh(size) if kind == 'strip' else R.fan_mesh(size)
                v, n, uv, share = R.draw_mesh(rng, xy, self.faces, components, jitter=0.05 if kind == 'strip' else 0.02)
            draws = [(v, n)]
            for b in range(1, scenes or 1):     # the scenes share the uvs: the further ones are the first with its positions and normals jittered
                vb = v.copy()
                vb[:, :3] += rng.normal(0., 0.02, (len(v), 3)).astype(np.float32)
                draws.append((vb, R._unit(n + rng.normal(0., 0.05, n.shape)).astype(np.float32)))
            self.v, self.n, self.uv, self.share = np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws]), uv, share
        self.go = rng.standard_normal(self.v.shape[:2] + (4,)).astype(np.float32)
        self.V = self.v.shape[1]

    def per_scene(self):
        return [(self.v[b], self.n[b], self.uv, self.faces, self.go[b]) for b in range(self.v.shape[0])]

    def reference(self):
        refs = [R.tangents(*args) for args in self.per_scene()]
        for r in refs:     # the cube and the jittered scenes, which no redraw looked at, stay off the discontinuities too
            assert (r['det_share'] >= R.MARGIN).all() and (r['w_share'] >= R.MARGIN).all() and (r['sin'] >= R.MIN_SIN).all()
        return {k: np.stack([r[k] for r in refs]) for k in ('tangents', 'd_vertices', 'd_normals', 'mass_tangents', 'mass_d_vertices', 'mass_d_normals')}


class Pixels:
    """One pixel comparison: n pixels of a G-buffer layout, a normal map, grad_out [n, Cg]."""

    def __init__(self, seed, layout='c12', n=FLAT, strength=1., encoded=True):
        rng = np.random.default_rng(seed)
        self.seed, self.layout, self.n, self.strength, self.encoded = seed, layout, n, strength, encoded
        self.cg, self.on, self.ot = LAYOUTS[layout]
        self.g, self.m, self.share = R.draw_pixels(rng, n, self.cg, self.on, self.ot, encoded)
        self.go = rng.standard_normal((n, self.cg)).astype(np.float32)

    def measure(self):
        return self.g, self.m, self.on, self.ot, self.strength, self.encoded, self.go

    def reference(self):
        return R.perturb_gbuffer(*self.measure())


MESHES = {
    'triangle': dict(seed=7000, kind='strip', size=3),
    'cube': dict(seed=7001, kind='cube'),
    'fan300': dict(seed=7002, kind='fan', size=300),                      # the hub's list has 300 entries
    'strip%d' % (TG_BLOCK - 1): dict(seed=7003, kind='strip', size=TG_BLOCK - 1),
    'strip%d' % TG_BLOCK: dict(seed=7004, kind='strip', size=TG_BLOCK),   # one workgroup of vertices, one fewer, one more
    'strip%d' % (TG_BLOCK + 1): dict(seed=7005, kind='strip', size=TG_BLOCK + 1),
    'strip_w': dict(seed=7006, kind='strip', size=TG_BLOCK + 1, components=4),
    'scenes3': dict(seed=7007, kind='strip', size=TG_BLOCK + 1, scenes=3),
    # a closed surface: normals over the whole sphere, 1 to 6 faces per vertex, 294 vertices (38 in a second workgroup)
    'torus': dict(seed=7008, kind='torus', size=(20, 13)),
    # the same draw with u -> 1 - u: w = -1 at every vertex.  (A normal jittered past 90 degrees from the surface's -- one vertex in
    # 2 500 -- turns its vertex's sign, rightly; test_the_cases_hold_what_their_names_say asserts that these seeds drew none.)
    'torus_mirrored': dict(seed=7008, kind='torus', size=(20, 13), mirrored=True),
    'torus_both': dict(seed=7010, kind='torus', size=(20, 13), mirrored='both'),        # both signs in one launch, 588 vertices
    'torus_w3': dict(seed=7011, kind='torus', size=(20, 13), mirrored='both', components=4, scenes=3),
}
PIXELS = dict(
    {'flat': dict(seed=7100), 'decoded': dict(seed=7101, encoded=False), 'strength0': dict(seed=7102, strength=0.),
     'strength2': dict(seed=7103, strength=2.)},
    **{name: dict(seed=7110 + i, layout=name, n=FLAT if LAYOUTS[name][0] < 255 else NM_BLOCK + 3) for i, name in enumerate(LAYOUTS)},
    # a pass of one pixel, a second pass of one pixel, a second workgroup of one pixel
    **{'px%d' % n: dict(seed=7120 + i, layout='c11', n=n) for i, n in enumerate((1, NM_BLOCK + 1, SPAN + 1))})
_CASES = {}


def case_of(name):
    if name not in _CASES:
        case = Mesh(**MESHES[name]) if name in MESHES else Pixels(**PIXELS[name])
        _CASES[name] = (case, case.reference())
    return _CASES[name]


def tolerance_cases():
    """-> (mesh cases, pixel cases) as `normal_map_reference.measure_f32` takes them"""
    meshes = [args for name in MESHES for args in case_of(name)[0].per_scene()]
    return meshes, [case_of(name)[0].measure() for name in PIXELS]


def check(got, ref, kinds, what, factor=KERNEL):
    """The mass rule per kind of result, exact equality where the mass is zero."""
    worst = R.ratios(got, ref, kinds)
    print(what, ' '.join('%s %.2f' % (k, v / F32[k]) for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= factor * F32[k], '%s %s: |got - ref64| / mass = %.3e, allowed %.3e' % (what, k, v, factor * F32[k])
    for _, key in kinds:
        if got.get(key) is None:
            continue
        a = R._f64(got[key]).reshape(ref[key].shape)
        assert np.isfinite(a).all(), (what, key)
        zero = ref['mass_' + key] == 0
        assert np.array_equal(a[zero], ref[key][zero]), '%s %s: an element of zero mass differs' % (what, key)


# ---- CPU tests: the specification

def _quad(flip_u=False):
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [1., 1., 0.], [0., 1., 0.]])
    uv = v[:, :2].clone()
    if flip_u:
        uv[:, 0] = 1. - uv[:, 0]
    return v, torch.tensor([[0., 0., 1.]]).repeat(4, 1), uv, torch.tensor([[0, 1, 2], [0, 2, 3]])


def test_known_answers_of_the_unit_quad():
    """The unit quad in the z = 0 plane with uv = xy and normal +z: (1, 0, 0, +1) at every vertex; with u -> 1 - u, (-1, 0, 0, -1)."""
    from dirt_amd import lighting
    for flip, want in ((False, (1., 0., 0., 1.)), (True, (-1., 0., 0., -1.))):
        v, n, uv, f = _quad(flip)
        for vertices in (v, torch.cat([v, torch.full((4, 1), 7.)], 1), v[None].repeat(2, 1, 1)):
            got = lighting.vertex_tangents(vertices, n.expand(vertices.shape[:-1] + (3,)), uv, f)
            assert got.shape == tuple(vertices.shape[:-1]) + (4,)
            assert torch.equal(got, torch.tensor(want).expand_as(got)), (flip, got)
        ref = R.tangents(v.numpy(), n.numpy(), uv.numpy(), f.numpy())
        assert np.array_equal(ref['tangents'], np.tile(want, (4, 1)))


def test_a_flat_normal_map_returns_unit_normals_unchanged():
    """(0.5, 0.5, 1) decodes to (0, 0, 1): the shading normal is the normal, to the rounding of one more normalisation."""
    from dirt_amd import lighting
    rng = np.random.default_rng(7200)
    n = torch.from_numpy(R._unit(rng.standard_normal((50, 3))).astype(np.float32))
    t = torch.from_numpy(rng.standard_normal((50, 4)).astype(np.float32))
    out = lighting.perturb_normals(n, t, torch.tensor([0.5, 0.5, 1.]).expand(50, 3))
    assert float((out - n).abs().max()) <= 2.4e-7
    out = lighting.perturb_normals(n, t, torch.tensor([0., 0., 1.]).expand(50, 3), strength=5., encoded=False)
    assert float((out - n).abs().max()) <= 2.4e-7
    axes = torch.eye(3)
    assert torch.equal(lighting.perturb_normals(axes, torch.tensor([[0., 1., 0., 1.], [0., 0., 1., 1.], [1., 0., 0., -1.]]),
                                                torch.tensor([0.5, 0.5, 1.]).expand(3, 3)), axes)


def test_the_torch_forms_agree_with_the_restatement_in_float64():
    """`lighting.vertex_tangents` and `lighting.perturb_normals` under torch's autograd in float64 against the restatement's
    hand-written forward and backward: 1e-12 of the masses, on every case of this file."""
    for name in MESHES:
        case, ref = case_of(name)
        for b, args in enumerate(case.per_scene()):
            got = R.torch_tangents(*args, torch.float64)
            one = {k: v[b] for k, v in ref.items()}
            for kind, x in R.ratios(got, one, R.TANGENT_KINDS).items():
                assert x <= 1e-12, (name, b, kind, x)
            assert np.array_equal(got['tangents'][:, 3], one['tangents'][:, 3])
    # batched, the uvs shared: the same values as scene by scene
    from dirt_amd import lighting
    case, ref = case_of('scenes3')
    batched = lighting.vertex_tangents(torch.from_numpy(case.v).double(), torch.from_numpy(case.n).double(), torch.from_numpy(case.uv).double(),
                                       torch.from_numpy(case.faces))
    assert np.abs(batched.numpy() - ref['tangents']).max() <= 1e-12
    for name in PIXELS:
        case, ref = case_of(name)
        got = R.torch_perturb_gbuffer(*case.measure(), torch.float64)
        for kind, x in R.ratios(got, ref, R.PIXEL_KINDS).items():
            assert x <= 1e-12, (name, kind, x)


def test_the_float32_composition_stays_within_the_committed_figures():
    """F32 is what `python -m tests.normal_map_reference` prints: measured again here on every case of this file, and the
    share of a first draw that was rejected stays under 5 % for every seed."""
    worst = dict.fromkeys(R.KINDS, 0.)
    for name in list(MESHES) + list(PIXELS):
        case, _ = case_of(name)
        assert case.share < 0.05, (name, case.share)
        measured = R.measure_f32(case.per_scene(), []) if name in MESHES else R.measure_f32([], [case.measure()])
        for k, v in measured.items():
            assert v <= F32[k], '%s %s: committed %.3e, measured on this case %.3e' % (name, k, F32[k], v)
            worst[k] = max(worst[k], v)
    print({k: '%.3e' % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v >= 0.5 * F32[k], '%s: committed %.3e is not what these inputs give (%.3e)' % (k, F32[k], v)


def test_the_cases_hold_what_their_names_say():
    assert (TG_BLOCK, NM_BLOCK, NM_ITER) == (256, 256, 4) and FLAT == 1027
    case, _ = case_of('fan300')
    assert case.V == 301 and int((case.faces == 0).sum()) == 300
    assert case_of('triangle')[0].faces.tolist() == [[0, 1, 2]]
    cube = case_of('cube')[0]
    assert cube.V == 24 and len(cube.faces) == 12 and len(np.unique(cube.uv, axis=0)) == 24     # split seams: no two vertices share a uv
    assert sorted(case_of(k)[0].V for k in MESHES if k.startswith('strip') and k[5:].isdigit()) == [255, 256, 257]
    assert case_of('strip_w')[0].v.shape == (1, 257, 4) and case_of('scenes3')[0].v.shape == (3, 257, 3)
    assert sorted({LAYOUTS[k][0] for k in LAYOUTS}) == [7, 11, 12, 257]
    assert LAYOUTS['c7'][1:] == (0, 3) and LAYOUTS['c7r'][1] > LAYOUTS['c7r'][2]
    for name in ('strip256', 'fan300'):
        assert set(np.unique(case_of(name)[1]['tangents'][..., 3])) <= {-1., 1.}
    # the tori, from the reference alone: both signs of the handedness, normals all over the sphere, every face count from 1 to 6
    w = {name: case_of(name)[1]['tangents'][..., 3] for name in MESHES if name.startswith('torus')}
    assert w['torus'].shape == (1, 294) and (w['torus'] == 1.).all() and (w['torus_mirrored'] == -1.).all()
    assert w['torus_both'].shape == (1, 588) and (w['torus_both'][0, :294] == 1.).all() and (w['torus_both'][0, 294:] == -1.).all()
    assert w['torus_w3'].shape == (3, 588) and all(int((row == s).sum()) == 294 for row in w['torus_w3'] for s in (-1., 1.))
    both = case_of('torus_w3')[0]
    assert both.v.shape == (3, 588, 4) and both.faces[:520].max() == 293 and both.faces[520:].min() == 294 and len(both.faces) == 1040
    for name in w:
        case = case_of(name)[0]
        nz = np.abs(case.n[..., 2])
        assert nz.min() < 0.1 and nz.max() > 0.9, name
        assert sorted(set(np.bincount(case.faces.reshape(-1), minlength=case.V)[:294])) == [1, 2, 3, 6], name
        assert -(-case.V // TG_BLOCK) == (2 if case.V == 294 else 3)
    for name in PIXELS:
        case, ref = case_of(name)
        assert ref['valid'].all() and (ref['sin'] >= R.MIN_SIN).all() and (ref['z'] >= R.MIN_Z).all(), name


INVALID = {   # name -> (normal, tangent and handedness, normal-map texel): the four kinds of pixel that keep their normal
    'zero normal': ((0., 0., 0.), (1., 0., 0., 1.), (0.7, 0.4, 0.9)),
    'zero tangent': ((0., 0.6, 0.8), (0., 0., 0., 1.), (0.7, 0.4, 0.9)),
    'parallel tangent': ((0., 0., 2.), (0., 0., -3., 1.), (0.7, 0.4, 0.9)),
    'zero decoded vector': ((0., 0.6, 0.8), (1., 0., 0., -1.), (0.5, 0.5, 0.5)),
}


@pytest.mark.parametrize('kind', sorted(INVALID))
def test_an_invalid_pixel_keeps_its_normal_and_passes_the_gradient_to_it_alone(kind):
    from dirt_amd import lighting
    n, t, m = (torch.tensor([x, (0.3, -0.5, 0.8) if i == 0 else (0.2, 0.9, 0.1, 1.) if i == 1 else (0.6, 0.3, 0.8)], requires_grad=True)
               for i, x in enumerate(INVALID[kind]))     # the invalid pixel and a valid one beside it
    out = lighting.perturb_normals(n, t, m)
    assert torch.equal(out[0], n[0].detach()) and not torch.equal(out[1], n[1].detach())
    g = torch.tensor([[0.25, -1.5, 2.], [1., 1., 1.]])
    out.backward(g)
    assert torch.equal(n.grad[0], g[0]) and not t.grad[0].any() and not m.grad[0].any()
    assert all(bool(torch.isfinite(x.grad).all()) for x in (n, t, m)) and bool(t.grad[1].any()) and bool(m.grad[1].any())
    ref = R.perturb(n.detach().numpy(), t.detach().numpy(), m.detach().numpy(), grad_out=g.numpy())
    assert ref['valid'].tolist() == [False, True]
    assert np.array_equal(ref['out'][0], n[0].detach().numpy()) and np.array_equal(ref['d_normals'][0], g[0].numpy())
    assert not ref['d_tangents'][0].any() and not ref['d_normal_map'][0].any()


def test_degenerate_uvs_and_unnamed_vertices_give_no_tangent_and_finite_gradients():
    """Face (0, 1, 2) has collinear uvs and is the only face of vertices 0 and 1; vertex 5 is named by no face: t = 0, w = 1
    there, and every gradient is finite (zero from those vertices)."""
    from dirt_amd import lighting
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.2], [1., 1., 0.], [2., 0.5, 0.1], [5., 5., 5.]], requires_grad=True)
    n = torch.tensor([[0., 0., 1.]]).repeat(6, 1).requires_grad_(True)
    uv = torch.tensor([[0., 0.], [0.5, 0.5], [1., 1.], [1., 0.], [2., 0.3], [0., 0.]])
    f = torch.tensor([[0, 1, 2], [2, 3, 4]])
    out = lighting.vertex_tangents(v, n, uv, f)
    for k in (0, 1, 5):
        assert out[k].tolist() == [0., 0., 0., 1.]
    assert abs(float(out[3, :3].detach().norm()) - 1.) < 1e-6
    out.backward(torch.ones_like(out))
    assert bool(torch.isfinite(v.grad).all()) and bool(torch.isfinite(n.grad).all())
    assert not v.grad[[0, 1, 5]].any() and not n.grad[[0, 1, 5]].any() and bool(v.grad[3].any())
    ref = R.tangents(v.detach().numpy(), n.detach().numpy(), uv.numpy(), f.numpy(), np.ones((6, 4), np.float32))
    assert np.array_equal(ref['tangents'][[0, 1, 5]], np.tile([0., 0., 0., 1.], (3, 1))) and ref['det_share'][0] == 0.
    assert np.abs(ref['d_vertices'] - v.grad.numpy()).max() <= 1e-5 and np.abs(ref['d_normals'] - n.grad.numpy()).max() <= 1e-5


BAD_UVS = {'nan u': (0, np.nan), 'nan v': (1, np.nan), 'inf u': (0, np.inf)}
BAD_VERTEX = 13     # of a strip of 30: faces 11, 12, 13 name it; vertices 11, 12, 14, 15 keep one or two live faces each


def dead_face_case(kind):
    """A strip of 30 vertices whose vertex 13 has a non-finite uv, and the restatement of the mesh with the three faces that name
    it REMOVED (and a finite uv in its place): what the dead-face rule must give at every vertex, vertex 13 having no face left.
    -> (vertices, normals, uvs, faces, grad_out, reference)"""
    case = Mesh(seed=7020, kind='strip', size=30)
    uv = case.uv.copy()
    column, value = BAD_UVS[kind]
    uv[BAD_VERTEX, column] = value
    live = ~(case.faces == BAD_VERTEX).any(1)
    assert int(live.sum()) == len(case.faces) - 3
    ref = R.tangents(case.v[0], case.n[0], case.uv, case.faces[live], case.go[0])
    assert (ref['det_share'] >= R.MARGIN).all() and (ref['w_share'] >= R.MARGIN).all() and (ref['sin'] >= R.MIN_SIN).all()     # still off the discontinuities
    assert ref['valid'].tolist() == [k != BAD_VERTEX for k in range(30)]
    return case.v[0], case.n[0], uv, case.faces, case.go[0], ref


def check_dead_faces(got, ref, what):
    """the bad vertex: (0, 0, 0, 1) and no gradient; every other vertex: the mesh without the dead faces; all of it finite"""
    got = {k: R._f64(v) for k, v in got.items()}
    assert all(np.isfinite(v).all() for v in got.values()), what
    assert got['tangents'][BAD_VERTEX].tolist() == [0., 0., 0., 1.], what
    assert not got['d_vertices'][BAD_VERTEX].any() and not got['d_normals'][BAD_VERTEX].any(), what
    check(got, ref, R.TANGENT_KINDS, what)
    assert np.array_equal(got['tangents'][:, 3], ref['tangents'][:, 3]), what


@pytest.mark.parametrize('kind', sorted(BAD_UVS))
def test_a_face_with_a_non_finite_uv_is_dead_in_the_torch_form_and_the_restatement(kind):
    """A face is live iff its det is finite and non-zero; a dead face has a = b = c = d = 0 exactly.  The restatement of the mesh
    with the non-finite uv equals that of the mesh without the dead faces, element for element; `lighting.vertex_tangents`
    matches it in float64 (1e-12 of the masses) and in float32 (the kernels' allowance)."""
    v, n, uv, faces, go, ref = dead_face_case(kind)
    ruled = R.tangents(v, n, uv, faces, go)
    for key in ('tangents', 'd_vertices', 'd_normals', 'mass_tangents', 'mass_d_vertices', 'mass_d_normals'):
        assert np.array_equal(ruled[key], ref[key]), key
    assert (ruled['det_share'][BAD_VERTEX - 2:BAD_VERTEX + 1] == 0.).all()
    got = R.torch_tangents(v, n, uv, faces, go, torch.float64)
    for k, x in R.ratios(got, ref, R.TANGENT_KINDS).items():
        assert x <= 1e-12, (kind, k, x)
    check_dead_faces(got, ref, kind + ' float64')
    check_dead_faces(R.torch_tangents(v, n, uv, faces, go, torch.float32), ref, kind + ' float32')


# ---- CPU tests: the interface

def test_the_functions_are_reachable_under_the_reference_package_name():
    import dirt
    import dirt_amd
    assert dirt.geometry.vertex_tangents is dirt_amd.geometry.vertex_tangents
    assert dirt.shading.perturb_normals is dirt_amd.shading.perturb_normals
    assert dirt.lighting.vertex_tangents is dirt_amd.lighting.vertex_tangents
    assert dirt.lighting.perturb_normals is dirt_amd.lighting.perturb_normals
    assert 'perturb_normals' in dirt.__doc__ and 'vertex_tangents' in dirt.__doc__


def test_the_c_abi_declares_exports_and_builds_the_new_entry_points():
    from dirt_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for name in ('dirt_tangent_forward', 'dirt_tangent_backward', 'dirt_tangent_scratch_bytes', 'dirt_normal_map_forward',
                 'dirt_normal_map_backward'):
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert '#define DIRT_ABI_VERSION 4' in header and '#define DIRT_NORMAL_MAP_ENCODED 1u' in header and _lib.NORMAL_MAP_ENCODED == 1
    assert 'dirt_tangent.hip' in build.SOURCES and 'dirt_normal_map.hip' in build.SOURCES
    assert 'dirt_tangent.hip' not in build.PER_SOURCE_FLAGS and 'dirt_normal_map.hip' not in build.PER_SOURCE_FLAGS
    assert lib.dirt_tangent_scratch_bytes(3, 100, 50) == 3 * 100 * 3 * 4 and lib.dirt_tangent_scratch_bytes(-1, 100, 50) == 0


def test_the_new_kernels_use_no_scratch_memory():
    from dirt_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if 'tangent_' in k or 'normal_map_' in k}
    assert sorted(res) == ['dirt::normal_map_backward_kernel', 'dirt::normal_map_forward_kernel', 'dirt::tangent_forward_kernel',
                           'dirt::tangent_frame_grad_kernel', 'dirt::tangent_gather_kernel'], sorted(res)
    for name, v in res.items():
        assert v['scratch'] == 0 and v['vgpr'] <= 64 and v['lds'] <= 8192, (name, v)


def test_the_c_abi_refuses_bad_arguments_before_any_device_work():
    from dirt_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)     # never dereferenced: validation fails first
    err = lambda: lib.dirt_last_error().decode()   # noqa: E731
    INV = _lib.E_INVALID_ARGUMENT
    assert lib.dirt_tangent_forward(one, 3, one, one, one, one, one, one, -1, 4, 2, None) == INV
    assert err() == 'dirt_tangent_forward: negative sizes (B=-1 V=4 F=2)'
    assert lib.dirt_tangent_forward(one, 5, one, one, one, one, one, one, 1, 4, 2, None) == INV
    assert err() == 'dirt_tangent_forward: vertices have 5 components, 3 or 4'
    assert lib.dirt_tangent_forward(one, 3, None, one, one, one, one, one, 1, 4, 2, None) == INV
    assert err() == 'dirt_tangent_forward: vertices / normals / uvs / offsets is NULL'
    assert lib.dirt_tangent_forward(one, 3, one, one, one, one, one, None, 1, 4, 2, None) == INV
    assert err() == 'dirt_tangent_forward: tangents is NULL'
    assert lib.dirt_tangent_forward(one, 3, one, one, None, one, one, one, 1, 4, 2, None) == INV
    assert err() == 'dirt_tangent_forward: faces / entries is NULL'
    assert lib.dirt_tangent_forward(None, 3, None, None, None, None, None, None, 0, 4, 2, None) == 0 and err() == ''
    assert lib.dirt_tangent_forward(None, 3, None, None, None, None, None, None, 2, 0, 0, None) == 0
    assert lib.dirt_tangent_backward(one, 3, one, one, one, one, one, None, one, one, one, 1 << 20, 1, 4, 2, None) == INV
    assert err() == 'dirt_tangent_backward: grad_tangents is NULL'
    assert lib.dirt_tangent_backward(one, 3, one, one, one, one, one, one, one, one, one, 47, 1, 4, 2, None) == INV
    assert err() == 'dirt_tangent_backward: scratch is NULL or smaller than dirt_tangent_scratch_bytes (47 < 48)'
    assert lib.dirt_tangent_backward(one, 3, one, one, one, one, one, one, None, None, None, 0, 1, 4, 2, None) == 0     # nothing wanted
    assert lib.dirt_tangent_backward(None, 3, None, None, None, None, None, None, None, None, None, 0, 0, 4, 2, None) == 0

    def forward(scenes=1, pixels=8, cg=12, stride=3, on=0, ot=3, flags=1, g=one, m=one, out=one):
        return lib.dirt_normal_map_forward(g, m, out, scenes, pixels, cg, stride, on, ot, 1., flags, None)

    for kw, text in ((dict(scenes=-1), 'negative sizes (scenes=-1 pixels=8)'), (dict(scenes=65536), '65536 scenes, at most 65535'),
                     (dict(cg=6), '6 G-buffer channels, 7..1024'), (dict(cg=1025), '1025 G-buffer channels, 7..1024'),
                     (dict(stride=2), "map_stride=2, a pixel's texel is 3 floats"), (dict(flags=2), 'unknown flags 0x2'),
                     (dict(on=10), 'normals at channel 10 does not fit in 12 channels'),
                     (dict(ot=9), 'tangents at channel 9 does not fit in 12 channels'),
                     (dict(on=2, ot=4), 'tangents (channel 4) overlaps normals (channel 2)'),
                     (dict(on=4, ot=1), 'tangents (channel 1) overlaps normals (channel 4)'),
                     (dict(g=None), 'gbuffer / normal_map / out is NULL'), (dict(out=None), 'gbuffer / normal_map / out is NULL')):
        assert forward(**kw) == INV and err() == 'dirt_normal_map_forward: ' + text, kw
    assert forward(scenes=0, g=None, m=None, out=None) == 0 and err() == '' and forward(pixels=0, g=None, m=None, out=None) == 0
    back = lambda *p: lib.dirt_normal_map_backward(*p, 1, 8, 12, 3, 0, 3, 1., 1, None)   # noqa: E731
    assert back(one, one, None, one, one) == INV and err() == 'dirt_normal_map_backward: gbuffer / normal_map / grad_out is NULL'
    assert back(one, one, one, None, None) == 0     # nothing wanted
    assert lib.dirt_normal_map_backward(None, None, None, None, None, 3, 0, 12, 3, 0, 3, 1., 1, None) == 0


TOPOLOGY = None
V4, N4, UV4 = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 2)
G = torch.zeros(4, 5, 12)
M = torch.zeros(4, 5, 3)
CPU = ' runs on an MI355X only; there is no CPU fallback'


def _topology():
    global TOPOLOGY
    if TOPOLOGY is None:
        from dirt_amd import geometry
        TOPOLOGY = geometry.MeshTopology(torch.tensor([[0, 1, 2], [0, 2, 3]]), 4)
    return TOPOLOGY


def _refusals():
    from dirt_amd import geometry, shading
    top = _topology()
    vt, pn = geometry.vertex_tangents, shading.perturb_normals
    many = V4[None].expand(65536, 4, 3)
    return [
        (lambda: vt(torch.zeros(4, 2), N4, UV4, top), ValueError, 'vertex_tangents expects vertices [V, 3|4] or [B, V, 3|4], got (4, 2)'),
        (lambda: vt(V4.numpy(), N4, UV4, top), ValueError, 'vertex_tangents expects vertices [V, 3|4] or [B, V, 3|4], got (4, 3)'),
        (lambda: vt(V4.double(), N4, UV4, top), ValueError, 'vertex_tangents expects float32 vertices, got torch.float64'),
        (lambda: vt(V4, N4, UV4, top.faces), ValueError, "vertex_tangents expects a MeshTopology (build it once per mesh), got 'Tensor'"),
        (lambda: vt(torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 2), top), ValueError,
         'vertex_tangents: 5 vertices, the topology was built for 4'),
        (lambda: vt(V4, torch.zeros(4, 4), UV4, top), ValueError,
         "normals must have shape [4, 3] (the vertices' [4, 3] with 3 components), got [4, 4]"),
        (lambda: vt(torch.zeros(2, 4, 4), N4, UV4, top), ValueError,
         "normals must have shape [2, 4, 3] (the vertices' [2, 4, 4] with 3 components), got [4, 3]"),
        (lambda: vt(V4, N4.double(), UV4, top), ValueError, 'normals must be float32, got torch.float64'),
        (lambda: vt(V4, N4.to('meta'), UV4, top), ValueError, 'normals is on meta, the vertices on cpu'),
        (lambda: vt(V4, N4, torch.zeros(2, 4, 2), top), ValueError,
         'uvs must have shape [4, 2] (one pair per vertex, shared by the scenes), got [2, 4, 2]'),
        (lambda: vt(V4, N4, UV4.numpy(), top), ValueError, 'uvs must have shape [4, 2] (one pair per vertex, shared by the scenes), got [4, 2]'),
        (lambda: vt(V4, N4, UV4.half(), top), ValueError, 'uvs must be float32, got torch.float16'),
        (lambda: vt(V4, N4, UV4.to('meta'), top), ValueError, 'uvs is on meta, the vertices on cpu'),
        (lambda: vt(many, N4[None].expand(65536, 4, 3), UV4, top), ValueError, 'vertex_tangents: 65536 scenes, at most 65535'),
        (lambda: vt(V4, N4, UV4, top.to('meta')), ValueError,
         'vertex_tangents: the topology is on meta, the vertices on cpu (use topology.to(device))'),
        (lambda: vt(V4, N4, UV4, top), RuntimeError, 'dirt_amd.geometry.vertex_tangents' + CPU),
        (lambda: pn(torch.zeros(12), M, normals=0, tangents=3), ValueError,
         'perturb_normals expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (12,)'),
        (lambda: pn(G.numpy(), M, normals=0, tangents=3), ValueError,
         'perturb_normals expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (4, 5, 12)'),
        (lambda: pn(G.long(), M, normals=0, tangents=3), ValueError, 'perturb_normals expects a float32 gbuffer, got torch.int64'),
        (lambda: pn(G, M, normals=None, tangents=3), ValueError, 'normals must be the index of a G-buffer channel, got None'),
        (lambda: pn(G, M, normals=0, tangents=3.), ValueError, 'tangents must be the index of a G-buffer channel, got 3.0'),
        (lambda: pn(G, M, normals=10, tangents=3), ValueError, 'normals at channel 10 does not fit in the 12 channels of the G-buffer'),
        (lambda: pn(G, M, normals=0, tangents=9), ValueError, 'tangents at channel 9 does not fit in the 12 channels of the G-buffer'),
        (lambda: pn(G, M, normals=4, tangents=1), ValueError, 'tangents (channel 1) overlaps normals (channel 4)'),
        (lambda: pn(G, M, normals=0, tangents=2), ValueError, 'tangents (channel 2) overlaps normals (channel 0)'),
        (lambda: pn(G, [M], normals=0, tangents=3), ValueError, 'normal_map must be a floating-point tensor, got list'),
        (lambda: pn(G, M.long(), normals=0, tangents=3), ValueError, 'normal_map must be a floating-point tensor, got torch.int64'),
        (lambda: pn(G, torch.zeros(4, 5, 4), normals=0, tangents=3), ValueError,
         "normal_map must have shape [4, 5, 3] (the G-buffer's [4, 5, 12] with 3 channels), got [4, 5, 4]"),
        (lambda: pn(G, M.to('meta'), normals=0, tangents=3), ValueError, 'normal_map is on meta, the G-buffer on cpu'),
        (lambda: pn(G, M, normals=0, tangents=3, strength='2'), ValueError, "strength must be a number, got '2'"),
        (lambda: pn(G, M, normals=0, tangents=3, strength=True), ValueError, 'strength must be a number, got True'),
        (lambda: pn(G, M, normals=0, tangents=3), RuntimeError, 'dirt_amd.shading.perturb_normals' + CPU),
    ]


@pytest.mark.parametrize('index', range(32))
def test_every_refusal_in_full(index):
    """The full text of what `vertex_tangents` and `perturb_normals` refuse, from types, shapes, dtypes and devices alone."""
    table = _refusals()
    assert len(table) == 32
    call, error, text = table[index]
    with pytest.raises(error) as caught:
        call()
    assert str(caught.value) == text


# ---- GPU tests: vertex_tangents

def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def fused_tangents(case, dev, want=(True, True)):
    """-> dict of the fused call's results on a mesh case: tangents and the gradients wanted of (vertices, normals)"""
    from dirt_amd import geometry
    batched = case.scenes is not None
    v = _dev(dev, case.v if batched else case.v[0]).requires_grad_(want[0])
    n = _dev(dev, case.n if batched else case.n[0]).requires_grad_(want[1])
    topology = geometry.MeshTopology(_dev(dev, case.faces), case.V)
    out = geometry.vertex_tangents(v, n, _dev(dev, case.uv), topology)
    assert out.shape == v.shape[:-1] + (4,)
    if out.requires_grad:
        out.backward(_dev(dev, case.go if batched else case.go[0]))
    return {'tangents': out.detach(), 'd_vertices': v.grad, 'd_normals': n.grad}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(MESHES))
def test_vertex_tangents_against_the_restatement(gpu, name):
    case, ref = case_of(name)
    check(fused_tangents(case, gpu), ref, R.TANGENT_KINDS, name)


@pytest.mark.gpu
@pytest.mark.parametrize('want', [(True, False), (False, True)])
def test_vertex_tangents_with_one_gradient_wanted(gpu, want):
    case, ref = case_of('fan300')
    got = fused_tangents(case, gpu, want)
    assert (got['d_vertices'] is None) == (not want[0]) and (got['d_normals'] is None) == (not want[1])
    check(got, ref, R.TANGENT_KINDS, 'fan300 %s' % (want,))


@pytest.mark.gpu
def test_vertex_tangents_gives_the_same_bits_on_every_run(gpu):
    for name in ('fan300', 'scenes3', 'torus_both'):
        a, b = fused_tangents(case_of(name)[0], gpu), fused_tangents(case_of(name)[0], gpu)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)


@pytest.mark.gpu
def test_vertex_tangents_of_degenerate_uvs_and_empty_calls(gpu):
    """The degenerate-uv face and the unnamed vertex of the CPU test, on the GPU; a mesh without faces; no vertices; no scenes."""
    from dirt_amd import geometry
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.2], [1., 1., 0.], [2., 0.5, 0.1], [5., 5., 5.]], device=gpu, requires_grad=True)
    n = torch.tensor([[0., 0., 1.]], device=gpu).repeat(6, 1).requires_grad_(True)
    uv = torch.tensor([[0., 0.], [0.5, 0.5], [1., 1.], [1., 0.], [2., 0.3], [0., 0.]], device=gpu)
    f = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    go = np.ones((6, 4), np.float32)
    out = geometry.vertex_tangents(v, n, uv, geometry.MeshTopology(_dev(gpu, f), 6))
    out.backward(_dev(gpu, go))
    ref = R.tangents(v.detach().cpu().numpy(), n.detach().cpu().numpy(), uv.cpu().numpy(), f, go)
    assert out[[0, 1, 5]].tolist() == [[0., 0., 0., 1.]] * 3 and not v.grad[[0, 1, 5]].any() and not n.grad[[0, 1, 5]].any()
    check({'tangents': out.detach(), 'd_vertices': v.grad, 'd_normals': n.grad}, ref, R.TANGENT_KINDS, 'degenerate')
    empty = geometry.MeshTopology(torch.zeros(0, 3, dtype=torch.int32, device=gpu), 6)
    assert geometry.vertex_tangents(v, n, uv, empty).tolist() == [[0., 0., 0., 1.]] * 6
    none = geometry.MeshTopology(torch.zeros(0, 3, dtype=torch.int32, device=gpu), 0)
    for lead in ((), (0,), (2,)):
        vv = torch.zeros(lead + (0, 3), device=gpu, requires_grad=True)
        out = geometry.vertex_tangents(vv, torch.zeros(lead + (0, 3), device=gpu), torch.zeros(0, 2, device=gpu), none)
        assert out.shape == lead + (0, 4)
        out.sum().backward()
        assert vv.grad.shape == vv.shape


def fused_tangents_of(dev, v, n, uv, faces, go):
    """the fused call and its backward on arrays: vertices [.., V, 3|4], normals, uvs [V, 2], faces, grad_out [.., V, 4]"""
    from dirt_amd import geometry
    vt, nt = _dev(dev, v).requires_grad_(True), _dev(dev, n).requires_grad_(True)
    out = geometry.vertex_tangents(vt, nt, _dev(dev, uv), geometry.MeshTopology(_dev(dev, faces), v.shape[-2]))
    out.backward(_dev(dev, go))
    return {'tangents': out.detach(), 'd_vertices': vt.grad, 'd_normals': nt.grad}


@pytest.mark.gpu
@pytest.mark.parametrize('kind', sorted(BAD_UVS))
def test_a_face_with_a_non_finite_uv_is_dead_in_the_kernels(gpu, kind):
    """The CPU test's mesh through the three tangent kernels: the vertex with the bad uv gets (0, 0, 0, 1) and no gradient, every
    other vertex what the mesh without the dead faces gives, and nothing is NaN."""
    v, n, uv, faces, go, ref = dead_face_case(kind)
    check_dead_faces(fused_tangents_of(gpu, v, n, uv, faces, go), ref, kind)


@pytest.mark.gpu
@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_a_non_finite_position_empties_the_frames_of_its_faces_only(gpu, value):
    """One coordinate of vertex 13 of the strip of 30 is NaN or Inf.  Its faces stay live (the uvs are fine), so T is NaN at their
    five vertices 11..15, x . x > 0 fails there, and those get t = 0, w = 1, G_T = 0 and d n = 0; every gradient is finite, and all
    of it is what the restatement, which masks the same way, gives.  (torch's autograd is not compared: it may leave a NaN where
    the specification says 0.)"""
    case = Mesh(seed=7020, kind='strip', size=30)
    v = case.v[0].copy()
    v[BAD_VERTEX, 1] = value
    with np.errstate(all='ignore'):
        ref = R.tangents(v, case.n[0], case.uv, case.faces, case.go[0])
    near = np.unique(case.faces[(case.faces == BAD_VERTEX).any(1)])
    assert near.tolist() == [11, 12, 13, 14, 15] and ref['valid'].tolist() == [k not in near for k in range(30)]
    for key in ('tangents', 'd_vertices', 'd_normals', 'mass_tangents', 'mass_d_vertices', 'mass_d_normals'):
        assert np.isfinite(ref[key]).all(), key
    assert np.array_equal(ref['tangents'][near], np.tile([0., 0., 0., 1.], (5, 1))) and not ref['d_normals'][near].any()
    assert not ref['mass_tangents'][near].any() and not ref['mass_d_normals'][near].any() and not ref['d_vertices'][BAD_VERTEX].any()
    far = ref['valid']
    assert (ref['w_share'][far] >= R.MARGIN).all() and (ref['sin'][far] >= R.MIN_SIN).all()
    got = fused_tangents_of(gpu, v, case.n[0], case.uv, case.faces, case.go[0])
    check(got, ref, R.TANGENT_KINDS, 'position %s' % value)
    assert np.array_equal(got['tangents'].cpu().numpy()[:, 3], ref['tangents'][:, 3])
    assert bool(got['d_vertices'][near].any())     # (the live neighbours' gradients still reach vertices 11, 12, 14, 15)


@pytest.mark.gpu
def test_vertex_tangents_at_the_scene_limit(gpu):
    """B = 65 535, the most gridDim.y takes (65 536 is refused: test_every_refusal_in_full), of one triangle: the scenes repeat a
    table of 7 draws; scenes 0..6 against the restatement, and every scene b the bits of scene b % 7, forward and both gradients."""
    B, period = 65535, 7
    table = Mesh(seed=7021, kind='strip', size=3, scenes=period)
    ref = table.reference()
    which = np.arange(B) % period
    got = fused_tangents_of(gpu, table.v[which], table.n[which], table.uv, table.faces, table.go[which])
    assert got['tangents'].shape == (B, 3, 4) and got['d_vertices'].shape == (B, 3, 3)
    check({k: x[:period] for k, x in got.items()}, ref, R.TANGENT_KINDS, 'scene limit')
    at = torch.from_numpy(which).to(gpu)
    for k, x in got.items():
        assert torch.equal(x.view(torch.int32), x[:period].view(torch.int32)[at]), k


# ---- GPU tests: perturb_normals

def fused_perturb(case, dev, shape=None, want=(True, True), g=None, m=None):
    """-> dict of the fused call's results on a pixel case: out [n, Cg] and the gradients wanted of (G-buffer, normal map)"""
    from dirt_amd import shading
    shape = shape or (case.n,)
    g = (_dev(dev, case.g).reshape(shape + (case.cg,)) if g is None else g).detach().requires_grad_(want[0])
    m = (_dev(dev, case.m).reshape(shape + (3,)) if m is None else m).detach().requires_grad_(want[1])
    out = shading.perturb_normals(g, m, normals=case.on, tangents=case.ot, strength=case.strength, encoded=case.encoded)
    assert out.shape == g.shape and out.is_contiguous()
    if out.requires_grad:
        out.backward(_dev(dev, case.go).reshape(out.shape))
    flat = lambda x, c: None if x is None else x.reshape(-1, c)   # noqa: E731
    return {'out': out.detach().reshape(-1, case.cg), 'd_gbuffer': flat(g.grad, case.cg), 'd_normal_map': flat(m.grad, 3)}


def untouched_bits(case, got):
    """every channel but the normals holds the input's bits; every channel of d gbuffer but normals and tangents grad_out's"""
    keep = np.ones(case.cg, bool)
    keep[case.on:case.on + 3] = False
    assert np.array_equal(got['out'].cpu().numpy()[:, keep].view(np.uint32), case.g[:, keep].view(np.uint32))
    if got.get('d_gbuffer') is not None:
        keep[case.ot:case.ot + 4] = False
        assert np.array_equal(got['d_gbuffer'].cpu().numpy()[:, keep].view(np.uint32), case.go[:, keep].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(PIXELS))
def test_perturb_normals_against_the_restatement(gpu, name):
    case, ref = case_of(name)
    got = fused_perturb(case, gpu)
    check(got, ref, R.PIXEL_KINDS, name)
    untouched_bits(case, got)
    assert float((got['out'][:, case.on:case.on + 3].norm(dim=1) - 1.).abs().max()) <= 3e-7


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(13, 79), (1, 13, 79), (1027,)])
def test_perturb_normals_on_the_three_gbuffer_shapes(gpu, shape):
    case, ref = case_of('flat')
    assert int(np.prod(shape)) == case.n
    got = fused_perturb(case, gpu, shape)
    check(got, ref, R.PIXEL_KINDS, 'shape %s' % (shape,))
    untouched_bits(case, got)


@pytest.mark.gpu
def test_perturb_normals_of_several_scenes(gpu):
    """[B, H, W, Cg] with B = 3: the scenes are one run of pixels"""
    case = Pixels(seed=7150, layout='c11', n=3 * 7 * 51)
    got = fused_perturb(case, gpu, (3, 7, 51))
    check(got, case.reference(), R.PIXEL_KINDS, 'scenes')
    untouched_bits(case, got)


@pytest.mark.gpu
@pytest.mark.parametrize('want', [(True, False), (False, True)])
def test_perturb_normals_with_one_gradient_wanted(gpu, want):
    case, ref = case_of('c11')
    got = fused_perturb(case, gpu, want=want)
    assert (got['d_gbuffer'] is None) == (not want[0]) and (got['d_normal_map'] is None) == (not want[1])
    check(got, ref, R.PIXEL_KINDS, 'c11 %s' % (want,))
    untouched_bits(case, got)


@pytest.mark.gpu
def test_a_strided_normal_map_is_read_in_place_with_the_same_bits(gpu):
    """`tex[..., 5:8]` of an 8-channel look-up: read where it lies (no copy is made: `_stage.rows_in_place` hands the slice on),
    the same bits as from a contiguous copy; d normal_map comes back dense either way."""
    from dirt_amd import _stage
    case, ref = case_of('flat')
    tex = torch.randn(case.n, 8, device=gpu)
    tex[:, 5:8] = _dev(gpu, case.m)
    view = tex[:, 5:8]
    src, stride = _stage.rows_in_place(view, 3)
    assert src.data_ptr() == view.data_ptr() and stride == 8 and not view.is_contiguous()
    a, b = fused_perturb(case, gpu, m=view), fused_perturb(case, gpu, m=view.contiguous())
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a['d_normal_map'].is_contiguous()
    check(a, ref, R.PIXEL_KINDS, 'strided')
    # a map that no constant stride describes is copied, and gives the same
    c = fused_perturb(case, gpu, m=_dev(gpu, case.m).t().contiguous().t())
    assert all(torch.equal(a[k], c[k]) for k in a)


@pytest.mark.gpu
def test_invalid_pixels_mixed_into_a_span(gpu):
    """The four kinds of pixel that keep their normal, scattered over a workgroup's span: each returns its normal's bits and
    grad_out for it, zeros for its tangent and texel; its valid neighbours are unaffected."""
    case = Pixels(seed=7160, layout='c12', n=FLAT)
    rows = {kind: np.arange(5 + 7 * i, FLAT, 97) for i, kind in enumerate(sorted(INVALID))}
    for kind, r in rows.items():
        n, t, m = INVALID[kind]
        case.g[r, case.on:case.on + 3], case.g[r, case.ot:case.ot + 4], case.m[r] = n, t, m
    ref = case.reference()
    bad = np.concatenate(list(rows.values()))
    assert not ref['valid'][bad].any() and int(ref['valid'].sum()) == FLAT - len(bad)
    got = fused_perturb(case, gpu)
    check(got, ref, R.PIXEL_KINDS, 'invalid')
    untouched_bits(case, got)
    out, dg, dm = (got[k].cpu().numpy() for k in ('out', 'd_gbuffer', 'd_normal_map'))
    sl_n, sl_t = slice(case.on, case.on + 3), slice(case.ot, case.ot + 4)
    assert np.array_equal(out[bad][:, sl_n].view(np.uint32), case.g[bad][:, sl_n].view(np.uint32))
    assert np.array_equal(dg[bad][:, sl_n], case.go[bad][:, sl_n]) and np.array_equal(dg[bad][:, sl_t], case.go[bad][:, sl_t])
    assert not dm[bad].any()


@pytest.mark.gpu
def test_non_finite_pixels_stay_in_their_own_pixel(gpu):
    """Five kinds of non-finite pixel scattered over a workgroup's span at a stride of 97, one on the last pixel of a pass and one
    on the first of the next: a NaN or Inf normal, a NaN tangent, a NaN handedness, a NaN texel.  By the restatement each fails
    one of the three `> 0` tests, keeps its normal -- non-finite where it was -- and hands grad_out to it alone.  Every other
    pixel gives what it gives in the clean input: nothing leaks through the LDS rows or the tile walk."""
    case = Pixels(seed=7161, layout='c12', n=FLAT)
    clean = case.reference()
    on, ot = case.on, case.ot
    put = {   # kind -> (first row, array, column, value)
        'nan normal': (5, case.g, on + 1, np.nan), 'inf normal': (12, case.g, on, np.inf), 'nan tangent': (19, case.g, ot + 2, np.nan),
        'nan handedness': (NM_BLOCK - 1 - 2 * 97, case.g, ot + 3, np.nan), 'nan texel': (NM_BLOCK - 2 * 97, case.m, 0, np.nan)}
    rows = {kind: np.arange(first, FLAT, 97) for kind, (first, _, _, _) in put.items()}
    assert NM_BLOCK - 1 in rows['nan handedness'] and NM_BLOCK in rows['nan texel']
    for kind, (_, array, column, value) in put.items():
        array[rows[kind], column] = value
    bad = np.concatenate(list(rows.values()))
    good = np.ones(FLAT, bool)
    good[bad] = False
    assert len(np.unique(bad)) == len(bad) == FLAT - int(good.sum()) and len(bad) > 50
    with np.errstate(all='ignore'):
        dirty = case.reference()
    sl_n, sl_t = slice(on, on + 3), slice(ot, ot + 4)
    # what the restatement says of the bad rows: invalid, the normal kept as it is, grad_out to the normal alone
    assert not dirty['valid'][bad].any() and dirty['valid'][good].all()
    assert np.array_equal(dirty['out'][bad][:, sl_n], case.g[bad][:, sl_n].astype(np.float64), equal_nan=True)
    assert np.array_equal(dirty['d_gbuffer'][bad], case.go[bad].astype(np.float64)) and not dirty['d_normal_map'][bad].any()
    for key in ('out', 'd_gbuffer', 'd_normal_map'):     # ... and of the others: what the clean input gives
        assert np.array_equal(dirty[key][good], clean[key][good]), key
    got = fused_perturb(case, gpu)
    keys = [key for _, key in R.PIXEL_KINDS]
    where = torch.from_numpy(good).to(gpu)
    check({key: got[key][where] for key in keys}, {k: clean[k][good] for key in keys for k in (key, 'mass_' + key)}, R.PIXEL_KINDS, 'non-finite')
    untouched_bits(case, got)
    out, dg, dm = (got[k].cpu().numpy() for k in keys)
    assert np.array_equal(out[bad][:, sl_n].view(np.uint32), case.g[bad][:, sl_n].view(np.uint32))
    assert np.array_equal(np.isfinite(out), np.isfinite(case.g)) and np.isfinite(dg).all() and np.isfinite(dm).all()
    assert np.array_equal(dg[bad][:, sl_n], case.go[bad][:, sl_n]) and np.array_equal(dg[bad][:, sl_t], case.go[bad][:, sl_t])
    assert not dm[bad].any()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['c7r', 'c257'])
def test_the_c_abi_writes_nothing_outside_its_outputs(gpu, name):
    """Both entry points called through ctypes with every output between two guard zones: the zones keep their bits, the
    outputs match the restatement."""
    from dirt_amd import _lib
    lib = _lib.load()
    case, ref = case_of(name)
    GUARD, PAD = 1.5e30, 4096

    def guarded(count):
        return torch.full((PAD + count + PAD,), GUARD, device=gpu)

    g, m, go = _dev(gpu, case.g), _dev(gpu, case.m), _dev(gpu, case.go)
    out, dg, dm = guarded(case.n * case.cg), guarded(case.n * case.cg), guarded(case.n * 3)
    at = lambda t: t.data_ptr() + 4 * PAD   # noqa: E731
    stream = torch.cuda.current_stream(gpu).cuda_stream
    flags = _lib.NORMAL_MAP_ENCODED if case.encoded else 0
    tail = (1, case.n, case.cg, 3, case.on, case.ot, case.strength, flags, stream)
    assert lib.dirt_normal_map_forward(g.data_ptr(), m.data_ptr(), at(out), *tail) == 0, _lib.last_error()
    assert lib.dirt_normal_map_backward(g.data_ptr(), m.data_ptr(), go.data_ptr(), at(dg), at(dm), *tail) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for t in (out, dg, dm):
        assert bool((t[:PAD] == GUARD).all()) and bool((t[-PAD:] == GUARD).all())
    got = {'out': out[PAD:-PAD].reshape(case.n, case.cg), 'd_gbuffer': dg[PAD:-PAD].reshape(case.n, case.cg),
           'd_normal_map': dm[PAD:-PAD].reshape(case.n, 3)}
    check(got, ref, R.PIXEL_KINDS, 'c abi ' + name)
    untouched_bits(case, got)


@pytest.mark.gpu
@pytest.mark.parametrize('name,vertex_gradient', [('scenes3', True), ('torus_w3', True), ('torus_w3', False)])
def test_the_tangent_c_abi_writes_nothing_outside_its_outputs(gpu, name, vertex_gradient):
    """Both entry points through ctypes, three scenes, every output and the scratch between two guard zones: the zones keep
    their bits and the outputs match the restatement.  `torus_w3` has four-component vertices: grad_vertices is [3, 588, 4], its
    fourth components exactly 0 (the store that follows each triple stays inside its row).  Without grad_vertices (NULL, and
    scratch NULL, 0) the gather is not launched: d normals alone."""
    from dirt_amd import _lib, geometry
    lib = _lib.load()
    case, ref = case_of(name)
    GUARD, PAD = 1.5e30, 4096
    B, V, C = 3, case.V, case.components
    assert case.v.shape == (B, V, C)
    top = geometry.MeshTopology(_dev(gpu, case.faces), V)
    v, n, uv, go = _dev(gpu, case.v), _dev(gpu, case.n), _dev(gpu, case.uv), _dev(gpu, case.go)
    out, dv, dn, scratch = (torch.full((PAD + B * V * c + PAD,), GUARD, device=gpu) for c in (4, C, 3, 3))
    at = lambda t: t.data_ptr() + 4 * PAD   # noqa: E731
    stream = torch.cuda.current_stream(gpu).cuda_stream
    head = (v.data_ptr(), C, n.data_ptr(), uv.data_ptr(), top.faces.data_ptr(), top.offsets.data_ptr(), top.entries.data_ptr())
    nbytes = lib.dirt_tangent_scratch_bytes(B, V, top.num_faces)
    assert nbytes == B * V * 12
    wanted = (at(dv), at(dn), at(scratch), nbytes) if vertex_gradient else (None, at(dn), None, 0)
    assert lib.dirt_tangent_forward(*head, at(out), B, V, top.num_faces, stream) == 0, _lib.last_error()
    assert lib.dirt_tangent_backward(*head, go.data_ptr(), *wanted, B, V, top.num_faces, stream) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for t in (out, dv, dn, scratch):
        assert bool((t[:PAD] == GUARD).all()) and bool((t[-PAD:] == GUARD).all())
    got = {'tangents': out[PAD:-PAD].reshape(B, V, 4), 'd_vertices': dv[PAD:-PAD].reshape(B, V, C), 'd_normals': dn[PAD:-PAD].reshape(B, V, 3)}
    if vertex_gradient:
        assert not bool((scratch[PAD:-PAD] == GUARD).any())     # d loss / d T of every vertex of every scene
        assert C == 3 or not bool(got['d_vertices'][..., 3].any())
    else:
        assert bool((dv == GUARD).all()) and bool((scratch == GUARD).all())
        got['d_vertices'] = None
    check(got, ref, R.TANGENT_KINDS, 'c abi tangents ' + name)
    assert torch.equal(got['tangents'][..., 3], _dev(gpu, ref['tangents'][..., 3]).float())


@pytest.mark.gpu
def test_a_captured_graph_replays_both_stages_on_new_inputs(gpu):
    """No host synchronisation in either call or its backward: captured with torch.cuda.graph and replayed after the inputs
    were rewritten in place, the replay equals the eager call on the new contents, bit for bit."""
    from dirt_amd import geometry, shading
    mesh, pix = case_of('fan300')[0], case_of('c11')[0]
    other_mesh, other_pix = Mesh(**dict(MESHES['fan300'], seed=7170)), Pixels(**dict(PIXELS['c11'], seed=7171))
    top = geometry.MeshTopology(_dev(gpu, mesh.faces), mesh.V)
    v, n, uv, gt = (_dev(gpu, x) for x in (mesh.v[0], mesh.n[0], mesh.uv, mesh.go[0]))
    g, m, go = (_dev(gpu, x) for x in (pix.g, pix.m, pix.go))

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (v, n, g, m)]
        t = geometry.vertex_tangents(leaves[0], leaves[1], uv, top)
        out = shading.perturb_normals(leaves[2], leaves[3], normals=pix.on, tangents=pix.ot)
        return (t.detach(), out.detach()) + tuple(torch.autograd.grad([t, out], leaves, [gt, go]))

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        for dst, src in ((v, other_mesh.v[0]), (n, other_mesh.n[0]), (g, other_pix.g), (m, other_pix.m)):
            dst.copy_(_dev(gpu, src))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)
    check({'out': captured[1], 'd_gbuffer': captured[4], 'd_normal_map': captured[5]},
          R.perturb_gbuffer(other_pix.g, other_pix.m, pix.on, pix.ot, 1., True, pix.go), R.PIXEL_KINDS, 'replay')


# ---- GPU tests: end to end

def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_the_example_pipeline_against_the_torch_route(gpu):
    """examples/fit_normal_map_fused.py at 64 x 64: the texture's gradient through vertex_stage -> vertex_tangents ->
    rasterise_deferred -> sample_texture_uv -> perturb_normals -> shade_gbuffer_pbr against the same pipeline with
    `lighting.perturb_normals` and a `torch.cat` in the shader.  Both runs shade the same G-buffer bits, and both forms of
    the stage are within 4 x F32 of the same float64 value: their normals differ by some 1e-6, which the Cook-Torrance lobe at
    a roughness of 0.5 (D <= 1 / (pi a2) = 5) turns into at most 1e-5 of a pixel; the texture's gradient, a sum of such pixels
    added up by float atomics in either run, is held to 1e-4 of the reference gradient's L1 norm (per-element masses are not
    available through the rasteriser's backward).  Measured on an MI355X: 4.5e-8 and 3.3e-8."""
    ex = _load_example('fit_normal_map_fused')
    vertices, uvs, topology, truth = ex.scene(gpu)
    results = []
    for fused in (True, False):
        texture = truth.clone().requires_grad_(True)
        image = ex.render(vertices, uvs, topology, texture, 64, 64, fused=fused)
        (image ** 2).sum().backward()
        results.append((image.detach(), texture.grad))
    (image_f, grad_f), (image_t, grad_t) = results
    assert image_f.shape == (64, 64, 3) and bool(torch.isfinite(image_f).all()) and bool(torch.isfinite(grad_f).all())
    print('image %.3e, gradient %.3e of its L1 norm' % (float((image_f - image_t).abs().max()),
                                                         float((grad_f - grad_t).abs().sum()) / float(grad_t.abs().sum())))
    assert float((image_f - image_t).abs().max()) <= 1e-5
    assert float(grad_t[..., 3:].abs().sum()) > 0.
    assert float((grad_f - grad_t).abs().sum()) <= 1e-4 * float(grad_t.abs().sum())


@pytest.mark.gpu
def test_the_example_fit_lowers_its_loss(gpu):
    ex = _load_example('fit_normal_map_fused')
    losses, before, after = ex.fit(width=64, height=64, steps=8, device=gpu)
    assert np.isfinite(losses).all() and losses[-1] < losses[0] and after < before
