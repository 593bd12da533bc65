"""`dirt_amd.geometry` (dirt_geometry.hip) against the restatement of tests/geometry_reference.py: `lighting.vertex_normals`
and two matmuls composed on the CPU in float64, gradients by torch's autograd.  Every comparison is per element,
|gpu - ref64| <= tol * (L1 mass of the element's terms); an element of zero mass must equal the reference exactly;
non-finite values must sit in the same places.  No element is excluded: the generators keep every face of the
non-degenerate meshes away from zero area and zero angle (geometry_reference.MIN_AREA_RATIO, MIN_ANGLE_DEG).

The tolerances are measured, not chosen: the float32 composition (the same functions, CPU, float32, torch autograd -- the
implementation users had before the kernel) is run on `tolerance_cases()`, the inputs of the tests below, and its worst
|f32 - ref64| / mass per kind of result is F32[kind]; the kernel, which may reorder a vertex's sums and use the
hardware's reciprocal, gets 4 x that (the allowance of tests/test_shade.py).  Produced by

    python -m tests.geometry_reference
"""
import ctypes
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from tests import geometry_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32 = {                           # worst |f32 - ref64| / mass of the float32 composition on tolerance_cases()
    'clip': 1.73e-7,
    'world': 1.55e-7,
    'normals': 2.09e-5,
    'd_vertices': 5.10e-6,
    'd_model': 1.24e-7,
    'd_view_projection': 9.06e-8,
}
KERNEL = 4                        # the kernel's allowance over the float32 composition

SIZES = (1, 3, 4, 257, 5000, 75000)
WANT_SUBSETS = [tuple(w for w, on in zip(R.VALUE_KINDS, bits) if on) for bits in itertools.product((False, True), repeat=3)]
GRAD_PATTERNS = list(itertools.product((False, True), repeat=3))   # requires_grad of (vertices, model, view_projection)


def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _names():
    return ['v%d' % n for n in SIZES] + ['fan', 'unreferenced', 'pre_split', 'c4', 'b3_shared', 'b3_per_scene', 'b3_mixed', 'no_model',
                                         'no_view_projection', 'neither']


CASES = _names()

# The hubs of `hubs`: (vertex, blades) -- where each list sits in the kernels' grid and how its length compares with the switch
# to the wave path (lists of more than 64 entries) and with the wave's 64 lanes.  3433 vertices, 1713 faces.
HUBS = [(5, 65),        # one past the switch; lane 5, the first of three pending lanes of wave 0
        (37, 129),      # a second turn of the wave's loop; two rounds of 64 and one lane with a third entry
        (63, 64),       # exactly the switch: stays on its lane, the last of the wave
        (64, 128),      # lane 0 of wave 1
        (255, 127),     # the last lane of workgroup 0
        (256, 200),     # the first lane of workgroup 1
        (3432, 1000)]   # the last vertex, in the last, partly empty workgroup
LONG_HUBS = [h for h, blades in HUBS if blades > 64]
# Random inputs added after the F32 figures were measured: not part of tolerance_cases(); the float32 composition stays within
# the committed figures on them (test_extra_cases_stay_within_the_committed_figures), so the kernel's bound rests on the same
# ground.  name: seed (7101 put the float32 composition's `world` at 1.06 x its figure on hubs_b3_per_scene: not used).
EXTRA_CASES = {'hubs': 7100, 'hubs_b3_per_scene': 7103, 'hubs_c4_b2': 7102}


def case(name, want=R.VALUE_KINDS):
    """The keyword arguments of geometry_reference.compose for one comparison (the GPU runs get the same arrays).  `want`:
    the outputs that receive a gradient."""
    rng = np.random.default_rng(EXTRA_CASES[name] if name in EXTRA_CASES else 7000 + CASES.index(name))
    pre_split, batch = name == 'pre_split', 3 if 'b3' in name else (2 if 'b2' in name else None)
    if name == 'fan':
        v, f = R.fan_mesh(rng)
    elif name.startswith('hubs'):
        v, f = R.hubs_mesh(rng, HUBS)
    elif name == 'unreferenced':   # 57 vertices no face names, in front of, between and behind the others
        v, f = R.grid_mesh(rng, 200)
        keep = np.sort(rng.permutation(257)[:200])
        keep[0], keep[-1] = 3, 250
        keep = np.unique(np.concatenate([keep, np.arange(100, 130)]))[:200]
        full = rng.uniform(-1., 1., (257, 3)).astype(np.float32)
        full[keep] = v
        v, f = full, keep[f].astype(np.int32)
    elif name == 'pre_split':
        v, f = R.split_mesh(*R.grid_mesh(rng, 100))
    else:
        v, f = R.grid_mesh(rng, int(name[1:]) if name[0] == 'v' and name[1:].isdigit() else 257)
    if name in ('c4', 'unreferenced', 'hubs_c4_b2'):
        v = np.concatenate([v, rng.uniform(0.99, 1.01, (len(v), 1)).astype(np.float32)], 1)
    if batch:
        v = (v[None] + rng.uniform(-0.01, 0.01, (batch,) + v.shape)).astype(np.float32)
    model = None if name in ('no_model', 'neither') else R.random_model(rng, batch if name.endswith('b3_per_scene') else None)
    vp = None if name in ('no_view_projection', 'neither') else R.random_view_projection(rng, batch if name.endswith(('b3_per_scene', 'b3_mixed')) else None)
    shape = v.shape[:-1]
    grads = {'clip': rng.standard_normal(shape + (4,)).astype(np.float32), 'world': rng.standard_normal(shape + (4,)).astype(np.float32),
             'normals': rng.standard_normal(shape + (3,)).astype(np.float32)}
    return dict(vertices=v, faces=f, model=model, view_projection=vp, pre_split=pre_split, grads={k: g for k, g in grads.items() if k in want})


def tolerance_cases():
    """The inputs the float32 figures are measured on: every random input of the comparisons below, the gradient taken
    through every subset of the outputs where a test does.  The hand-made degenerate meshes are not part: they are a
    few exactly representable values."""
    for name in CASES:
        yield case(name)
    for name in ('v257', 'pre_split', 'b3_mixed'):
        for want in WANT_SUBSETS:
            yield case(name, want)


# ---------------------------------------------------------------------------------------------------------------- helpers

def close(got, ref, mass, tol, what):
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64).reshape(np.shape(ref))
    ref, mass = np.asarray(ref, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), '%s: non-finite values in other places than the restatement' % what
    err = np.where(fin, np.abs(got - np.where(fin, ref, 0.)), 0.)
    zero = fin & ~(mass > 0)
    assert np.all(err[zero] == 0.), '%s: %d elements of zero mass differ from the restatement' % (what, int((err[zero] != 0).sum()))
    pos = fin & (mass > 0) & np.isfinite(mass)
    ratio = float((err[pos] / mass[pos]).max()) if pos.any() else 0.
    print('%-60s worst |gpu - ref64| / mass = %.3e (tol %.3e)' % (what, ratio, tol))
    assert ratio <= tol, '%s: |gpu - ref64| / mass = %.3e > %.3e at element %d' % (what, ratio, tol, int(np.argmax(np.where(pos, err / np.where(pos, mass, 1.), 0.))))
    return ratio


def run_fused(kw, dev, want=R.VALUE_KINDS, requires=(True, True, True)):
    """-> ({output name: tensor or None}, {gradient name: tensor or None}) of vertex_stage on the arrays of `kw`"""
    from dirt_amd import geometry
    v = torch.from_numpy(kw['vertices']).to(dev).requires_grad_(requires[0])
    topology = geometry.MeshTopology(torch.from_numpy(kw['faces']).to(dev), int(kw['vertices'].shape[-2]))
    m = torch.from_numpy(kw['model']).to(dev).requires_grad_(requires[1]) if kw['model'] is not None else None
    p = torch.from_numpy(kw['view_projection']).to(dev).requires_grad_(requires[2]) if kw['view_projection'] is not None else None
    outs = dict(zip(R.VALUE_KINDS, geometry.vertex_stage(v, topology, m, p, pre_split=kw['pre_split'], want=want)))
    pairs = [(outs[k], torch.from_numpy(kw['grads'][k]).to(dev)) for k in R.VALUE_KINDS if outs[k] is not None and k in kw['grads']]
    if pairs and any(o.requires_grad for o, _ in pairs):
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    return outs, {'d_vertices': v.grad, 'd_model': m.grad if m is not None else None, 'd_view_projection': p.grad if p is not None else None}


def compare(kw, dev, what, want=R.VALUE_KINDS, requires=(True, True, True), factor=KERNEL):
    ref = R.compose(**kw)
    outs, grads = run_fused(kw, dev, want=want, requires=requires)
    for k in R.VALUE_KINDS:
        if k not in want or ref[k] is None:
            assert outs[k] is None, '%s: %s was not asked for (or has no view_projection) and is not None' % (what, k)
        else:
            assert outs[k].shape == ref[k].shape
            close(outs[k], ref[k], ref['mass_' + k], factor * F32[k], '%s %s' % (what, k))
    flowing = any(k in want and ref[k] is not None for k in kw['grads'])
    for k, on in zip(R.GRAD_KINDS, requires):
        if ref[k] is None or not on or not flowing:
            assert grads[k] is None, '%s: %s has a gradient nobody asked for' % (what, k)
        else:
            assert grads[k].shape == ref[k].shape
            close(grads[k], ref[k], ref['mass_' + k], factor * F32[k], '%s %s' % (what, k))
    return outs, grads


def brute_force_index(faces, num_vertices):
    lists = [[] for _ in range(num_vertices)]
    for f, tri in enumerate(np.asarray(faces).reshape(-1, 3)):
        for corner, vertex in enumerate(tri):
            lists[int(vertex)].append(3 * f + corner)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return offsets, np.asarray([e for x in lists for e in x], np.int32)


DEGENERATE = {   # small integers: every product of the composition is exact in float32, so a zero area is exactly zero there too
    'repeated_index': ([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 1], [4, 1, 3]], [[0, 1, 2], [1, 3, 2], [3, 3, 4], [4, 1, 4]]),
    'collinear': ([[0, 0, 0], [1, 1, 2], [2, 2, 4], [3, 3, 6], [0, 2, 1], [2, 0, 1]], [[0, 1, 2], [1, 2, 3], [0, 4, 5], [0, 3, 1]]),
    'coincident': ([[0, 0, 0], [2, 0, 0], [2, 0, 0], [0, 2, 0], [2, 0, 0], [1, 1, 3]], [[0, 1, 3], [1, 2, 4], [1, 2, 5], [2, 4, 4]]),
}


def degenerate_case(name, pre_split=False):
    v, f = DEGENERATE[name]
    rng = np.random.default_rng(9000 + list(DEGENERATE).index(name))
    v = np.asarray(v, np.float32)
    model = np.asarray([[0, 2, 0, 0], [-2, 0, 0, 0], [0, 0, 1, 0], [1, -3, 2, 1]], np.float32)   # a quarter turn, scales, a shift: exact
    grads = {'clip': rng.integers(-2, 3, (len(v), 4)).astype(np.float32), 'world': rng.integers(-2, 3, (len(v), 4)).astype(np.float32),
             'normals': rng.integers(-2, 3, (len(v), 3)).astype(np.float32)}
    return dict(vertices=v, faces=np.asarray(f, np.int32), model=model, view_projection=R.random_view_projection(rng), pre_split=pre_split, grads=grads)


# ---------------------------------------------------------------------------------------------------------------- CPU tests

def test_committed_tolerances_are_not_below_the_float32_composition():
    """The F32 constants restate what `python -m tests.geometry_reference` measures; the kernel's bound may not rest on a
    figure smaller than the float32 composition's own error."""
    measured = R.measure_f32(tolerance_cases())
    print(measured)
    for k, v in measured.items():
        assert F32[k] >= v, '%s: committed %.3e, measured %.3e' % (k, F32[k], v)
        assert F32[k] <= 1.25 * v + 1e-12, '%s: committed %.3e is more than the measured %.3e (rounded up)' % (k, F32[k], v)


def test_extra_cases_stay_within_the_committed_figures():
    """EXTRA_CASES are not part of what F32 was measured on; the float32 composition's own error on them is within the
    committed figures all the same, so 4 x F32 allows the kernel there what it allows it on tolerance_cases()."""
    measured = R.measure_f32(case(name) for name in EXTRA_CASES)
    print(measured)
    for k, v in measured.items():
        assert v <= F32[k], '%s: committed %.3e, measured on the extra cases %.3e' % (k, F32[k], v)


def test_meshes_keep_their_bounds():
    """Every face of the non-degenerate cases keeps its area and smallest angle above the stated bounds, in object space and
    after the model matrix; the float32 composition is finite on them, and every float64 result is within its own mass; the
    cases hold what their names say."""
    for name in CASES + list(EXTRA_CASES):
        kw = case(name)
        v, m = kw['vertices'], kw['model']
        for scene in (v if v.ndim == 3 else v[None]):
            area, angle = R.face_quality(scene, kw['faces'])
            assert area >= R.MIN_AREA_RATIO and angle >= R.MIN_ANGLE_DEG, (name, area, angle)
        if m is not None and not name.endswith('b3_per_scene'):
            v4 = np.concatenate([v[..., :3], v[..., 3:] if v.shape[-1] == 4 else np.ones_like(v[..., :1])], -1).astype(np.float64)
            area, angle = R.face_quality((v4 @ m.astype(np.float64)).reshape(-1, 4)[:v.shape[-2]], kw['faces'])
            assert area >= 0.8 * R.MIN_AREA_RATIO and angle >= 0.8 * R.MIN_ANGLE_DEG, (name, area, angle)
        if name == 'v75000':
            continue   # (the two passes below are slow there and add nothing: the tolerance test runs them anyway)
        r32 = R.compose(dtype=torch.float32, masses=False, **kw)
        r64 = R.compose(**kw)
        for k in R.VALUE_KINDS + R.GRAD_KINDS:
            if r64[k] is not None:
                assert bool(torch.isfinite(r32[k]).all()), (name, k)
                assert bool((r64[k].abs() <= r64['mass_' + k] * (1 + 1e-9) + 1e-300).all()), (name, k)
    assert len(case('v1')['faces']) == 0 and len(case('v3')['faces']) == 1 and len(case('v4')['faces']) == 2
    assert np.bincount(case('fan')['faces'].reshape(-1))[0] == 2000
    kw = case('unreferenced')
    assert len(np.setdiff1d(np.arange(257), kw['faces'])) == 57 and 0 not in kw['faces'] and 256 not in kw['faces']
    # the hubs sit where HUBS says, with lists of exactly those lengths, and every other vertex has one entry
    from dirt_amd import geometry, _lib
    for name in EXTRA_CASES:
        kw = case(name)
        V = kw['vertices'].shape[-2]
        assert (V, len(kw['faces'])) == (3433, 1713) and HUBS[-1][0] == V - 1 and V % 256 != 0
        assert kw['vertices'].shape == {'hubs': (V, 3), 'hubs_b3_per_scene': (3, V, 3), 'hubs_c4_b2': (2, V, 4)}[name]
        lengths = np.diff(geometry.MeshTopology(torch.from_numpy(kw['faces']), V).offsets.numpy())
        assert [(h, int(lengths[h])) for h, _ in HUBS] == HUBS
        assert np.all(np.delete(lengths, [h for h, _ in HUBS]) == 1)
    switch = _lib.GEOM_LONG_LIST_DEFAULT
    assert switch == 64 and LONG_HUBS == [5, 37, 64, 255, 256, 3432] and sorted(b for _, b in HUBS)[:2] == [switch, switch + 1]
    assert {b for _, b in HUBS} >= {127, 128, 129}
    assert sum(h // 64 == 0 and b > switch for h, b in HUBS) == 2 and sum(h // 64 == 0 for h, _ in HUBS) == 3   # wave 0: two turns, one list left to its lane


def test_mesh_topology_is_the_brute_force_inversion():
    from dirt_amd import geometry
    rng = np.random.default_rng(11)
    meshes = [(case(name)['faces'], case(name)['vertices'].shape[-2]) for name in ('v4', 'v257', 'v5000', 'fan', 'unreferenced', 'pre_split')]
    meshes.append((rng.integers(0, 50, (400, 3)).astype(np.int32), 50))                 # random triples: repeats inside a face happen
    meshes.append((np.asarray([[2, 2, 5], [5, 2, 2], [7, 7, 7]], np.int64), 9))         # a face repeating an index, int64
    meshes.append((np.zeros((0, 3), np.int32), 6))                                      # F = 0
    meshes.append((np.zeros((0, 3), np.int32), 0))
    for faces, nv in meshes:
        t = geometry.MeshTopology(torch.from_numpy(faces), nv)
        offsets, entries = brute_force_index(faces, nv)
        assert t.offsets.dtype == t.entries.dtype == t.faces.dtype == torch.int32
        assert np.array_equal(t.offsets.numpy(), offsets) and np.array_equal(t.entries.numpy(), entries)
        assert np.array_equal(t.faces.numpy(), faces) and t.num_vertices == nv and t.num_faces == len(faces)
        assert t.offsets.shape == (nv + 1,) and t.entries.shape == (3 * len(faces),)
    t = geometry.MeshTopology(torch.tensor([[2, 2, 5]]), 6)
    assert t.entries.tolist() == [0, 1, 2] and t.offsets.tolist() == [0, 0, 0, 2, 2, 2, 3]
    moved = t.to('cpu')
    assert isinstance(moved, geometry.MeshTopology) and moved.device.type == 'cpu' and torch.equal(moved.entries, t.entries)


def test_refuses_bad_arguments():
    from dirt_amd import geometry
    T = geometry.MeshTopology
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    for bad, nv, match in ((faces.reshape(-1), 4, 'faces .F, 3.'), (faces.reshape(3, 2), 4, 'faces .F, 3.'), (faces.float(), 4, 'int32 or int64'),
                           (faces, 3, 'outside'), (faces - 1, 4, 'outside'), (faces, -1, 'num_vertices'), (faces, 4., 'num_vertices'),
                           (faces.numpy(), 4, 'faces .F, 3.')):
        with pytest.raises(ValueError, match=match):
            T(bad, nv)
    topo = T(faces, 4)
    v = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match='runs on an MI355X only; there is no CPU fallback'):
        geometry.vertex_stage(v, topo)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        geometry.vertex_normals(v, topo)
    eye = torch.eye(4)
    for args, kw, match in (((torch.zeros(4, 2), topo), {}, 'expects vertices'), ((torch.zeros(4), topo), {}, 'expects vertices'),
                            ((torch.zeros(2, 2, 4, 3), topo), {}, 'expects vertices'), ((v.double(), topo), {}, 'float32 vertices'),
                            ((v, faces), {}, 'MeshTopology'), ((torch.zeros(5, 3), topo), {}, 'built for 4'),
                            ((v, topo, torch.zeros(3, 3)), {}, 'model must have shape'), ((v, topo, torch.zeros(2, 4, 4)), {}, 'model must have shape'),
                            ((torch.zeros(2, 4, 3), topo, torch.zeros(3, 4, 4)), {}, 'model must have shape'),
                            ((v, topo, eye, torch.zeros(4)), {}, 'view_projection must have shape'), ((v, topo, eye.double()), {}, 'model must be float32'),
                            ((v, topo, eye, eye.numpy()), {}, 'view_projection must have shape'),
                            ((v, topo, eye.to('meta')), {}, 'model is on meta'), ((v.to('meta'), topo), {}, 'topology is on cpu'),
                            ((v, topo), dict(want=('clip', 'colours')), 'want must be'), ((v, topo), dict(want='clip'), 'want must be')):
        with pytest.raises(ValueError, match=match):
            geometry.vertex_stage(*args, **kw)
    assert geometry._check_arguments(torch.zeros(2, 4, 4), topo, eye, None, True, ('normals', 'clip')) == (2, 4, 4, True, ('normals',), 1)
    assert geometry.LONG_LIST is None


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    for s in ('dirt_geometry_scratch_bytes', 'dirt_geometry_forward', 'dirt_geometry_backward'):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for cite in ('dirt/lighting.py:21-28,31-89', 'dirt/lighting.py:97-129', 'samples/deferred.py:40-51'):
        assert cite in header, cite
    assert '#define DIRT_GEOM_PRE_SPLIT 1u' in header and _lib.GEOM_PRE_SPLIT == 1 and 'DIRT_FLAG_PRE_SPLIT' not in header
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    good = dict(v=one, c=3, f=one, o=one, e=one, m=one, ms=1, p=one, ps=1, B=2, V=64, F=100, flags=0)

    def fwd(clip=one, world=one, normals=one, **over):
        a = dict(good, **over)
        return lib.dirt_geometry_forward(a['v'], a['c'], a['f'], a['o'], a['e'], a['m'], a['ms'], a['p'], a['ps'], clip, world, normals, a['B'], a['V'],
                                         a['F'], a['flags'], None)

    def bwd(gc=one, gw=one, gn=one, gv=one, gm=one, gp=one, scratch=one, nbytes=1 << 20, **over):
        a = dict(good, **over)
        return lib.dirt_geometry_backward(a['v'], a['c'], a['f'], a['o'], a['e'], a['m'], a['ms'], a['p'], a['ps'], gc, gw, gn, gv, gm, gp, scratch,
                                          nbytes, a['B'], a['V'], a['F'], a['flags'], None)

    bad = [dict(v=None), dict(o=None), dict(f=None), dict(e=None), dict(c=2), dict(c=5), dict(B=-1), dict(V=-1), dict(F=-2), dict(B=70000),
           dict(V=(1 << 28) + 1), dict(F=(1 << 29) + 1), dict(ms=3), dict(ps=5), dict(m=None), dict(p=None), dict(ms=0), dict(ps=0), dict(flags=2),
           dict(flags=1 << 24)]
    for over in bad:
        assert fwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_geometry_forward'), over
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_geometry_backward'), over
    assert fwd(p=None, ps=0) == _lib.E_INVALID_ARGUMENT                # clip wanted without a view_projection
    assert bwd(p=None, ps=0, gp=None) == _lib.E_INVALID_ARGUMENT       # a gradient for a clip output that cannot exist
    assert bwd(m=None, ms=0, gc=None) == _lib.E_INVALID_ARGUMENT       # grad_model without a model
    assert bwd(scratch=None) == _lib.E_INVALID_ARGUMENT and bwd(nbytes=8) == _lib.E_INVALID_ARGUMENT
    assert bwd(scratch=ctypes.c_void_p(18)) == _lib.E_INVALID_ARGUMENT
    with pytest.raises(ValueError, match='dirt_geometry_backward'):
        _lib.check(bwd(nbytes=8))
    # no scenes or no vertices: a success that launches nothing, whatever the pointers; nothing wanted likewise
    nothing = dict(v=None, f=None, o=None, e=None)
    assert fwd(clip=None, world=None, normals=None, B=0, **nothing) == 0 and fwd(V=0, F=0, **nothing) == 0
    assert bwd(gc=None, gw=None, gn=None, gv=None, gm=None, gp=None, scratch=None, nbytes=0, V=0, F=0, **nothing) == 0
    assert fwd(clip=None, world=None, normals=None) == 0 and bwd(gv=None, gm=None, gp=None, scratch=None, nbytes=0) == 0
    assert lib.dirt_last_error() == b''
    # scratch: three floats per vertex and scene, and one row of 32 floats per workgroup of 256 vertices and scene
    assert lib.dirt_geometry_scratch_bytes(1, 75000, 150000) == 4 * (75000 * 3 + 293 * 32)
    assert lib.dirt_geometry_scratch_bytes(3, 257, 0) == 4 * 3 * (257 * 3 + 2 * 32)
    assert lib.dirt_geometry_scratch_bytes(0, 5, 5) == 0 and lib.dirt_geometry_scratch_bytes(-1, 5, 5) == 0
    assert lib.dirt_geometry_scratch_bytes(1, (1 << 28) + 1, 5) == 0


def test_the_module_is_exported_under_both_package_names():
    import dirt
    import dirt_amd
    import dirt.geometry
    assert dirt.geometry is dirt_amd.geometry and dirt_amd.vertex_stage is dirt_amd.geometry.vertex_stage
    assert dirt_amd.MeshTopology is dirt_amd.geometry.MeshTopology and callable(dirt_amd.geometry.vertex_normals)
    from dirt_amd import build
    assert 'dirt_geometry.hip' in build.SOURCES
    res = {k: v for k, v in build.kernel_resources().items() if 'geometry_' in k}
    assert len(res) == 5 and all(v['scratch'] == 0 for v in res.values()), res


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_values_and_gradients_against_the_restatement(gpu, name):
    compare(case(name), gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['v257', 'pre_split', 'b3_mixed'])
@pytest.mark.parametrize('want', WANT_SUBSETS, ids=['+'.join(w) or 'nothing' for w in WANT_SUBSETS])
def test_every_subset_of_the_outputs(gpu, name, want):
    """Outputs not named in `want` are None; the gradients are those of the named ones alone."""
    compare(case(name, want), gpu, '%s want=%s' % (name, want), want=want)


@pytest.mark.gpu
@pytest.mark.parametrize('requires', GRAD_PATTERNS, ids=[''.join(n for n, on in zip('vmp', r) if on) or 'none' for r in GRAD_PATTERNS])
def test_every_pattern_of_requires_grad(gpu, requires):
    outs, grads = compare(case('b3_mixed'), gpu, 'requires_grad=%s' % (requires,), requires=requires)
    assert all(o.requires_grad == any(requires) for o in outs.values())


@pytest.mark.gpu
def test_the_wave_path_equals_the_lane_path(gpu):
    """The fan's hub is summed by a whole wave (2000 entries > 64); asked to leave every list to its lane
    (DIRT_GEOM_LONG_LIST(65535)) the library gives the same vertex within the kernel's tolerance, and every other vertex
    -- whose lists are short either way -- to the bit."""
    from dirt_amd import geometry, _lib
    kw = case('fan')
    ref = R.compose(**kw)
    outs, _ = run_fused(kw, gpu)
    assert geometry.LONG_LIST is None and _lib.GEOM_LONG_LIST_DEFAULT == 64
    try:
        geometry.LONG_LIST = 65535
        lane, _ = run_fused(kw, gpu)
    finally:
        geometry.LONG_LIST = None
    assert torch.equal(outs['normals'][1:], lane['normals'][1:])
    close(lane['normals'], ref['normals'], ref['mass_normals'], KERNEL * F32['normals'], 'fan, every list walked by its lane: normals')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(EXTRA_CASES))
def test_several_hubs_against_the_restatement(gpu, name):
    """Seven hubs in one mesh (HUBS): the wave path takes a second and a third pending list in one wave, from lanes other than
    0, in waves other than the first, in the last workgroup and in scenes past the first."""
    compare(case(name), gpu, name)


def _with_long_list(value, kw, dev):
    from dirt_amd import geometry
    assert geometry.LONG_LIST is None
    try:
        geometry.LONG_LIST = value
        return run_fused(kw, dev)
    finally:
        geometry.LONG_LIST = None


def _close_to(ref, outs, grads, what):
    for k in R.VALUE_KINDS + R.GRAD_KINDS:
        if ref[k] is not None:
            close((outs if k in R.VALUE_KINDS else grads)[k], ref[k], ref['mass_' + k], KERNEL * F32[k], '%s %s' % (what, k))


@pytest.mark.gpu
def test_several_hubs_wave_path_equals_the_lane_path(gpu):
    """`hubs` with every list left to its lane (DIRT_GEOM_LONG_LIST(65535)): the six hubs of more than 64 entries, and the
    gradients, are within the kernel's tolerance of the restatement both ways; every other vertex -- the hub of exactly 64
    included, whose list is walked by its lane either way -- has the same bits in every output."""
    kw = case('hubs')
    ref = R.compose(**kw)
    outs, grads = run_fused(kw, gpu)
    lane, lane_grads = _with_long_list(65535, kw, gpu)
    rest = torch.ones(kw['vertices'].shape[-2], dtype=torch.bool, device=gpu)
    rest[LONG_HUBS] = False
    assert int(rest.sum()) == len(rest) - 6
    for k in R.VALUE_KINDS:
        assert torch.equal(outs[k][rest], lane[k][rest]), k
    assert not torch.equal(outs['normals'], lane['normals'])   # (six sums of 65 to 1000 terms in two orders: the knob did something)
    _close_to(ref, outs, grads, 'hubs, the long lists summed by their wave:')
    _close_to(ref, lane, lane_grads, 'hubs, every list walked by its lane:')


@pytest.mark.gpu
@pytest.mark.parametrize('long_list', [1, 3])
@pytest.mark.parametrize('name', ['v257', 'c4', 'unreferenced', 'b3_mixed'])
def test_every_list_on_the_wave_path(gpu, name, long_list):
    """Grids (lists of 1 to 6 entries) with the switch at 1 -- nearly every lane of every wave pending, one turn of the wave's
    loop per vertex -- and at 3: walked and pending lists side by side in each wave (`unreferenced`: and live lanes with an
    empty list).  Within the usual bound of the restatement; a vertex whose list stays with its lane has the bits of the
    default run."""
    from dirt_amd import geometry
    kw = case(name)
    outs, _ = run_fused(kw, gpu)
    got, got_grads = _with_long_list(long_list, kw, gpu)
    _close_to(R.compose(**kw), got, got_grads, '%s, lists of more than %d on the wave path:' % (name, long_list))
    lengths = np.diff(geometry.MeshTopology(torch.from_numpy(kw['faces']), kw['vertices'].shape[-2]).offsets.numpy())
    walked = torch.from_numpy(lengths <= long_list).to(gpu)
    assert int(walked.sum()) >= (2 if long_list == 1 else 60) and int((~walked).sum()) >= 140   # (valence 6 inside the grid, 3 on its border)
    for k in R.VALUE_KINDS:
        assert torch.equal(outs[k][..., walked, :], got[k][..., walked, :]), k


def _presented(array, how, dev, transposed=False):
    """The values of `array` on the device as a plain tensor ('plain'), as a contiguous view that starts one float into its
    buffer ('misaligned': 4 mod 16 bytes) or as a non-contiguous view ('strided': the leading columns of a wider buffer; with
    `transposed`, for a matrix, the transpose of a tensor that holds the transposed values)"""
    t = torch.from_numpy(np.ascontiguousarray(array)).to(dev)
    if how == 'plain':
        return t
    if how == 'misaligned':
        flat = torch.zeros(t.numel() + 1, device=dev)
        flat[1:] = t.reshape(-1)
        view = flat[1:].view(t.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    if transposed:
        view = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    else:
        wide = torch.full(t.shape[:-1] + (t.shape[-1] + 3,), 7., device=dev)
        wide[..., :t.shape[-1]] = t
        view = wide[..., :t.shape[-1]]
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _run_presented(kw, dev, how, grads):
    """vertex_stage on the arrays of `kw` presented as `how`; grads: {output: array} presented the same way, or 'expanded':
    the stride-0 ones of out.sum().backward().  -> (outputs, leaves)"""
    from dirt_amd import geometry
    leaves = [_presented(kw[k], how, dev, transposed=k != 'vertices').detach().requires_grad_(True) for k in ('vertices', 'model', 'view_projection')]
    outs = geometry.vertex_stage(leaves[0], geometry.MeshTopology(torch.from_numpy(kw['faces']).to(dev), kw['vertices'].shape[-2]), *leaves[1:])
    if grads == 'expanded':
        sum(o.sum() for o in outs).backward()
    else:
        torch.autograd.backward(outs, [_presented(grads[k], how, dev) for k in R.VALUE_KINDS])
    return outs, leaves


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['v257', 'c4'])
def test_misaligned_and_non_contiguous_operands(gpu, name):
    """The same values as contiguous views 4 bytes past a 16-byte boundary (the kernels' 12- and 16-byte accesses to rows that
    are only 4-byte aligned) and as non-contiguous views (the wrapper's .contiguous() branches), the incoming gradients
    likewise -- a strided [.., :n] view is what the rasteriser's state hands back, an expanded one what .sum() does: the
    kernels see the same numbers in the same order, so every output and gradient equals the plain run's to the bit, and every
    leaf's .grad has the leaf's shape."""
    kw = case(name)
    plain, plain_leaves = _run_presented(kw, gpu, 'plain', kw['grads'])
    assert all(bool(l.grad.abs().max() > 0) for l in plain_leaves)
    for how in ('misaligned', 'strided'):
        outs, leaves = _run_presented(kw, gpu, how, kw['grads'])
        for k, a, b in zip(R.VALUE_KINDS, plain, outs):
            assert torch.equal(a, b), (how, k)
        for k, a, b in zip(R.GRAD_KINDS, plain_leaves, leaves):
            assert b.grad.shape == b.shape and torch.equal(a.grad, b.grad), (how, k)
    ones = {k: np.ones(o.shape, np.float32) for k, o in zip(R.VALUE_KINDS, plain)}
    _, want = _run_presented(kw, gpu, 'plain', ones)
    _, got = _run_presented(kw, gpu, 'plain', 'expanded')
    for k, a, b in zip(R.GRAD_KINDS, want, got):
        assert b.grad.shape == b.shape and torch.equal(a.grad, b.grad) and bool(a.grad.abs().max() > 0), ('expanded', k)


@pytest.mark.gpu
@pytest.mark.parametrize('pre_split', [False, True])
@pytest.mark.parametrize('name', list(DEGENERATE))
def test_degenerate_faces_follow_the_composition(gpu, name, pre_split):
    """A face naming a vertex twice, three collinear vertices, coincident vertices: zero face normals (0 / (0 + 1e-12)), zero
    vertex normals where nothing else contributes, and gradients that pass d n / 1e-12 to the cross product -- huge, finite,
    and in the places the float64 composition has them (compare() checks every element)."""
    kw = degenerate_case(name, pre_split)
    ref = R.compose(**kw)
    outs, grads = compare(kw, gpu, '%s pre_split=%s' % (name, pre_split))
    assert bool(torch.isfinite(grads['d_vertices']).all())
    # a face that names a vertex twice sends that vertex +x and -x, however large x is: nothing huge is left; the other two
    # kinds send them to different vertices
    huge = name != 'repeated_index'
    assert (float(ref['d_vertices'].abs().max()) > 1e10) == huge and (float(grads['d_vertices'].abs().max()) > 1e10) == huge


@pytest.mark.gpu
def test_degenerate_vertex_normals_are_zero(gpu):
    """vertex 5 of this mesh is named by zero-area faces only: its normal is exactly zero, as torch's is"""
    from dirt_amd import geometry
    v = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 0], [3, 3, 0], [4, 4, 0]], device=gpu)
    faces = torch.tensor([[0, 1, 2], [3, 4, 5], [5, 5, 0]], device=gpu, dtype=torch.int32)
    n = geometry.vertex_normals(v, geometry.MeshTopology(faces, 6))
    assert n[5].tolist() == [0., 0., 0.] and n[3].tolist() == [0., 0., 0.] and n[1].tolist() == [0., 0., 1.]
    from dirt_amd import lighting
    assert torch.equal(n, lighting.vertex_normals(v, faces))


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_backward_is_reentrant(gpu):
    for name in ('v75000', 'fan', 'b3_mixed'):
        kw = case(name)
        (o1, g1), (o2, g2) = run_fused(kw, gpu), run_fused(kw, gpu)
        for k in R.VALUE_KINDS:
            assert torch.equal(o1[k], o2[k]), (name, k)
        for k in R.GRAD_KINDS:
            assert torch.equal(g1[k], g2[k]), (name, k)     # bit for bit: gathers in list order, fixed-order sums, no atomics
    # backward twice over one forward (retain_graph=True)
    from dirt_amd import geometry
    kw = case('b3_mixed')
    v, m, p = (torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('vertices', 'model', 'view_projection'))
    outs = geometry.vertex_stage(v, geometry.MeshTopology(torch.from_numpy(kw['faces']).to(gpu), 257), m, p)
    gos = [torch.from_numpy(kw['grads'][k]).to(gpu) for k in R.VALUE_KINDS]
    a = torch.autograd.grad(outs, [v, m, p], gos, retain_graph=True)
    b = torch.autograd.grad(outs, [v, m, p], gos, retain_graph=True)
    for x, y, k in zip(a, b, R.GRAD_KINDS):
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr(), k
        assert torch.equal(x, g1[k]), k


@pytest.mark.gpu
def test_a_captured_step_replays_to_the_bits_of_eager(gpu):
    """vertex_stage makes no host synchronisation: a step (stage, loss, gradients) is captured with torch.cuda.graph --
    GraphedStep binds the rasteriser's inputs as leaves and cannot hold a stage in front of them -- and its replay, on new
    vertex values written in place, returns the loss and gradients of the eager step to the bit."""
    from dirt_amd import geometry
    kw = case('v5000')
    v, m, p = (torch.from_numpy(kw[k]).to(gpu) for k in ('vertices', 'model', 'view_projection'))
    topology = geometry.MeshTopology(torch.from_numpy(kw['faces']).to(gpu), 5000)
    target = torch.from_numpy(kw['grads']['normals']).to(gpu)

    def step():
        leaves = [t.detach().requires_grad_(True) for t in (v, m, p)]
        clip, world, normals = geometry.vertex_stage(*leaves[:1], topology, *leaves[1:])
        loss = (clip ** 2).mean() + (world[..., :3] * normals).sum() * 1e-3 + ((normals - target) ** 2).mean()
        return loss.detach(), torch.autograd.grad(loss, leaves)

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grads_g = step()
    with torch.no_grad():
        v += 0.001 * torch.from_numpy(kw['grads']['world'][:, :3]).to(gpu)
    graph.replay()
    loss_e, grads_e = step()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for a, b in zip(grads_g, grads_e):
        assert torch.equal(a, b) and bool(a.abs().max() > 0)


@pytest.mark.gpu
def test_reference_fixtures(gpu):
    """The vertex-normal entries of tests/golden/helpers_ref.npz (the reference's own dirt/lighting.py run on the seeded inputs
    of tests/golden/make_helpers_golden.py) within the 2e-6 the torch port is held to in tests/test_helpers_ref.py."""
    from dirt_amd import geometry
    from tests.golden import make_helpers_golden as gold
    want = np.load(os.path.join(ROOT, 'tests', 'golden', 'helpers_ref.npz'))
    x = gold.inputs()
    faces = torch.from_numpy(x['faces']).to(gpu)
    topology = geometry.MeshTopology(faces, x['verts'].shape[-2])
    split_v, split_f = R.split_mesh(x['verts'], x['faces'])
    for key, got in (('vertex_normals', geometry.vertex_normals(torch.from_numpy(x['verts']).to(gpu), topology)),
                     ('vertex_normals_single_w', geometry.vertex_normals(torch.from_numpy(x['verts4']).to(gpu), topology)),
                     ('vertex_normals_pre_split', geometry.vertex_normals(torch.from_numpy(split_v).to(gpu),
                                                                          geometry.MeshTopology(torch.from_numpy(split_f).to(gpu), split_v.shape[-2]),
                                                                          pre_split=True))):
        got = got.cpu().numpy()
        assert got.shape == want[key].shape, key
        scale = max(1.0, float(np.abs(want[key]).max()))
        assert np.allclose(got, want[key], rtol=2e-6, atol=2e-6 * scale), (key, float(np.abs(got - want[key]).max()))


@pytest.mark.gpu
def test_the_cube_of_the_deferred_sample_end_to_end(gpu):
    """examples/deferred_fused.py with its geometry() replaced by vertex_stage.  The stage's outputs against geometry()'s: both
    are float32 evaluations of one composition -- torch's within F32 of the float64 one, the kernel within 4 x that -- so they
    are within 5 x of each other, by the mass of the terms (the clip mass taken through view and projection one after the
    other, as geometry() multiplies them).  The shaded images: within one 8-bit level on >= 99.95 % of the pixels (the
    criterion of tests/test_oracle_ref.py for sample-versus-port images; the rasteriser is discontinuous in its input)."""
    import dirt_amd
    from dirt_amd import geometry, lighting, matrices
    ex, fused = _load_example('deferred'), _load_example('deferred_fused')
    verts_np, faces_np = ex.build_cube()
    view = matrices.compose(matrices.translation(torch.tensor([0., -1.5, -3.5], device=gpu)), matrices.rodrigues(torch.tensor([-0.3, 0., 0.], device=gpu)))
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=gpu), dim=0)
    model = matrices.rodrigues(torch.tensor([0., 0.5, 0.], device=gpu))
    projection = matrices.perspective_projection(near=0.1, far=20., right=0.1, aspect=float(ex.frame_height) / ex.frame_width).to(gpu)
    background = torch.zeros([ex.frame_height, ex.frame_width, 10], device=gpu)

    vertices_a = torch.from_numpy(verts_np).to(gpu).requires_grad_(True)
    clip_a, faces_a, attributes_a = ex.geometry(vertices_a, torch.from_numpy(faces_np).to(gpu), view)
    pixels_a = dirt_amd.rasterise_deferred(vertices=clip_a, vertex_attributes=attributes_a, faces=faces_a, background_attributes=background,
                                           shader_fn=fused.shader_fn, shader_additional_inputs=[view, light])

    vertices_b = torch.from_numpy(verts_np).to(gpu).requires_grad_(True)
    split, split_faces = lighting.split_vertices_by_face(vertices_b, torch.from_numpy(faces_np).to(gpu))
    topology = geometry.MeshTopology(split_faces, 36)
    clip_b, world_b, normals_b = geometry.vertex_stage(split, topology, model, view @ projection, pre_split=True)
    attributes_b = torch.cat([torch.ones_like(world_b[:, :1]), world_b[:, :3], torch.ones_like(normals_b), normals_b], dim=1)
    pixels_b = dirt_amd.rasterise_deferred(vertices=clip_b, vertex_attributes=attributes_b, faces=topology.faces, background_attributes=background,
                                           shader_fn=fused.shader_fn, shader_additional_inputs=[view, light])

    ref = R.compose(split.detach().cpu().numpy(), split_faces.cpu().numpy(), model.cpu().numpy(), (view @ projection).cpu().numpy(), pre_split=True)
    close(world_b[:, :3], attributes_a[:, 1:4].detach().cpu().numpy(), ref['mass_world'][:, :3], 5 * F32['world'], 'cube: world')
    close(normals_b, attributes_a[:, 7:10].detach().cpu().numpy(), ref['mass_normals'], 5 * F32['normals'], 'cube: normals')
    mass_clip = (ref['mass_world'] @ view.cpu().double().abs()) @ projection.cpu().double().abs()
    close(clip_b, clip_a.detach().cpu().numpy(), mass_clip, 5 * F32['clip'], 'cube: clip')
    a, b = (torch.round(p.detach() * 255.) for p in (pixels_a, pixels_b))
    share = float(((a - b).abs().amax(-1) <= 1.).double().mean())
    print('cube: %.4f %% of the pixels within one 8-bit level' % (100. * share))
    assert share >= 0.9995
    (pixels_b ** 2).mean().backward()
    assert bool(torch.isfinite(vertices_b.grad).all()) and bool(vertices_b.grad.abs().max() > 0)


@pytest.mark.gpu
def test_the_fitting_example_descends(gpu):
    """examples/fit_mesh_fused.py: vertex_stage -> rasterise_deferred with shade_gbuffer -> loss -> backward, for a few steps of
    gradient descent on the vertices: the losses are finite and the loop ends below where it began."""
    losses = _load_example('fit_mesh_fused').main(steps=12)
    assert len(losses) == 12 and all(np.isfinite(losses)) and losses[-1] < losses[0]
