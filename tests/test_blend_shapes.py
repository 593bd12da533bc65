"""`dirt_amd.blendshapes` (dirt_blend.hip) against the restatement of tests/blend_reference.py: the blend-shape composition
with the dense regressor on the CPU in float64, gradients by torch's autograd.  Every comparison is per element,
|gpu - ref64| <= tol * (L1 mass of the element's terms); an element of zero mass must equal the reference exactly;
non-finite values must sit in the same places.  No element is excluded.

The tolerances are measured, not chosen: the float32 composition (the same function, CPU, float32, torch autograd -- the
matmuls users wrote before the kernel) is run on `tolerance_cases()`, the inputs of the tests below, and its worst
|f32 - ref64| / mass per kind of result is F32[kind]; the kernel, which sums in another order, gets 4 x that (the allowance
of tests/test_shade.py, tests/test_geometry.py and tests/test_skinning.py).  Produced by

    python -m tests.blend_reference
"""
import ctypes
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import blend_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32 = {                           # worst |f32 - ref64| / mass of the float32 composition on tolerance_cases()
    'vertices': 2.6e-7,
    'joints': 1.7e-7,
    'd_template': 1.3e-7,
    'd_coefficients': 8.8e-8,
}
KERNEL = 4                        # the kernel's allowance over the float32 composition

# the constants of dirt_blend.hip the shapes bracket (test_the_cases_hold_what_their_names_say reads them out of the source)
SLAB, S, UNROLL, KR, SLOTS, AHEAD, AHEAD_ONE = 1024, 4, 8, 8, 32, 16, 32

# name: (V, K, Ks, J, scenes of the template, scenes of the coefficients, lengths of the regressor's rows or None: 1 to 12).
# V: one vertex; 63, 64 and 65 lanes' quads of elements (3 V = 252, 255, 258: the last quad whole, three elements, two); the
# last element of a slab and one past it (3 V = 1023, 1026); 33 slabs, one more than the reduce has slots.  K: 0, 1, either
# side of UNROLL = KR = 8 and of two of them, 300; either side of the rows a forward lane loads ahead: AHEAD_ONE = 32 for a
# single scene (k31, k32, k33), AHEAD = 16 for tiles of scenes (b5_k15, b5_k16, b5_k17).  Ks: 0, 1, K - 1, K.  J: 0, 1, 24, 256.  Rows: empty, one entry, longer
# than a wave, every vertex.  B: a batch of one; S and S + 1; 32 and 33 scenes of shared coefficients (one slab: 32 and 33
# rows for the reduce's 32 slots).
SHAPES = {
    'v1_k1_j1': (1, 1, 1, 1, None, None, None),
    'v84_k7': (84, 7, 7, 3, None, None, None),
    'v85_k8_ks0': (85, 8, 0, 3, None, None, None),
    'v86_k9_ks1': (86, 9, 1, 3, None, None, None),
    'v341_k16_ks15': (341, 16, 15, 24, None, None, None),
    'v342_k17': (342, 17, 17, 24, None, None, None),
    'k0': (70, 0, 0, 4, None, None, None),
    'k0_b3': (70, 0, 0, 4, 3, None, None),
    'k300_ks290': (70, 300, 290, 24, None, None, None),
    'j0': (257, 5, 5, 0, None, None, None),
    'j0_b2': (257, 5, 5, 0, 2, 2, None),
    'j256': (300, 12, 10, 256, None, None, None),
    'rows_0_1_100_200': (200, 6, 3, 4, None, None, (0, 1, 100, 200)),
    'slabs33': (10925, 3, 2, 2, None, None, None),
    'b1_template': (86, 9, 4, 3, 1, None, None),
    'b1_coefficients': (86, 9, 4, 3, None, 1, None),
    'b1_both': (86, 9, 4, 3, 1, 1, None),
    'b4_shared_template': (342, 10, 4, 24, None, 4, None),
    'b5_shared_template': (342, 10, 4, 24, None, 5, None),
    'b5_shared_coefficients': (342, 10, 4, 24, 5, None, None),
    'b5_both': (342, 10, 4, 24, 5, 5, None),
    'b32_shared_coefficients': (86, 9, 4, 3, 32, None, None),
    'b33_shared_coefficients': (86, 9, 4, 3, 33, None, None),
    'k31': (86, 31, 31, 3, None, None, None),
    'k32': (86, 32, 20, 3, None, None, None),
    'k33': (86, 33, 33, 3, None, None, None),
    'b5_k15': (86, 15, 15, 3, None, 5, None),
    'b5_k16': (86, 16, 9, 3, 5, 5, None),
    'b5_k17': (86, 17, 17, 3, 5, None, None),
}
CASES = list(SHAPES)
SOURCES = ('both', 'vertices', 'joints')                             # the outputs a gradient arrives from; the other arrives as None
PATTERN_CASES = ('b5_shared_template', 'b5_shared_coefficients', 'b5_both', 'v342_k17')   # the four combinations of operands
GRAD_PATTERNS = list(itertools.product((False, True), repeat=2))     # requires_grad of (template, coefficients)
EXACT = ((10925, None), (21846, None), (70, 33), (70, 65))           # (V, scenes of the template): 33 and 65 slabs; one slab x 33 and 65 scenes


def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _random(V, K, Ks, J, tb, cb, rows, seed):
    rng = np.random.default_rng(seed)
    lead = (tb or cb,) if (tb or cb) else ()
    return dict(template=rng.uniform(-1., 1., ((tb,) if tb else ()) + (V, 3)).astype(np.float32),
                coefficients=rng.standard_normal(((cb,) if cb else ()) + (K,)).astype(np.float32),
                directions=(rng.standard_normal((K, V, 3)) * 0.1).astype(np.float32),
                regressor=R.random_regressor(rng, J, V, rows) if J else None, joint_shapes=Ks,
                grad_vertices=rng.standard_normal(lead + (V, 3)).astype(np.float32),
                grad_joints=rng.standard_normal(lead + (J, 3)).astype(np.float32))


def case(name, source='both'):
    """The keyword arguments of blend_reference.compose for one comparison (the GPU runs get the same arrays); source: the
    outputs the gradient arrives from"""
    kw = _random(*SHAPES[name], seed=8500 + CASES.index(name))
    if source == 'vertices':
        kw['grad_joints'] = None
    if source == 'joints':
        kw['grad_vertices'] = None
    return kw


def smpl_case(scenes=2):
    """An SMPL-sized model: 6 890 vertices, 10 shape + 207 pose-corrective directions, 24 joints, per-scene coefficients"""
    return _random(6890, 217, 10, 24, None, scenes, None, seed=8600)


def tolerance_cases():
    """The inputs the float32 figures are measured on: every random input of the comparisons below.  The exact cases are
    not part: they are a few exactly representable values."""
    for name in CASES:
        yield case(name)
    for name in PATTERN_CASES:
        for source in SOURCES[1:]:
            yield case(name, source)
    yield smpl_case()


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


def shapes_of(kw, dev):
    from dirt_amd import blendshapes
    reg = None if kw['regressor'] is None else torch.from_numpy(kw['regressor']).to(dev)
    return blendshapes.BlendShapes(torch.from_numpy(kw['directions']).to(dev), reg, kw['joint_shapes'])


def run_fused(kw, dev, requires=(True, True)):
    """-> (vertices, joints, {gradient name: tensor or None}) of blend_shapes on the arrays of `kw`"""
    from dirt_amd import blendshapes
    t = torch.from_numpy(kw['template']).to(dev).requires_grad_(requires[0])
    c = torch.from_numpy(kw['coefficients']).to(dev).requires_grad_(requires[1])
    vertices, joints = blendshapes.blend_shapes(t, c, shapes_of(kw, dev))
    outs = [(o, torch.from_numpy(kw[g]).to(dev).reshape(o.shape)) for o, g in ((vertices, 'grad_vertices'), (joints, 'grad_joints')) if kw[g] is not None]
    if vertices.requires_grad and outs:
        torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
    return vertices, joints, {'d_template': t.grad, 'd_coefficients': c.grad}


def compare(kw, dev, what, requires=(True, True), factor=KERNEL):
    ref = R.compose(**kw)
    vertices, joints, grads = run_fused(kw, dev, requires=requires)
    for k, o in (('vertices', vertices), ('joints', joints)):
        assert o.shape == ref[k].shape and o.requires_grad == any(requires), k
        close(o, ref[k], ref['mass_' + k], factor * F32[k], '%s %s' % (what, k))
    for k, on in zip(R.GRAD_KINDS, requires):
        if not on:
            assert grads[k] is None, '%s: %s has a gradient nobody asked for' % (what, k)
        else:
            assert grads[k].shape == ref[k].shape
            close(grads[k], ref[k], ref['mass_' + k], factor * F32[k], '%s %s' % (what, k))
    return vertices, joints, grads, ref


def exact_case(V, scenes):
    """Small integers and binary fractions: the template and the gradients in -3 .. 3, directions in -2 .. 2, coefficients and
    regressor weights in {0.25, 0.5, 1, 2}: joint_directions are multiples of 0.25 and every product and sum of the
    composition is a multiple of 1 / 64 far below 2^24 / 64, exact in float32 in any order.  K = 3, Ks = 2, two joints with
    rows of 5 and 130 entries."""
    rng = np.random.default_rng(9500 + V + (scenes or 0))
    K, J = 3, 2
    reg = np.zeros((J, V), np.float32)
    for j, n in enumerate((5, min(130, V))):
        reg[j, rng.permutation(V)[:n]] = rng.choice(np.asarray([0.25, 0.5, 1., 2.], np.float32), n)
    lead = (scenes,) if scenes else ()
    return dict(template=rng.integers(-3, 4, lead + (V, 3)).astype(np.float32), coefficients=rng.choice(np.asarray([0.25, -0.5, 1., 2.], np.float32), (K,)),
                directions=rng.integers(-2, 3, (K, V, 3)).astype(np.float32), regressor=reg, joint_shapes=2,
                grad_vertices=rng.integers(-3, 4, lead + (V, 3)).astype(np.float32), grad_joints=rng.integers(-3, 4, lead + (J, 3)).astype(np.float32))


def brute_force_indices(reg):
    """(row_offsets, row_vertices, row_weights, column_offsets, column_joints, column_weights) of a dense regressor, by loops"""
    J, V = reg.shape
    ro, rv, rw, co, cj, cw = [0], [], [], [0], [], []
    for j in range(J):
        for v in range(V):
            if reg[j, v] != 0:
                rv.append(v), rw.append(reg[j, v])
        ro.append(len(rv))
    for v in range(V):
        for j in range(J):
            if reg[j, v] != 0:
                cj.append(j), cw.append(reg[j, v])
        co.append(len(cj))
    return [np.asarray(x, d) for x, d in ((ro, np.int32), (rv, np.int32), (rw, np.float32), (co, np.int32), (cj, np.int32), (cw, np.float32))]


# ---------------------------------------------------------------------------------------------------------------- CPU tests

def test_committed_tolerances_are_not_below_the_float32_composition():
    """The F32 constants restate what `python -m tests.blend_reference` measures; the kernel's bound may not rest on a figure
    smaller than the float32 composition's own error."""
    measured = R.measure_f32(tolerance_cases())
    print(measured)
    for k, v in measured.items():
        assert F32[k] >= v, '%s: committed %.3e, measured %.3e' % (k, F32[k], v)
        assert F32[k] <= 1.25 * v + 1e-12, '%s: committed %.3e is more than the measured %.3e (rounded up)' % (k, F32[k], v)


def test_the_restatement_is_smpls_formulation_and_within_its_masses():
    """SMPL regresses its joints from the shaped mesh: regressor @ (template + S beta), S the first Ks directions.  The
    restatement's joints use the float32 constant joint_directions instead; the two differ by its rounding alone, at most
    2^-24 of every term |c[k]| |w[j, v]| |directions[k, v]|.  Every float64 result is within its own mass."""
    for name in ('v342_k17', 'v341_k16_ks15', 'b5_both', 'b5_shared_template', 'rows_0_1_100_200', 'k300_ks290'):
        kw = case(name)
        r = R.compose(**kw)
        for k in R.VALUE_KINDS + R.GRAD_KINDS:
            assert bool((r[k].abs() <= r['mass_' + k] * (1 + 1e-9) + 1e-300).all()), (name, k)
        t, c, D, reg = (torch.from_numpy(kw[k]).double() for k in ('template', 'coefficients', 'directions', 'regressor'))
        Ks = kw['joint_shapes']
        shaped = t + torch.einsum('...k,kvc->...vc', c[..., :Ks], D[:Ks])
        rounding = 2. ** -24 * torch.einsum('...k,kjc->...jc', c[..., :Ks].abs(), torch.einsum('jv,kvc->kjc', reg.abs(), D[:Ks].abs()))
        assert bool(((torch.matmul(reg, shaped) - r['joints']).abs() <= rounding + 1e-15).all()), name
        assert torch.allclose(t + torch.einsum('...k,kvc->...vc', c, D), r['vertices'], rtol=1e-13, atol=1e-13), name


def test_the_cases_hold_what_their_names_say():
    """The constants the shapes bracket are those of the source, and every case reaches what it is for: a change of a constant
    fails here instead of leaving the cases short of the paths they were made for."""
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_blend.hip')).read()
    for name, value in (('BL_BLOCK', 256), ('BL_QUAD', 4), ('BL_S', S), ('BL_UNROLL', UNROLL), ('BL_KR', KR), ('BL_SLOTS', SLOTS), ('BL_AHEAD', AHEAD),
                        ('BL_AHEAD_ONE', AHEAD_ONE)):
        assert re.search(r'constexpr int %s = %d;' % (name, value), source), name
    assert SLAB == 256 * 4

    def slabs(name):
        return -(-3 * SHAPES[name][0] // SLAB)

    assert [3 * SHAPES[n][0] for n in ('v84_k7', 'v85_k8_ks0', 'v86_k9_ks1')] == [63 * 4, 64 * 4 - 1, 64 * 4 + 2]
    assert 3 * SHAPES['v341_k16_ks15'][0] == SLAB - 1 and slabs('v341_k16_ks15') == 1 and slabs('v342_k17') == 2
    assert slabs('slabs33') == SLOTS + 1
    assert [SHAPES[n][1] for n in ('v84_k7', 'v85_k8_ks0', 'v86_k9_ks1', 'v341_k16_ks15', 'v342_k17')] == [UNROLL - 1, UNROLL, UNROLL + 1, 2 * KR, 2 * KR + 1]
    assert [SHAPES[n][1] for n in ('k31', 'k32', 'k33')] == [AHEAD_ONE - 1, AHEAD_ONE, AHEAD_ONE + 1] and all(SHAPES[n][4:6] == (None, None) for n in ('k31', 'k32', 'k33'))
    assert [SHAPES[n][1] for n in ('b5_k15', 'b5_k16', 'b5_k17')] == [AHEAD - 1, AHEAD, AHEAD + 1] and all((SHAPES[n][4] or SHAPES[n][5]) == S + 1 for n in ('b5_k15', 'b5_k16', 'b5_k17'))
    assert SHAPES['k300_ks290'][1] > 30 * UNROLL and SHAPES['k300_ks290'][2] > 4 * 64     # the joints' k loop: more than four turns of a wave
    assert {SHAPES[n][3] for n in CASES} >= {0, 1, 24, 256}
    for name in CASES:
        V, K, Ks, J, tb, cb, rows = SHAPES[name]
        assert 0 <= Ks <= K
    assert {(SHAPES[n][1] - SHAPES[n][2], SHAPES[n][2]) for n in ('v85_k8_ks0', 'v86_k9_ks1', 'v341_k16_ks15', 'v342_k17')} == {(8, 0), (8, 1), (1, 15), (0, 17)}
    reg = case('rows_0_1_100_200')['regressor']
    assert ((reg != 0).sum(1) == (0, 1, 100, 200)).all() and 100 > 64
    assert any(not (case(n)['regressor'] != 0).any(0).all() for n in ('v342_k17',))       # a vertex no joint names
    assert [SHAPES[n][4:6] for n in ('b4_shared_template', 'b5_shared_template')] == [(None, S), (None, S + 1)]
    assert [SHAPES[n][4] * slabs(n) for n in ('b32_shared_coefficients', 'b33_shared_coefficients')] == [SLOTS, SLOTS + 1]
    assert case('b1_both')['template'].shape == (1, 86, 3) and case('b1_both')['coefficients'].shape == (1, 9)
    assert {(SHAPES[n][4] is not None, SHAPES[n][5] is not None) for n in PATTERN_CASES} == set(itertools.product((False, True), repeat=2))
    for V, scenes in EXACT:
        # the partial rows the second launch adds per direction: slabs, times the scenes for the shared coefficients
        assert -(-3 * V // SLAB) * (scenes or 1) in (SLOTS + 1, 2 * SLOTS + 1)
        kw = exact_case(V, scenes)
        ref = R.compose(**kw)
        ref32 = R.compose(dtype=torch.float32, masses=False, **kw)
        for k in R.VALUE_KINDS + R.GRAD_KINDS:
            assert 2 ** 24 > 64 * float(ref['mass_' + k].max()), k
            assert bool((64 * ref[k] == (64 * ref[k]).round()).all()) and torch.equal(ref32[k].double(), ref[k]), k
        # the test bites: a reduce that took only the first turn of its slots would write another d c
        g, D = torch.from_numpy(kw['grad_vertices']).double().reshape(-1, 3 * V), torch.from_numpy(kw['directions']).double().reshape(3, 3 * V)
        pad = -(-3 * V // SLAB) * SLAB - 3 * V
        rows = (torch.nn.functional.pad(g, (0, pad))[:, None, :] * torch.nn.functional.pad(D, (0, pad))[None]).reshape(g.shape[0], 3, -1, SLAB).sum(-1)
        rows = rows.permute(0, 2, 1).reshape(-1, 3)                                              # [scene x slab, K]
        assert len(rows) > SLOTS and not torch.equal(rows[:SLOTS].sum(0), rows.sum(0))


def test_blend_shapes_object_is_the_brute_force_construction():
    from dirt_amd import blendshapes
    rng = np.random.default_rng(21)
    for V, K, J, Ks in ((5, 3, 4, None), (7, 2, 3, 0), (8, 4, 2, 4), (1, 1, 1, 1), (6, 0, 2, None), (4, 2, 0, 1), (0, 2, 3, 2)):
        D = rng.standard_normal((K, V, 3)).astype(np.float32)
        reg = R.random_regressor(rng, J, V, rng.integers(0, 4, J)) if J and V else np.zeros((J, V), np.float32)
        if J > 1 and V:
            reg[1] = 0.                                                                            # a joint with an empty row
        if V > 2:
            reg[:, 2] = 0.                                                                         # a vertex no joint names
        s = blendshapes.BlendShapes(torch.from_numpy(D), torch.from_numpy(reg) if J else None, Ks)
        assert (s.num_shapes, s.num_vertices, s.num_joints, s.joint_shapes) == (K, V, J, K if Ks is None else Ks)
        assert s.stride % 4 == 0 and 3 * V <= s.stride < 3 * V + 4 and s.packed.shape == (K, s.stride) and s.packed.is_contiguous()
        assert np.array_equal(s.packed[:, :3 * V].numpy(), D.reshape(K, 3 * V)) and bool((s.packed[:, 3 * V:] == 0).all())
        assert torch.equal(s.directions(), torch.from_numpy(D))
        got = (s.row_offsets, s.row_vertices, s.row_weights, s.column_offsets, s.column_joints, s.column_weights)
        for a, b in zip(got, brute_force_indices(reg)):
            assert a.is_contiguous() and a.numpy().dtype == b.dtype and np.array_equal(a.numpy(), b)
        assert torch.equal(s.dense_regressor(), torch.from_numpy(reg))
        want = np.einsum('jv,kvc->kjc', reg.astype(np.float64), D[:s.joint_shapes].astype(np.float64)).astype(np.float32)
        assert s.joint_directions.shape == (s.joint_shapes, J, 3) and np.array_equal(s.joint_directions.numpy(), want)
        if J > 1 and V:
            assert int(s.row_offsets[1]) == int(s.row_offsets[2])
        if V > 2:
            assert int(s.column_offsets[2]) == int(s.column_offsets[3])
    assert [blendshapes.BlendShapes(torch.zeros(1, v, 3)).stride for v in (1, 2, 3, 4, 5)] == [4, 8, 12, 12, 16]
    s = blendshapes.BlendShapes(torch.ones(2, 3, 3), torch.tensor([[0., 2., 1.], [3., 0., 4.]]), 1)
    assert s.row_offsets.tolist() == [0, 2, 4] and s.row_vertices.tolist() == [1, 2, 0, 2] and s.row_weights.tolist() == [2., 1., 3., 4.]
    assert s.column_offsets.tolist() == [0, 1, 2, 4] and s.column_joints.tolist() == [1, 0, 0, 1] and s.column_weights.tolist() == [3., 2., 1., 4.]
    assert s.joint_directions.tolist() == [[[3.] * 3, [7.] * 3]]
    moved = s.to('cpu')
    assert isinstance(moved, blendshapes.BlendShapes) and moved.device.type == 'cpu' and torch.equal(moved.packed, s.packed)
    assert (moved.num_shapes, moved.num_vertices, moved.num_joints, moved.joint_shapes, moved.stride) == (2, 3, 2, 1, 12)
    learned = blendshapes.BlendShapes(torch.ones(2, 3, 3, requires_grad=True), torch.ones(2, 3, requires_grad=True))
    assert not any(getattr(learned, n).requires_grad for n in blendshapes.BlendShapes._TENSORS)   # constants: no gradient goes to them


def test_refuses_bad_arguments():
    from dirt_amd import blendshapes, _lib
    BS = blendshapes.BlendShapes
    D, reg = torch.zeros(4, 5, 3), torch.zeros(2, 5)
    for args, match in (((D.reshape(4, 15),), 'directions .K, V, 3.'), ((torch.zeros(4, 5, 2),), 'directions .K, V, 3.'), ((D.numpy(),), 'directions .K, V, 3.'),
                        ((D.double(),), 'float32 directions'), ((torch.zeros(1, 1, 3).expand(4097, 1, 3),), 'at most 4096 shapes'),
                        ((torch.zeros(1, 1, 3).expand(1, (1 << 26) + 1, 3),), 'at most 4096 shapes and %d vertices' % (1 << 26)),
                        ((D, torch.zeros(2, 4)), 'joint_regressor .J, 5.'), ((D, torch.zeros(5)), 'joint_regressor .J, 5.'), ((D, reg.numpy()), 'joint_regressor .J, 5.'),
                        ((D, reg.double()), 'float32 joint_regressor'), ((D, reg.to('meta')), 'joint_regressor is on meta'),
                        ((D, torch.zeros(257, 5)), '257 joints, at most 256'), ((D, reg, 5), 'joint_shapes'), ((D, reg, -1), 'joint_shapes'),
                        ((D, reg, 2.), 'joint_shapes'), ((D, reg, True), 'joint_shapes')):
        with pytest.raises(ValueError, match=match):
            BS(*args)
    assert _lib.BLEND_MAX_JOINTS == _lib.KINEMATICS_MAX_JOINTS
    s = BS(D, reg)
    t, c = torch.zeros(5, 3), torch.zeros(4)
    with pytest.raises(RuntimeError, match='runs on an MI355X only; there is no CPU fallback'):
        blendshapes.blend_shapes(t, c, s)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        blendshapes.blend_shapes(t[None], c[None], s)
    for args, match in (((t, c, (D, reg)), 'expects a BlendShapes'), ((torch.zeros(4, 3), c, s), 'template must have shape'), ((torch.zeros(5, 4), c, s), 'template must have shape'),
                        ((torch.zeros(15), c, s), 'template must have shape'), ((t.numpy(), c, s), 'template must have shape'), ((t.double(), c, s), 'template must be float32'),
                        ((t, torch.zeros(3), s), 'coefficients must have shape'), ((t, torch.zeros(1, 1, 4), s), 'coefficients must have shape'),
                        ((t, c.numpy(), s), 'coefficients must have shape'), ((t, c.double(), s), 'coefficients must be float32'),
                        ((t, c.to('meta'), s), 'coefficients is on meta'), ((t.to('meta'), c.to('meta'), s), 'BlendShapes is on cpu'),
                        ((torch.zeros(2, 5, 3), torch.zeros(3, 4), s), '2 scenes of template, 3 of coefficients'),
                        ((torch.zeros(1, 5, 3).expand(65536, 5, 3), c, s), '65536 scenes, at most 65535')):
        with pytest.raises(ValueError, match=match):
            blendshapes.blend_shapes(*args)
    assert blendshapes._check_arguments(t, c, s) == (1, 5, 4, 2, False)
    assert blendshapes._check_arguments(t[None], c, s) == (1, 5, 4, 2, True)
    assert blendshapes._check_arguments(t, c[None].repeat(6, 1), s) == (6, 5, 4, 2, True)
    assert blendshapes._check_arguments(t, c, BS(D)) == (1, 5, 4, 0, False)
    for bad in (torch.zeros(3), torch.zeros(2, 4), torch.zeros(0, 3), np.zeros((2, 3), np.float32)):
        with pytest.raises(ValueError, match='pose_corrective_features'):
            blendshapes.pose_corrective_features(bad)


def test_pose_corrective_features_against_a_hand_written_case():
    """A quarter turn about z: matrices.rodrigues gives, indexed [in, out], [[0, -1, 0], [1, 0, 0], [0, 0, 1]] -- the matrix
    cv2.Rodrigues gives for the same vector, which SMPL flattens row-major after taking the identity off.  The root joint is
    left out; a zero rotation gives zeros."""
    from dirt_amd import blendshapes, matrices
    rot = torch.tensor([[0.3, -0.2, 0.1], [0., 0., np.pi / 2], [0., 0., 0.], [np.pi / 2, 0., 0.]], dtype=torch.float32)
    f = blendshapes.pose_corrective_features(rot)
    assert f.shape == (27,) and f.dtype == torch.float32
    want = torch.tensor([-1., -1., 0., 1., -1., 0., 0., 0., 0.] + [0.] * 9 + [0., 0., 0., 0., -1., -1., 0., 1., -1.])
    assert torch.allclose(f, want, atol=1e-6), f
    full = matrices.rodrigues(rot, three_by_three=True)
    assert torch.equal(f.reshape(3, 3, 3), full[1:] - torch.eye(3))                      # as returned: no transpose
    assert not torch.allclose(f.reshape(3, 3, 3), full[1:].transpose(-1, -2) - torch.eye(3), atol=1e-3)
    batch = torch.stack([rot, 2 * rot])
    fb = blendshapes.pose_corrective_features(batch)
    assert fb.shape == (2, 27) and torch.equal(fb[0], f)
    assert blendshapes.pose_corrective_features(rot[:1]).shape == (0,)
    leaf = rot.clone().requires_grad_(True)
    blendshapes.pose_corrective_features(leaf).sum().backward()
    assert bool((leaf.grad[0] == 0).all()) and bool(leaf.grad[1:].abs().sum() > 0)       # differentiable; the root has no part


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    for s in ('dirt_blend_scratch_bytes', 'dirt_blend_forward', 'dirt_blend_backward'):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    assert '#define DIRT_BLEND_MAX_SHAPES %d' % _lib.BLEND_MAX_SHAPES in header and '#define DIRT_BLEND_MAX_JOINTS %d' % _lib.BLEND_MAX_JOINTS in header
    assert '#define DIRT_BLEND_MAX_VERTICES (1 << 26)' in header and _lib.BLEND_MAX_VERTICES == 1 << 26
    assert '#define DIRT_BLEND_MAX_ENTRIES (1 << 30)' in header and _lib.BLEND_MAX_ENTRIES == 1 << 30 and '#define DIRT_ABI_VERSION 4' in header
    assert _lib.BLEND_MAX_SHAPES >= 4096
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    good = dict(ts=1, cs=2, d=one, stride=192, jd=one, B=2, V=64, K=9, Ks=4, J=3, flags=0)

    def fwd(t=one, c=one, ro=one, rv=one, rw=one, vertices=one, joints=one, **over):
        a = dict(good, **over)
        return lib.dirt_blend_forward(t, a['ts'], c, a['cs'], a['d'], a['stride'], ro, rv, rw, a['jd'], vertices, joints, a['B'], a['V'], a['K'], a['Ks'],
                                      a['J'], a['flags'], None)

    def bwd(co=one, cj=one, cw=one, gv=one, gj=one, gt=one, gc=one, scratch=one, nbytes=1 << 20, **over):
        a = dict(good, **over)
        return lib.dirt_blend_backward(a['ts'], a['cs'], a['d'], a['stride'], co, cj, cw, a['jd'], gv, gj, gt, gc, scratch, nbytes, a['B'], a['V'], a['K'],
                                       a['Ks'], a['J'], a['flags'], None)

    bad = [dict(d=None), dict(d=ctypes.c_void_p(20)), dict(jd=None), dict(B=-1), dict(V=-1), dict(K=-1), dict(Ks=-1), dict(J=-1), dict(B=65536),
           dict(V=(1 << 26) + 1, stride=3 * (1 << 26) + 4), dict(K=4097), dict(J=257), dict(Ks=10), dict(ts=0), dict(ts=3), dict(cs=0), dict(cs=1, ts=5),
           dict(stride=191), dict(stride=188), dict(stride=194), dict(flags=1), dict(flags=1 << 31)]
    for over in bad:
        assert fwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_blend_forward'), over
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_blend_backward'), over
    for over in (dict(t=None), dict(c=None), dict(ro=None)):
        assert fwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_blend_forward'), over
    need = 4 * 32 * 1 * 2 * 1
    assert lib.dirt_blend_scratch_bytes(2, 64, 9) == need
    for over in (dict(co=None), dict(scratch=None), dict(nbytes=8), dict(nbytes=need - 1), dict(scratch=ctypes.c_void_p(18))):
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_blend_backward'), over
    with pytest.raises(ValueError, match='dirt_blend_backward.*dirt_blend_scratch_bytes'):
        _lib.check(bwd(nbytes=8))
    # no scenes or no vertices: a success that launches nothing, whatever the pointers; nothing wanted likewise
    assert fwd(t=None, c=None, ro=None, rv=None, rw=None, vertices=None, joints=None, B=0, ts=1, cs=1, d=None, jd=None) == 0
    assert fwd(t=None, c=None, ro=None, V=0, stride=0, d=None, jd=None) == 0 and fwd(vertices=None, joints=None) == 0
    assert fwd(vertices=None, J=0, ro=None, jd=None) == 0                                                     # no regressor: `joints` is ignored
    assert bwd(co=None, gv=None, gj=None, gt=None, gc=None, scratch=None, nbytes=0, V=0, stride=0, d=None, jd=None) == 0
    assert bwd(gt=None, gc=None, scratch=None, nbytes=0) == 0 and bwd(gt=None, K=0, Ks=0, d=None, scratch=None, nbytes=0) == 0
    assert lib.dirt_last_error() == b''
    # scratch: one row of 32 floats per (tile of 4 scenes, range of 8 directions, slab of 1024 elements)
    assert lib.dirt_blend_scratch_bytes(1, 6890, 217) == 4 * 32 * 1 * 28 * 21 and lib.dirt_blend_scratch_bytes(5, 342, 8) == 4 * 32 * 2 * 1 * 2
    assert lib.dirt_blend_scratch_bytes(0, 5, 5) == 0 and lib.dirt_blend_scratch_bytes(5, 0, 5) == 0 and lib.dirt_blend_scratch_bytes(5, 5, 0) == 0
    assert lib.dirt_blend_scratch_bytes(-1, 5, 5) == 0 and lib.dirt_blend_scratch_bytes(5, -1, 5) == 0 and lib.dirt_blend_scratch_bytes(5, 5, -1) == 0
    assert lib.dirt_blend_scratch_bytes(65536, 5, 5) == 0 and lib.dirt_blend_scratch_bytes(1, (1 << 26) + 1, 5) == 0 and lib.dirt_blend_scratch_bytes(1, 5, 4097) == 0


def test_the_module_is_exported_under_both_package_names():
    import dirt
    import dirt_amd
    import dirt.blendshapes
    assert dirt.blendshapes is dirt_amd.blendshapes and dirt_amd.blend_shapes is dirt_amd.blendshapes.blend_shapes
    assert dirt_amd.BlendShapes is dirt_amd.blendshapes.BlendShapes
    from dirt_amd import build
    assert 'dirt_blend.hip' in build.SOURCES and 'dirt_blend.hip' not in build.PER_SOURCE_FLAGS
    res = build.kernel_resources()
    blend = {k: v for k, v in res.items() if 'blend_' in k}
    assert len(blend) == 5 and all(v['scratch'] == 0 for v in blend.values()), blend
    assert all(v['occupancy'] >= 3 for v in blend.values()), blend     # the single-scene forward holds 32 rows: 3 waves per SIMD
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_blend.hip')).read()
    assert 'atomicAdd' not in source and 'atomic_' not in source


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_values_and_gradients_against_the_restatement(gpu, name):
    kw = case(name)
    vertices, joints, grads, _ = compare(kw, gpu, name)
    if name.startswith('b1'):
        assert vertices.shape == (1, 86, 3) and joints.shape == (1, 3, 3)
        for k, operand in zip(R.GRAD_KINDS, ('template', 'coefficients')):
            assert grads[k].shape == kw[operand].shape, k
    if name.startswith('k0'):
        assert torch.equal(vertices.cpu(), torch.from_numpy(kw['template']))             # K = 0 still copies the template
    if name.startswith('j0'):
        assert joints.shape[-2:] == (0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize('name', PATTERN_CASES)
@pytest.mark.parametrize('source', SOURCES)
@pytest.mark.parametrize('requires', GRAD_PATTERNS, ids=[''.join(n for n, on in zip('tc', r) if on) or 'none' for r in GRAD_PATTERNS])
def test_every_pattern_of_requires_grad_and_every_source_of_the_gradient(gpu, name, source, requires):
    compare(case(name, source), gpu, '%s from %s requires_grad=%s' % (name, source, requires), requires=requires)


@pytest.mark.gpu
@pytest.mark.parametrize('V,scenes', EXACT)
def test_more_rows_than_slots_exactly(gpu, V, scenes):
    """exact_case: every sum is exact in float32 in any order (checked on the CPU by test_the_cases_hold_what_their_names_say),
    so the kernels equal the float64 composition to the bit: a partial row left out or added twice cannot hide under a
    tolerance.  33 and 65 rows per direction for the reduce's 32 slots: slabs of one scene, and scenes of one slab under
    shared coefficients."""
    for source in SOURCES:
        kw = exact_case(V, scenes)
        if source != 'both':
            kw['grad_joints' if source == 'vertices' else 'grad_vertices'] = None
        compare(kw, gpu, 'exact V=%d scenes=%s from %s' % (V, scenes, source), factor=0.)


def _presented(array, how, dev):
    """The values of `array` on the device as a plain tensor ('plain'), as a contiguous view that starts one float into its
    buffer ('misaligned': 4 mod 16 bytes) or as a non-contiguous view ('strided': the leading columns of a wider buffer)"""
    t = torch.from_numpy(np.ascontiguousarray(array)).to(dev)
    if how == 'plain':
        return t
    if how == 'misaligned':
        flat = torch.zeros(t.numel() + 1, device=dev)
        flat[1:] = t.reshape(-1)
        view = flat[1:].view(t.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    if t.dim() == 1:                                                                       # every other element of a buffer twice as long
        buf = torch.full((2 * t.shape[0],), 7., device=dev)
        buf[::2] = t
        view = buf[::2]
    else:
        buf = torch.full(t.shape[:-1] + (t.shape[-1] + 3,), 7., device=dev)
        buf[..., :t.shape[-1]] = t
        view = buf[..., :t.shape[-1]]
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _run_presented(kw, dev, how, expanded=False):
    from dirt_amd import blendshapes
    leaves = [_presented(kw[k], how, dev).detach().requires_grad_(True) for k in ('template', 'coefficients')]
    vertices, joints = blendshapes.blend_shapes(leaves[0], leaves[1], shapes_of(kw, dev))
    if expanded:
        (vertices.sum() + joints.sum()).backward()
    else:
        torch.autograd.backward([vertices, joints], [_presented(kw['grad_vertices'], how, dev), _presented(kw['grad_joints'], how, dev)])
    return vertices, joints, leaves


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['v342_k17', 'b5_both'])
def test_misaligned_and_non_contiguous_operands(gpu, name):
    """The same values as contiguous views 4 bytes past a 16-byte boundary (the kernels' 16-byte accesses to rows that are only
    4-byte aligned) and as non-contiguous views (the wrapper's .contiguous() branches), the incoming gradients likewise, and
    the expanded gradient of .sum(): the kernels see the same numbers in the same order, so the outputs and every gradient
    equal the plain run's to the bit, and every leaf's .grad has the leaf's shape."""
    kw = case(name)
    v0, j0, plain = _run_presented(kw, gpu, 'plain')
    assert all(bool(l.grad.abs().max() > 0) for l in plain)
    for how in ('misaligned', 'strided'):
        v1, j1, leaves = _run_presented(kw, gpu, how)
        assert torch.equal(v0, v1) and torch.equal(j0, j1), how
        for k, a, b in zip(R.GRAD_KINDS, plain, leaves):
            assert b.grad.shape == b.shape and torch.equal(a.grad, b.grad), (how, k)
    ones = dict(kw, grad_vertices=np.ones_like(kw['grad_vertices']), grad_joints=np.ones_like(kw['grad_joints']))
    _, _, want = _run_presented(ones, gpu, 'plain')
    _, _, got = _run_presented(kw, gpu, 'plain', expanded=True)
    for k, a, b in zip(R.GRAD_KINDS, want, got):
        assert b.grad.shape == b.shape and torch.equal(a.grad, b.grad) and bool(a.grad.abs().max() > 0), ('expanded', k)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_backward_is_reentrant(gpu):
    from dirt_amd import blendshapes
    for name in ('slabs33', 'k300_ks290', 'b33_shared_coefficients', 'b5_shared_template', 'b5_both'):
        kw = case(name)
        (v1, j1, g1), (v2, j2, g2) = run_fused(kw, gpu), run_fused(kw, gpu)
        assert torch.equal(v1, v2) and torch.equal(j1, j2), name
        for k in R.GRAD_KINDS:
            assert torch.equal(g1[k], g2[k]), (name, k)     # bit for bit: fixed-order sums, no atomics
    # backward twice over one forward (retain_graph=True)
    t, c = (torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('template', 'coefficients'))
    outs = blendshapes.blend_shapes(t, c, shapes_of(kw, gpu))
    go = [torch.from_numpy(kw[k]).to(gpu) for k in ('grad_vertices', 'grad_joints')]
    a = torch.autograd.grad(outs, [t, c], go, retain_graph=True)
    b = torch.autograd.grad(outs, [t, c], go, retain_graph=True)
    for x, y, k in zip(a, b, R.GRAD_KINDS):
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr(), k
        assert torch.equal(x, g1[k]), k


@pytest.mark.gpu
def test_a_scene_has_the_same_bits_alone_and_in_a_batch(gpu):
    """A single scene runs the forward with 32 rows loaded ahead, a batch with tiles of four scenes and 16: the blocks of the
    sum are the same eight directions in both, so scene b of a batch equals that scene run alone, to the bit (K = 300: both
    main loops and both tails)."""
    from dirt_amd import blendshapes
    kw = _random(342, 300, 290, 24, 5, 5, None, seed=8700)
    shapes = shapes_of(kw, gpu)
    t, c = (torch.from_numpy(kw[k]).to(gpu) for k in ('template', 'coefficients'))
    vertices, joints = blendshapes.blend_shapes(t, c, shapes)
    for b in range(5):
        v1, j1 = blendshapes.blend_shapes(t[b], c[b], shapes)
        assert torch.equal(v1, vertices[b]) and torch.equal(j1, joints[b]), b


@pytest.mark.gpu
def test_a_captured_step_replays_to_the_bits_of_eager(gpu):
    """blend_shapes makes no host synchronisation: a step (stage, loss, gradients) is captured with torch.cuda.graph and its
    replay, on new coefficient values written in place, returns the loss and gradients of the eager step to the bit."""
    from dirt_amd import blendshapes
    kw = case('b5_shared_template')
    t, c = (torch.from_numpy(kw[k]).to(gpu) for k in ('template', 'coefficients'))
    shapes = shapes_of(kw, gpu)
    target, joint_target = (torch.from_numpy(kw[k]).to(gpu) for k in ('grad_vertices', 'grad_joints'))

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (t, c)]
        vertices, joints = blendshapes.blend_shapes(leaves[0], leaves[1], shapes)
        loss = ((vertices - target) ** 2).mean() + ((joints - joint_target) ** 2).sum() * 1e-2
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
        c += 0.01 * torch.from_numpy(np.random.default_rng(5).standard_normal(c.shape).astype(np.float32)).to(gpu)
    graph.replay()
    loss_e, grads_e = step()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for a, b in zip(grads_g, grads_e):
        assert torch.equal(a, b) and bool(a.abs().max() > 0)


@pytest.mark.gpu
def test_the_torch_composition_agrees_at_smpl_size(gpu):
    """The composition a user writes in torch on the GPU (template + c @ D, a dense-regressor einsum, autograd) against the
    kernel at SMPL size: both are float32 evaluations of one composition -- torch's within F32 of the float64 one, the kernel
    within 4 x that -- so they are within (1 + KERNEL) x F32 of each other, by the mass of the terms."""
    from dirt_amd import blendshapes
    kw = smpl_case()
    ref = R.compose(**kw)
    shapes = shapes_of(kw, gpu)
    go = [torch.from_numpy(kw[k]).to(gpu) for k in ('grad_vertices', 'grad_joints')]
    t, c = (torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('template', 'coefficients'))
    torch.autograd.backward(blendshapes.blend_shapes(t, c, shapes), go)

    t2, c2 = (x.detach().clone().requires_grad_(True) for x in (t, c))
    D, reg = torch.from_numpy(kw['directions']).to(gpu), torch.from_numpy(kw['regressor']).to(gpu)
    vertices2 = t2 + (c2 @ D.reshape(217, -1)).reshape(-1, 6890, 3)
    Ks = kw['joint_shapes']
    joints2 = torch.einsum('jv,vc->jc', reg, t2) + (c2[:, :Ks] @ shapes.joint_directions.reshape(Ks, -1)).reshape(-1, 24, 3)
    torch.autograd.backward([vertices2, joints2], go)
    vertices, joints = blendshapes.blend_shapes(t.detach(), c.detach(), shapes)
    for k, a, b in (('vertices', vertices, vertices2), ('joints', joints, joints2), ('d_template', t.grad, t2.grad), ('d_coefficients', c.grad, c2.grad)):
        close(a, b.detach().cpu().numpy(), ref['mass_' + k], (1 + KERNEL) * F32[k], 'torch composition: %s' % k)
        close(a, ref[k], ref['mass_' + k], KERNEL * F32[k], 'smpl: %s' % k)


@pytest.mark.gpu
def test_the_shape_fitting_example_descends(gpu):
    """examples/fit_body_shape_fused.py: blend_shapes -> pose_skeleton -> skin_vertices -> vertex_stage -> rasterise_deferred with
    shade_gbuffer -> loss -> backward, for a few steps on the shape coefficients and the rotations together: the losses are
    finite and the loop ends below where it began."""
    losses = _load_example('fit_body_shape_fused').main(steps=12)
    assert len(losses) == 12 and all(np.isfinite(losses)) and losses[-1] < losses[0]
