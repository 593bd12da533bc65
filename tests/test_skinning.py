"""`dirt_amd.skinning` (dirt_skin.hip) against the restatement of tests/skin_reference.py: linear-blend skinning composed on
the CPU in float64, gradients by torch's autograd.  Every comparison is per element, |gpu - ref64| <= tol * (L1 mass of the
element's terms); an element of zero mass must equal the reference exactly; non-finite values must sit in the same
places.  No element is excluded.

The tolerances are measured, not chosen: the float32 composition (the same function, CPU, float32, torch autograd -- the
gather form users wrote before the kernel) is run on `tolerance_cases()`, the inputs of the tests below, and its worst
|f32 - ref64| / mass per kind of result is F32[kind]; the kernel, which sums a bone's entries in another order, gets 4 x
that (the allowance of tests/test_shade.py and tests/test_geometry.py).  Produced by

    python -m tests.skin_reference
"""
import ctypes
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from tests import skin_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32 = {                           # worst |f32 - ref64| / mass of the float32 composition on tolerance_cases()
    'posed': 1.8e-7,
    'd_vertices': 1.8e-7,
    'd_transforms': 1.5e-7,
    'd_weights': 1.9e-7,
}
KERNEL = 4                        # the kernel's allowance over the float32 composition

# name: (V, K, J, components, scenes of the vertices, scenes of the transforms, every vertex on bone 0).  V: around the
# wave (63, 64, 65), more than one workgroup (257), and `root`: one bone's list of 5000 entries, at least three chunks.
# K: the compiled 4 and the generic path at 1, 5, 8.  J: 1, 2, 24 staged in LDS, 300 above the staging limit of 256.
SHAPES = {
    'v1': (1, 4, 2, 3, None, None, False),
    'v63_k1_j1': (63, 1, 1, 3, None, None, False),
    'v64_k5': (64, 5, 24, 3, None, None, False),
    'v65_k8_c4': (65, 8, 2, 4, None, None, False),
    'v257': (257, 4, 24, 3, None, None, False),
    'root': (5000, 4, 24, 3, None, None, True),
    'j300': (257, 4, 300, 3, None, None, False),
    'j300_k5_c4': (65, 5, 300, 4, None, None, False),
    'b3_shared_rest': (257, 4, 24, 3, None, 3, False),
    'b3_per_scene_k5': (257, 5, 24, 3, 3, 3, False),
    'b3_shared_pose_c4': (257, 4, 24, 4, 3, None, False),
    'b3_shared_rest_k8_j300': (65, 8, 300, 3, None, 3, False),
    'b3_per_scene_j300': (65, 4, 300, 4, 3, 3, False),
    'b3_root_shared_pose': (2200, 4, 24, 3, 3, None, True),
    'b3_root_shared_rest': (2200, 4, 24, 3, None, 3, True),
}
CASES = list(SHAPES)
# Random inputs added after the F32 figures were measured: not part of tolerance_cases(); the float32 composition stays within
# the committed figures on them (test_extra_cases_stay_within_the_committed_figures), so the kernel's bound rests on the same
# ground.  name: the columns of SHAPES (a scene count of 1 is a batch of one: [1, V, C], [1, J, 4, 4]), then the `chunk` the
# SkinWeights is built with (None: the library's own) and the seed.  The bone gradient's second launch gives every column 21
# slots, each summing a bone's rows slot, slot + 21, ...: a bone has one row per chunk, per scene too for shared transforms.
EXTRA_SHAPES = {
    'rows_per_scene': (352, 4, 3, 3, 2, 2, True, 16, 8200),             # bone 0: at least 22 chunks in every scene, per-scene output
    'rows_shared_pose': (65, 4, 2, 3, 8, None, True, 32, 8201),         # at least 3 chunks x 8 scenes: rows decoded as (scene, chunk)
    'rows_shared_rest_k5': (65, 5, 2, 4, None, 8, True, 32, 8202),      # the same chunks through the generic-K sum kernel, per-scene output
    'b40_shared_pose': (64, 4, 3, 3, 40, None, False, None, 8203),      # 40 rows per bone with the library's own chunking
    'j256': (600, 4, 256, 3, None, None, False, None, 8264),            # the staging array exactly full (seed 8204: float32's own d_transforms at 1.25 x F32)
    'j257': (600, 4, 257, 3, None, None, False, None, 8205),            # the first J that is not staged
    'j256_k5_b2': (300, 5, 256, 4, 2, 2, False, None, 8206),            # the same, generic K, restaged per scene in the shared backward
    'j257_k5_b2': (300, 5, 257, 4, 2, 2, False, None, 8207),
    'b1_vertices': (257, 4, 24, 3, 1, None, False, None, 8208),         # a batch of one: batched shapes in and out
    'b1_transforms': (257, 5, 24, 4, None, 1, False, None, 8209),
    'b1_both': (257, 4, 24, 4, 1, 1, False, None, 8210),
}
EXTRA_CASES = list(EXTRA_SHAPES)
EXACT_ROWS = (21, 22, 42, 43, 64)                                       # around one and two turns of the 21 slots, and into the fourth
GRAD_PATTERNS = list(itertools.product((False, True), repeat=3))   # requires_grad of (vertices, transforms, weights)


def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(name):
    """The keyword arguments of skin_reference.compose for one comparison (the GPU runs get the same arrays)."""
    if name in EXTRA_SHAPES:
        V, K, J, C, vb, tb, root, _chunk, seed = EXTRA_SHAPES[name]
    else:
        (V, K, J, C, vb, tb, root), seed = SHAPES[name], 8000 + CASES.index(name)
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1., 1., ((vb,) if vb else ()) + (V, 3))
    if C == 4:
        v = np.concatenate([v, rng.uniform(0.9, 1.1, v.shape[:-1] + (1,))], -1)
    idx, w = R.random_weights(rng, V, K, J, root=root)
    if name.startswith('j25'):
        idx[0, 0], idx[-1, -1] = 0, J - 1      # the first and the last staged block (or the first unstaged bone) are read
    grad = rng.standard_normal(((vb or tb,) if (vb or tb) else ()) + (V, 3)).astype(np.float32)
    return dict(vertices=v.astype(np.float32), bone_indices=idx, bone_weights=w, transforms=R.random_transforms(rng, J, tb), grad=grad)


def smpl_case():
    """An SMPL-sized mesh: 6 890 vertices, 24 bones, four distinct bones per vertex -- as a dense [V, J] matrix"""
    rng = np.random.default_rng(8100)
    V, J = 6890, 24
    dense = np.zeros((V, J), np.float32)
    for i in range(V):
        bones = rng.permutation(J)[:4]
        w = rng.uniform(0.05, 1., 4)
        dense[i, bones] = w / w.sum()
    return dict(vertices=rng.uniform(-1., 1., (V, 3)).astype(np.float32), dense=dense, transforms=R.random_transforms(rng, J),
                grad=rng.standard_normal((V, 3)).astype(np.float32))


def tolerance_cases():
    """The inputs the float32 figures are measured on: every random input of the comparisons below.  The hand-made index
    cases are not part: they are a few exactly representable values."""
    for name in CASES:
        yield case(name)
    from dirt_amd import skinning
    kw = smpl_case()
    skin = skinning.SkinWeights.from_dense(torch.from_numpy(kw.pop('dense')))
    yield dict(kw, bone_indices=skin.bone_indices.numpy(), bone_weights=skin.bone_weights.numpy())


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


def run_fused(kw, dev, requires=(True, True, True), chunk=None):
    """-> (posed, {gradient name: tensor or None}) of skin_vertices on the arrays of `kw`; chunk: that of the SkinWeights"""
    from dirt_amd import skinning
    v = torch.from_numpy(kw['vertices']).to(dev).requires_grad_(requires[0])
    T = torch.from_numpy(kw['transforms']).to(dev).requires_grad_(requires[1])
    w = torch.from_numpy(kw['bone_weights']).to(dev).requires_grad_(requires[2])
    skin = skinning.SkinWeights(torch.from_numpy(kw['bone_indices']).to(dev), torch.from_numpy(kw['bone_weights']).to(dev), int(kw['transforms'].shape[-3]),
                               chunk=chunk)
    posed = skinning.skin_vertices(v, skin, T, weights=w)
    if posed.requires_grad:
        posed.backward(torch.from_numpy(kw['grad']).to(dev))
    return posed, {'d_vertices': v.grad, 'd_transforms': T.grad, 'd_weights': w.grad}


def compare(kw, dev, what, requires=(True, True, True), factor=KERNEL, chunk=None):
    ref = R.compose(**kw)
    posed, grads = run_fused(kw, dev, requires=requires, chunk=chunk)
    assert posed.shape == ref['posed'].shape and posed.requires_grad == any(requires)
    close(posed, ref['posed'], ref['mass_posed'], factor * F32['posed'], '%s posed' % what)
    for k, on in zip(R.GRAD_KINDS, requires):
        if not on:
            assert grads[k] is None, '%s: %s has a gradient nobody asked for' % (what, k)
        else:
            assert grads[k].shape == ref[k].shape
            close(grads[k], ref[k], ref['mass_' + k], factor * F32[k], '%s %s' % (what, k))
    return posed, grads, ref


def brute_force_index(bone_indices, num_bones, chunk):
    idx = np.asarray(bone_indices)
    lists = [[] for _ in range(num_bones)]
    for position, bone in enumerate(idx.reshape(-1)):
        lists[int(bone)].append(position)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    table, chunk_offsets = [], [0]
    for bone, entries in enumerate(lists):
        for begin in range(0, len(entries), chunk):
            table.append((bone, offsets[bone] + begin, offsets[bone] + min(begin + chunk, len(entries))))
        chunk_offsets.append(len(table))
    return (offsets, np.asarray([e for x in lists for e in x], np.int32), np.asarray(table, np.int32).reshape(-1, 3),
            np.asarray(chunk_offsets, np.int32))


def hand_made_case():
    """Small integers and binary fractions: every product and sum of the composition is exact in float32.  Bone 2 has no
    entry; vertex 0 and vertex 3 name one bone in both slots; vertices 1 and 2 carry a zero-weight padding slot (on bones 3
    and 3: bone 3 has padding entries only); no row of weights sums to one; the transforms are not affine (a last column
    that is not (0, 0, 0, 1), a last row that scales w) and the vertices carry their own w."""
    rng = np.random.default_rng(9101)
    idx = np.asarray([[0, 0], [1, 3], [3, 1], [1, 1], [0, 1]], np.int32)
    w = np.asarray([[0.5, 0.25], [1., 0.], [0., 2.], [0.75, 0.75], [1.5, 0.5]], np.float32)
    v = np.concatenate([rng.integers(-3, 4, (5, 3)), rng.integers(1, 3, (5, 1))], 1).astype(np.float32)
    T = rng.integers(-2, 3, (4, 4, 4)).astype(np.float32)
    return dict(vertices=v, bone_indices=idx, bone_weights=w, transforms=T, grad=rng.integers(-2, 3, (5, 3)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- CPU tests

def test_committed_tolerances_are_not_below_the_float32_composition():
    """The F32 constants restate what `python -m tests.skin_reference` measures; the kernel's bound may not rest on a figure
    smaller than the float32 composition's own error."""
    measured = R.measure_f32(tolerance_cases())
    print(measured)
    for k, v in measured.items():
        assert F32[k] >= v, '%s: committed %.3e, measured %.3e' % (k, F32[k], v)
        assert F32[k] <= 1.25 * v + 1e-12, '%s: committed %.3e is more than the measured %.3e (rounded up)' % (k, F32[k], v)


def test_the_restatement_is_the_dense_composition_and_within_its_masses():
    """The gather form of tests/skin_reference.py equals the dense form ([V, J] @ [J, 16]) in float64, and every float64
    result is within its own mass; the cases hold what their names say."""
    from dirt_amd import skinning
    for name in ('v65_k8_c4', 'b3_per_scene_k5', 'b3_shared_rest', 'b3_shared_pose_c4'):
        kw = case(name)
        r = R.compose(**kw)
        for k in R.VALUE_KINDS + R.GRAD_KINDS:
            assert bool((r[k].abs() <= r['mass_' + k] * (1 + 1e-9) + 1e-300).all()), (name, k)
        skin = skinning.SkinWeights(torch.from_numpy(kw['bone_indices']), torch.from_numpy(kw['bone_weights']), kw['transforms'].shape[-3])
        v, T = torch.from_numpy(kw['vertices']).double(), torch.from_numpy(kw['transforms']).double()
        v4 = v if v.shape[-1] == 4 else torch.cat([v, torch.ones_like(v[..., :1])], -1)
        M = (skin.dense(skin.bone_weights.double()) @ T.reshape(T.shape[:-2] + (16,))).reshape(T.shape[:-3] + (-1, 4, 4))
        assert torch.allclose((v4[..., None, :] @ M)[..., 0, :3], r['posed'], rtol=1e-12, atol=1e-12), name
        assert bool((r['d_transforms'][..., 3] == 0).all()) and bool((r['mass_d_transforms'][..., 3] == 0).all())
    from dirt_amd import _lib
    root = skinning.SkinWeights(torch.from_numpy(case('root')['bone_indices']), torch.from_numpy(case('root')['bone_weights']), 24)
    assert int(root.chunk_offsets[1]) >= 3 and int(root.offsets[1]) >= 5000     # every vertex on bone 0, over at least three chunks
    assert SHAPES['j300'][2] > _lib.SKIN_LDS_BONES
    smpl = smpl_case()
    assert ((smpl['dense'] != 0).sum(1) == 4).all()


def test_extra_cases_stay_within_the_committed_figures():
    """EXTRA_CASES are not part of what F32 was measured on; the float32 composition's own error on them is within the
    committed figures all the same, so 4 x F32 allows the kernel there what it allows it on tolerance_cases()."""
    measured = R.measure_f32(case(name) for name in EXTRA_CASES)
    print(measured)
    for k, v in measured.items():
        assert v <= F32[k], '%s: committed %.3e, measured on the extra cases %.3e' % (k, F32[k], v)


def bone_rows(kw, chunk):
    """rows the bone gradient's second launch adds per bone and output scene: the bone's chunks, times the scenes for shared transforms"""
    from dirt_amd import skinning
    skin = skinning.SkinWeights(torch.from_numpy(kw['bone_indices']), torch.from_numpy(kw['bone_weights']), kw['transforms'].shape[-3], chunk=chunk)
    scenes = kw['vertices'].shape[0] if kw['vertices'].ndim == 3 and kw['transforms'].ndim == 3 else 1
    return np.diff(skin.chunk_offsets.numpy()) * scenes


def exact_rows_case(n, scenes=None):
    """K = 1, two bones, 70 vertices, the first n on bone 0; weights of 0.5, 1 and 2, small integers everywhere else (vertices
    with their own w, transforms that are not affine): every product and sum of the composition is exact in float32 in any
    order.  Built with chunk=1, bone 0 has n rows of one entry each -- 3 n with `scenes`=3 of per-scene vertices under shared
    transforms."""
    rng = np.random.default_rng(9200 + n)
    V = 70
    idx = (np.arange(V) >= n).astype(np.int32)[:, None]
    w = rng.choice(np.asarray([0.5, 1., 2.], np.float32), (V, 1))
    lead = (scenes,) if scenes else ()
    v = np.concatenate([rng.integers(-3, 4, lead + (V, 3)), rng.integers(1, 3, lead + (V, 1))], -1).astype(np.float32)
    return dict(vertices=v, bone_indices=idx, bone_weights=w, transforms=rng.integers(-2, 3, (2, 4, 4)).astype(np.float32),
                grad=rng.integers(-2, 3, lead + (V, 3)).astype(np.float32))


def test_the_extra_cases_hold_what_their_names_say():
    """The row counts that take the reduce kernel's slots into a second turn, the slot count itself, and the staging limit the
    J cases straddle: a change of SK_SLOTS, CHUNK or DIRT_SKIN_LDS_BONES fails here instead of leaving the cases short of
    the paths they are for."""
    from dirt_amd import _lib, skinning
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_skin.hip')).read()
    assert 'constexpr int SK_SLOTS = 21;' in source
    slots = 21
    rows = {name: bone_rows(case(name), EXTRA_SHAPES[name][7]) for name in EXTRA_CASES}
    for name in ('rows_per_scene', 'rows_shared_pose', 'b40_shared_pose'):
        assert rows[name].max() > slots, (name, rows[name])
    assert rows['rows_per_scene'][0] >= 22 and case('rows_per_scene')['transforms'].shape == (2, 3, 4, 4)
    assert rows['rows_shared_pose'][0] >= 3 * 8 and rows['rows_shared_pose'][0] % 8 == 0 and case('rows_shared_pose')['transforms'].ndim == 3
    assert rows['b40_shared_pose'].tolist() == [40, 40, 40] and EXTRA_SHAPES['b40_shared_pose'][7] is None and skinning.CHUNK >= 4 * 64
    # (per-scene transforms: the rows of an output are one scene's chunks; this case is for the scene index of the generic-K FIRST launch)
    kw = case('rows_shared_rest_k5')
    assert rows['rows_shared_rest_k5'][0] >= 3 and kw['transforms'].shape == (8, 2, 4, 4) and kw['bone_indices'].shape[1] == 5
    for n in EXACT_ROWS:
        assert bone_rows(exact_rows_case(n), 1).tolist() == [n, 70 - n] and bone_rows(exact_rows_case(n, 3), 1).tolist() == [3 * n, 3 * (70 - n)]
        # every value is a multiple of 0.5 below 2^23: float32 holds each partial sum exactly, in whatever order they are added
        for scenes in (None, 3):
            kw = exact_rows_case(n, scenes)
            ref = R.compose(**kw)
            assert 2 ** 24 > 2 * max(float(ref['mass_' + k].max()) for k in R.VALUE_KINDS + R.GRAD_KINDS)
            assert all(bool((2 * ref[k] == (2 * ref[k]).round()).all()) for k in R.VALUE_KINDS + R.GRAD_KINDS)
            # the test bites: a reduce that took only the first turn of its slots (rows 0 .. 20 of bone 0, scene by scene then
            # chunk by chunk) would write another d T[0] -- the rows it left out do not cancel
            v4, g = torch.from_numpy(kw['vertices']).double().reshape(-1, 70, 4), torch.from_numpy(kw['grad']).double().reshape(-1, 70, 3)
            per_row = (torch.from_numpy(kw['bone_weights']).double()[None, :n, :, None] * v4[:, :n, :, None] * g[:, :n, None, :]).reshape(-1, 4, 3)
            assert torch.equal(per_row.sum(0), ref['d_transforms'][0, :, :3])
            if len(per_row) > slots:
                assert not torch.equal(per_row[:slots].sum(0), per_row.sum(0)), (n, scenes)
    assert _lib.SKIN_LDS_BONES == 256
    for name in EXTRA_CASES:
        if name.startswith('j25'):
            kw = case(name)
            J = kw['transforms'].shape[-3]
            assert J == (256 if name.startswith('j256') else 257) and kw['bone_indices'][0, 0] == 0 and kw['bone_indices'][-1, -1] == J - 1
    assert case('j256')['transforms'].shape[-3] == _lib.SKIN_LDS_BONES == case('j257')['transforms'].shape[-3] - 1
    for name, vs, ts in (('b1_vertices', (1, 257, 3), (24, 4, 4)), ('b1_transforms', (257, 4), (1, 24, 4, 4)), ('b1_both', (1, 257, 4), (1, 24, 4, 4))):
        kw = case(name)
        assert kw['vertices'].shape == vs and kw['transforms'].shape == ts and kw['grad'].shape == (1, 257, 3)


def test_skin_weights_is_the_brute_force_inversion():
    from dirt_amd import skinning
    rng = np.random.default_rng(12)
    tables = [(np.asarray([[0, 0], [1, 3], [3, 1], [1, 1], [0, 1]], np.int32), 4, 2), (np.asarray([[2], [2], [0]], np.int64), 3, 1),
              (rng.integers(0, 7, (50, 3)).astype(np.int32), 9, 4), (rng.integers(0, 2, (300, 8)).astype(np.int64), 2, 256),
              (np.zeros((0, 4), np.int32), 5, 1024), (np.zeros((0, 1), np.int32), 0, 1024), (case('root')['bone_indices'], 24, None)]
    for idx, J, chunk in tables:
        w = torch.from_numpy(rng.uniform(0., 1., idx.shape).astype(np.float32))
        s = skinning.SkinWeights(torch.from_numpy(idx), w, J, chunk=chunk)
        offsets, entries, table, chunk_offsets = brute_force_index(idx, J, chunk or skinning.CHUNK)
        for t in (s.bone_indices, s.entries, s.offsets, s.chunk_table, s.chunk_offsets):
            assert t.dtype == torch.int32 and t.is_contiguous()
        assert np.array_equal(s.entries.numpy(), entries) and np.array_equal(s.offsets.numpy(), offsets)
        assert np.array_equal(s.chunk_table.numpy(), table) and np.array_equal(s.chunk_offsets.numpy(), chunk_offsets)
        assert s.chunk_table.shape == (s.num_chunks, 3) and s.entries.shape == (idx.size,)
        assert (s.num_vertices, s.num_bones, s.influences) == (idx.shape[0], J, idx.shape[1])
        assert np.array_equal(s.bone_indices.numpy(), idx) and torch.equal(s.bone_weights, w)
    s = skinning.SkinWeights(torch.tensor([[0, 0], [1, 3], [3, 1]]), torch.ones(3, 2), 4, chunk=2)
    assert s.entries.tolist() == [0, 1, 2, 5, 3, 4] and s.offsets.tolist() == [0, 2, 4, 4, 6]
    assert s.chunk_table.tolist() == [[0, 0, 2], [1, 2, 4], [3, 4, 6]] and s.chunk_offsets.tolist() == [0, 1, 2, 2, 3]
    assert skinning.SkinWeights(torch.zeros(5, 1, dtype=torch.int32), torch.ones(5, 1), 1, chunk=2).chunk_table.tolist() == [[0, 0, 2], [0, 2, 4], [0, 4, 5]]
    moved = s.to('cpu')
    assert isinstance(moved, skinning.SkinWeights) and moved.device.type == 'cpu' and torch.equal(moved.chunk_table, s.chunk_table)
    assert (moved.num_vertices, moved.num_bones, moved.influences, moved.num_chunks) == (3, 4, 2, 3)
    assert s.dense().tolist() == [[2., 0, 0, 0], [0, 1, 0, 1], [0, 1, 0, 1]]   # two slots on one bone add up


def test_from_dense_round_trips():
    from dirt_amd import skinning
    rng = np.random.default_rng(13)
    dense = np.zeros((40, 9), np.float32)
    for i in range(40):
        n = int(rng.integers(0, 6))   # rows of zero to five non-zero weights
        dense[i, rng.permutation(9)[:n]] = rng.uniform(0.1, 1., n)
    dense[7:9] = 0.
    dense[8, [0, 2, 4, 6, 8]] = [1., 2., 3., 4., -1.]
    s = skinning.SkinWeights.from_dense(torch.from_numpy(dense))
    assert s.influences == 5 and s.num_bones == 9 and s.num_vertices == 40
    assert torch.equal(s.dense(), torch.from_numpy(dense))
    assert s.bone_indices[8].tolist() == [0, 2, 4, 6, 8] and s.bone_weights[8].tolist() == [1., 2., 3., 4., -1.]
    assert s.bone_indices[7].tolist() == [0] * 5 and s.bone_weights[7].tolist() == [0.] * 5     # padding: bone 0, weight 0
    pad = s.bone_weights == 0
    assert bool((s.bone_indices[pad] == 0).all())
    kw = smpl_case()
    smpl = skinning.SkinWeights.from_dense(torch.from_numpy(kw['dense']))
    assert smpl.influences == 4 and torch.equal(smpl.dense(), torch.from_numpy(kw['dense']))
    assert skinning.SkinWeights.from_dense(torch.zeros(3, 2)).influences == 1
    with pytest.raises(ValueError, match='9 non-zero weights, at most 8'):
        skinning.SkinWeights.from_dense(torch.ones(2, 9))
    for bad in (torch.ones(2, 9, dtype=torch.float64), torch.ones(4), np.ones((2, 2), np.float32), torch.ones(3, 0)):
        with pytest.raises(ValueError, match='from_dense'):
            skinning.SkinWeights.from_dense(bad)


def test_refuses_bad_arguments():
    from dirt_amd import skinning
    S = skinning.SkinWeights
    idx = torch.tensor([[0, 1], [1, 2], [2, 0]], dtype=torch.int32)
    w = torch.full((3, 2), 0.5)
    for a, b, J, match in ((idx.reshape(-1), w.reshape(-1), 3, 'bone_indices .V, K.'), (idx.float(), w, 3, 'int32 or int64'),
                           (torch.zeros(3, 9, dtype=torch.int32), torch.zeros(3, 9), 3, '1 <= K <= 8'), (torch.zeros(3, 0, dtype=torch.int32), torch.zeros(3, 0), 3, '1 <= K <= 8'),
                           (idx, w[:2], 3, 'shaped like bone_indices'), (idx, w.double(), 3, 'float32 bone_weights'), (idx, w.numpy(), 3, 'shaped like'),
                           (idx.numpy(), w, 3, 'bone_indices .V, K.'), (idx, w, 2, 'outside'), (idx - 1, w, 3, 'outside'), (idx, w, -1, 'num_bones'),
                           (idx, w, 3., 'num_bones'), (idx, w, 1 << 17, 'at most'), (idx, w.to('meta'), 3, 'bone_weights is on meta')):
        with pytest.raises(ValueError, match=match):
            S(a, b, J)
    with pytest.raises(ValueError, match='chunk >= 1'):
        S(idx, w, 3, chunk=0)
    many = (1 << 27) + 1        # V K past int32's reach, refused by the shape alone (expanded views: no memory behind them)
    with pytest.raises(ValueError, match='at most %d entries' % (1 << 30)):
        S(torch.zeros(1, 8, dtype=torch.int32).expand(many, 8), torch.zeros(1, 8).expand(many, 8), 3)
    skin = S(idx, w, 3)
    v, T = torch.zeros(3, 3), torch.eye(4).repeat(3, 1, 1)
    with pytest.raises(RuntimeError, match='runs on an MI355X only; there is no CPU fallback'):
        skinning.skin_vertices(v, skin, T)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        skinning.skin_vertices(v[None], skin, T[None], weights=w)
    for args, kw, match in (((torch.zeros(3, 2), skin, T), {}, 'expects vertices'), ((torch.zeros(3), skin, T), {}, 'expects vertices'),
                            ((torch.zeros(1, 1, 3, 3), skin, T), {}, 'expects vertices'), ((v.double(), skin, T), {}, 'float32 vertices'),
                            ((v.numpy(), skin, T), {}, 'expects vertices'), ((v, (idx, w), T), {}, 'SkinWeights'),
                            ((torch.zeros(4, 3), skin, T), {}, 'built for 3'), ((v, skin, T[:2]), {}, 'bone_transforms must have shape'),
                            ((v, skin, torch.zeros(3, 3, 4)), {}, 'bone_transforms must have shape'), ((v, skin, T[0]), {}, 'bone_transforms must have shape'),
                            ((v, skin, T.numpy()), {}, 'bone_transforms must have shape'), ((v, skin, T.double()), {}, 'bone_transforms must be float32'),
                            ((v, skin, T.to('meta')), {}, 'bone_transforms is on meta'), ((v.to('meta'), skin, T), {}, 'SkinWeights is on cpu'),
                            ((torch.zeros(2, 3, 3), skin, torch.zeros(4, 3, 4, 4)), {}, '2 scenes of vertices, 4 of bone_transforms'),
                            ((v, skin, T), dict(weights=torch.zeros(3, 3)), 'weights must have shape'), ((v, skin, T), dict(weights=w.numpy()), 'weights must have shape'),
                            ((v, skin, T), dict(weights=w.double()), 'weights must be float32'), ((v, skin, T), dict(weights=w.to('meta')), 'weights is on meta')):
        with pytest.raises(ValueError, match=match):
            skinning.skin_vertices(*args, **kw)
    assert skinning._check_arguments(torch.zeros(3, 4), skin, T, None) == (1, 3, 4, False)
    assert skinning._check_arguments(torch.zeros(3, 4), skin, T[None].repeat(5, 1, 1, 1), w) == (5, 3, 4, True)
    assert skinning._check_arguments(torch.zeros(2, 3, 3), skin, T, None) == (2, 3, 3, True)


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    for s in ('dirt_skin_scratch_bytes', 'dirt_skin_forward', 'dirt_skin_backward'):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    assert 'samples/deferred.py:40-41' in header and '#define DIRT_SKIN_MAX_INFLUENCES 8' in header
    assert '#define DIRT_SKIN_MAX_BONES %d' % _lib.SKIN_MAX_BONES in header and '#define DIRT_SKIN_LDS_BONES %d' % _lib.SKIN_LDS_BONES in header
    assert _lib.SKIN_MAX_INFLUENCES == 8 and '#define DIRT_ABI_VERSION 4' in header
    assert _lib.SKIN_MAX_ENTRIES == 1 << 30 and '#define DIRT_SKIN_MAX_ENTRIES (1 << 30)' in header   # V K stays inside int32
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    good = dict(v=one, c=3, vs=1, i=one, w=one, t=one, ts=2, B=2, V=64, K=4, J=24, flags=0)

    def fwd(posed=one, **over):
        a = dict(good, **over)
        return lib.dirt_skin_forward(a['v'], a['c'], a['vs'], a['i'], a['w'], a['t'], a['ts'], posed, a['B'], a['V'], a['K'], a['J'], a['flags'], None)

    def bwd(e=one, ct=one, co=one, g=one, gv=one, gt=one, gw=one, scratch=one, nbytes=1 << 20, chunks=30, **over):
        a = dict(good, **over)
        return lib.dirt_skin_backward(a['v'], a['c'], a['vs'], a['i'], a['w'], a['t'], a['ts'], e, ct, co, g, gv, gt, gw, scratch, nbytes, a['B'], a['V'],
                                      a['K'], a['J'], chunks, a['flags'], None)

    bad = [dict(v=None), dict(i=None), dict(w=None), dict(t=None), dict(c=2), dict(c=5), dict(K=0), dict(K=9), dict(K=-1), dict(J=(1 << 16) + 1),
           dict(J=0), dict(J=-1), dict(B=-1), dict(V=-1), dict(B=70000), dict(V=(1 << 28) + 1), dict(V=(1 << 27) + 1, K=8), dict(V=1 << 28, K=5), dict(vs=0), dict(vs=3), dict(ts=0), dict(ts=5),
           dict(flags=1), dict(flags=1 << 31)]
    for over in bad:
        assert fwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_skin_forward'), over
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_skin_backward'), over
    for over in (dict(g=None), dict(e=None), dict(ct=None), dict(co=None), dict(chunks=0), dict(chunks=-1), dict(chunks=1 << 31), dict(scratch=None),
                 dict(nbytes=8), dict(nbytes=4 * 12 * 2 * 30 - 1), dict(scratch=ctypes.c_void_p(18))):
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_skin_backward'), over
    with pytest.raises(ValueError, match='dirt_skin_backward.*dirt_skin_scratch_bytes'):
        _lib.check(bwd(nbytes=8))
    # no scenes or no vertices: a success that launches nothing, whatever the pointers; nothing wanted likewise
    nothing = dict(v=None, i=None, w=None, t=None)
    assert fwd(posed=None, B=0, vs=1, ts=1, **nothing) == 0 and fwd(V=0, J=0, **nothing) == 0 and fwd(posed=None) == 0
    assert bwd(e=None, ct=None, co=None, g=None, gv=None, gt=None, gw=None, scratch=None, nbytes=0, chunks=0, V=0, **nothing) == 0
    assert bwd(gv=None, gt=None, gw=None, scratch=None, nbytes=0, g=None) == 0
    assert lib.dirt_last_error() == b''
    # scratch: one row of twelve floats per scene and chunk
    assert lib.dirt_skin_scratch_bytes(1, 27) == 4 * 12 * 27 and lib.dirt_skin_scratch_bytes(32, 50) == 4 * 12 * 32 * 50
    assert lib.dirt_skin_scratch_bytes(0, 5) == 0 and lib.dirt_skin_scratch_bytes(5, 0) == 0
    assert lib.dirt_skin_scratch_bytes(-1, 5) == 0 and lib.dirt_skin_scratch_bytes(5, -1) == 0
    assert lib.dirt_skin_scratch_bytes(65536, 5) == 0 and lib.dirt_skin_scratch_bytes(1, 1 << 31) == 0


def test_the_module_is_exported_under_both_package_names():
    import dirt
    import dirt_amd
    import dirt.skinning
    assert dirt.skinning is dirt_amd.skinning and dirt_amd.skin_vertices is dirt_amd.skinning.skin_vertices
    assert dirt_amd.SkinWeights is dirt_amd.skinning.SkinWeights
    from dirt_amd import build
    assert 'dirt_skin.hip' in build.SOURCES
    res = build.kernel_resources()
    skin = {k: v for k, v in res.items() if 'skin_' in k}
    assert len(skin) == 15 and all(v['scratch'] == 0 for v in skin.values()), skin
    assert not any(s in k for k in skin for s in ('geometry_', 'shade_', 'texture_', 'mip_'))
    assert all(v['lds'] <= 12288 for v in skin.values())     # the staging budget: 256 bones x 12 floats
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_skin.hip')).read()
    assert 'atomicAdd' not in source and 'atomic_' not in source


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_values_and_gradients_against_the_restatement(gpu, name):
    compare(case(name), gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['b3_shared_rest', 'b3_per_scene_k5'])
@pytest.mark.parametrize('requires', GRAD_PATTERNS, ids=[''.join(n for n, on in zip('vtw', r) if on) or 'none' for r in GRAD_PATTERNS])
def test_every_pattern_of_requires_grad(gpu, name, requires):
    compare(case(name), gpu, '%s requires_grad=%s' % (name, requires), requires=requires)


@pytest.mark.gpu
def test_hand_made_index_cases_follow_the_composition(gpu):
    """A bone nobody names, a vertex naming one bone twice, zero-weight padding, weights that do not sum to one, transforms
    that are not affine: every value is exact in float32, so the kernels equal the float64 composition to the bit."""
    kw = hand_made_case()
    posed, grads, ref = compare(kw, gpu, 'hand-made', factor=0.)
    dT, dw = grads['d_transforms'].cpu(), grads['d_weights'].cpu()
    assert torch.equal(dT[2], torch.zeros(4, 4))                        # a bone without entries: zero, written
    assert torch.equal(dT[3], torch.zeros(4, 4))                        # padding entries only: zero contribution
    assert bool((dT[..., 3] == 0).all()) and bool(dT[0].abs().sum() > 0) and bool(dT[1].abs().sum() > 0)
    v4, T, g = (torch.from_numpy(kw[k]) for k in ('vertices', 'transforms', 'grad'))
    for vertex, slot in ((1, 1), (2, 0)):                               # the padding slots: the composition's value, not zero
        want = float(((v4[vertex] @ T[kw['bone_indices'][vertex, slot]])[:3] * g[vertex]).sum())
        assert float(dw[vertex, slot]) == want
    assert bool(dw[1, 1] != 0) and bool(dw[2, 0] != 0)
    assert torch.equal(dw[0, 0], dw[0, 1]) and torch.equal(dw[3, 0], dw[3, 1])    # one bone in both slots


@pytest.mark.gpu
@pytest.mark.parametrize('name', EXTRA_CASES)
def test_extra_cases_against_the_restatement(gpu, name):
    """More rows per bone than the reduce kernel has slots (per scene, over the scenes of a shared pose, with the library's own
    chunking), J at and one past the LDS staging limit, and a batch of one on either operand or both."""
    kw = case(name)
    posed, grads, _ = compare(kw, gpu, name, chunk=EXTRA_SHAPES[name][7])
    if name.startswith('b1'):
        assert posed.shape == (1, 257, 3)
        for k, operand in zip(R.GRAD_KINDS, ('vertices', 'transforms', 'bone_weights')):
            assert grads[k].shape == kw[operand].shape, k


@pytest.mark.gpu
@pytest.mark.parametrize('n', EXACT_ROWS)
def test_more_rows_than_slots_exactly(gpu, n):
    """exact_rows_case: bone 0 has n rows (3 n over three scenes of a shared pose) of one entry each, and every sum is exact in
    float32 in any order, so the kernels equal the float64 composition to the bit: a row left out or added twice cannot hide
    under a tolerance."""
    compare(exact_rows_case(n), gpu, '%d rows' % n, factor=0., chunk=1)
    compare(exact_rows_case(n, 3), gpu, '3 x %d rows, shared transforms' % n, factor=0., chunk=1)


def _presented(array, how, dev, transposed=False):
    """The values of `array` on the device as a plain tensor ('plain'), as a contiguous view that starts one float into its
    buffer ('misaligned': 4 mod 16 bytes) or as a non-contiguous view ('strided': the leading columns of a wider buffer; with
    `transposed`, for matrices, the transpose of a tensor that holds the transposed values)"""
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
        buf = torch.full(t.shape[:-1] + (t.shape[-1] + 3,), 7., device=dev)
        buf[..., :t.shape[-1]] = t
        view = buf[..., :t.shape[-1]]
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _run_presented(kw, dev, how, grad):
    """skin_vertices on the arrays of `kw` presented as `how`; grad: an array presented the same way, or 'expanded': the
    stride-0 ones of posed.sum().backward().  -> (posed, leaves)"""
    from dirt_amd import skinning
    leaves = [_presented(kw[k], how, dev, transposed=k == 'transforms').detach().requires_grad_(True) for k in ('vertices', 'transforms', 'bone_weights')]
    skin = skinning.SkinWeights(torch.from_numpy(kw['bone_indices']).to(dev), torch.from_numpy(kw['bone_weights']).to(dev), int(kw['transforms'].shape[-3]))
    posed = skinning.skin_vertices(leaves[0], skin, leaves[1], weights=leaves[2])
    if isinstance(grad, str):
        posed.sum().backward()
    else:
        posed.backward(_presented(grad, how, dev))
    return posed, leaves


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['v257', 'b3_per_scene_k5'])
def test_misaligned_and_non_contiguous_operands(gpu, name):
    """The same values as contiguous views 4 bytes past a 16-byte boundary (the kernels' 12- and 16-byte accesses to rows that
    are only 4-byte aligned, the K = 4 path's 16-byte load of `weights` among them) and as non-contiguous views (the
    wrapper's .contiguous() branches), the incoming gradient likewise -- a strided [.., :3] view is what the rasteriser's
    state hands back, an expanded one what .sum() does: the kernels see the same numbers in the same order, so the output
    and every gradient equal the plain run's to the bit, and every leaf's .grad has the leaf's shape."""
    kw = case(name)
    plain, plain_leaves = _run_presented(kw, gpu, 'plain', kw['grad'])
    assert all(bool(l.grad.abs().max() > 0) for l in plain_leaves)
    for how in ('misaligned', 'strided'):
        posed, leaves = _run_presented(kw, gpu, how, kw['grad'])
        assert torch.equal(plain, posed), how
        for k, a, b in zip(R.GRAD_KINDS, plain_leaves, leaves):
            assert b.grad.shape == b.shape and torch.equal(a.grad, b.grad), (how, k)
    _, want = _run_presented(kw, gpu, 'plain', np.ones(plain.shape, np.float32))
    _, got = _run_presented(kw, gpu, 'plain', 'expanded')
    for k, a, b in zip(R.GRAD_KINDS, want, got):
        assert b.grad.shape == b.shape and torch.equal(a.grad, b.grad) and bool(a.grad.abs().max() > 0), ('expanded', k)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_backward_is_reentrant(gpu):
    from dirt_amd import skinning
    for name in ('root', 'b3_root_shared_pose', 'b3_root_shared_rest', 'b3_per_scene_k5'):
        kw = case(name)
        (o1, g1), (o2, g2) = run_fused(kw, gpu), run_fused(kw, gpu)
        assert torch.equal(o1, o2), name
        for k in R.GRAD_KINDS:
            assert torch.equal(g1[k], g2[k]), (name, k)     # bit for bit: fixed-order sums, no atomics
    # backward twice over one forward (retain_graph=True)
    v, T, w = (torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('vertices', 'transforms', 'bone_weights'))
    skin = skinning.SkinWeights(torch.from_numpy(kw['bone_indices']).to(gpu), w.detach(), 24)
    posed = skinning.skin_vertices(v, skin, T, weights=w)
    go = torch.from_numpy(kw['grad']).to(gpu)
    a = torch.autograd.grad(posed, [v, T, w], go, retain_graph=True)
    b = torch.autograd.grad(posed, [v, T, w], go, retain_graph=True)
    for x, y, k in zip(a, b, R.GRAD_KINDS):
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr(), k
        assert torch.equal(x, g1[k]), k


@pytest.mark.gpu
def test_a_captured_step_replays_to_the_bits_of_eager(gpu):
    """skin_vertices makes no host synchronisation: a step (stage, loss, gradients) is captured with torch.cuda.graph and its
    replay, on new transform values written in place, returns the loss and gradients of the eager step to the bit."""
    from dirt_amd import skinning
    kw = case('b3_root_shared_rest')
    v, T, w = (torch.from_numpy(kw[k]).to(gpu) for k in ('vertices', 'transforms', 'bone_weights'))
    skin = skinning.SkinWeights(torch.from_numpy(kw['bone_indices']).to(gpu), w, 24)
    target = torch.from_numpy(kw['grad']).to(gpu)

    def step():
        leaves = [t.detach().requires_grad_(True) for t in (v, T, w)]
        posed = skinning.skin_vertices(leaves[0], skin, leaves[1], weights=leaves[2])
        loss = ((posed - target) ** 2).mean() + (posed ** 2).sum() * 1e-3
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
        T += 0.001 * torch.from_numpy(R.random_transforms(np.random.default_rng(5), 24, 3)).to(gpu)
    graph.replay()
    loss_e, grads_e = step()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for a, b in zip(grads_g, grads_e):
        assert torch.equal(a, b) and bool(a.abs().max() > 0)


@pytest.mark.gpu
def test_the_dense_form_agrees(gpu):
    """An SMPL-sized mesh with `from_dense` weights against the dense torch composition on the GPU ([V, J] @ [J, 16], the
    other form users write): both are float32 evaluations of one composition -- torch's within F32 of the float64 one, the
    kernel within 4 x that -- so they are within 5 x of each other, by the mass of the terms."""
    from dirt_amd import skinning
    kw = smpl_case()
    dense = torch.from_numpy(kw['dense']).to(gpu)
    skin = skinning.SkinWeights.from_dense(dense)
    ref = R.compose(kw['vertices'], skin.bone_indices.cpu().numpy(), skin.bone_weights.cpu().numpy(), kw['transforms'], grad=kw['grad'])
    go = torch.from_numpy(kw['grad']).to(gpu)

    v, T = (torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('vertices', 'transforms'))
    w = skin.bone_weights.detach().clone().requires_grad_(True)
    posed = skinning.skin_vertices(v, skin, T, weights=w)
    posed.backward(go)

    v2, T2, d2 = (t.detach().clone().requires_grad_(True) for t in (v, T, dense))
    M = (d2 @ T2.reshape(-1, 16)).reshape(-1, 4, 4)
    v4 = torch.cat([v2, torch.ones_like(v2[:, :1])], 1)
    posed2 = (v4[:, None, :] @ M)[:, 0, :3]
    posed2.backward(go)

    close(posed, posed2.detach().cpu().numpy(), ref['mass_posed'], 5 * F32['posed'], 'dense form: posed')
    close(v.grad, v2.grad.cpu().numpy(), ref['mass_d_vertices'], 5 * F32['d_vertices'], 'dense form: d_vertices')
    close(T.grad, T2.grad.cpu().numpy(), ref['mass_d_transforms'], 5 * F32['d_transforms'], 'dense form: d_transforms')
    close(w.grad, torch.gather(d2.grad, 1, skin.bone_indices.long()).cpu().numpy(), ref['mass_d_weights'], 5 * F32['d_weights'], 'dense form: d_weights')


@pytest.mark.gpu
def test_the_pose_fitting_example_descends(gpu):
    """examples/fit_pose_fused.py: skin_vertices -> vertex_stage -> rasterise_deferred with shade_gbuffer -> loss -> backward,
    for a few steps of gradient descent on the bone rotations: the losses are finite and the loop ends below where it began."""
    losses = _load_example('fit_pose_fused').main(steps=12)
    assert len(losses) == 12 and all(np.isfinite(losses)) and losses[-1] < losses[0]
