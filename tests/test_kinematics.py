"""`dirt_amd.kinematics` (dirt_kinematics.hip) against the restatement of tests/kinematics_reference.py: the forward kinematics
of a skeleton composed on the CPU in float64, gradients by torch's autograd.  Every comparison is per element, |gpu - ref64|
<= tol * (L1 mass of the element's terms); an element of zero mass must equal the reference exactly (column 3 of the
transforms is (0, 0, 0, 1) to the bit); non-finite values must sit in the same places.  No element is excluded.

The tolerances are measured, not chosen: the float32 composition (the same function, CPU, float32, torch autograd -- what
users wrote before the kernel) is run on `tolerance_cases()`, the random inputs of the comparisons below, and its worst
|f32 - ref64| / mass per kind of result is F32[kind]; the kernel, which walks a joint's children in another order than
autograd, gets 4 x that (the allowance of tests/test_shade.py, tests/test_geometry.py and tests/test_skinning.py).  Produced by

    python -m tests.kinematics_reference

Angles: random unit axes with angles uniform in [0.3, 3.0]; exact zero vectors at a root, an inner joint and a leaf of the
designated cases; one case with angles of 4 and 7 rad.  Non-zero angles below 0.3 are left out on purpose: the reference
formula's 1 - cos cancels there in float32, and the kernel inherits that by specification (it is matrices.rodrigues operation
for operation), so such inputs would measure the formula, not the kernel.
"""
import ctypes
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from tests import kinematics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32 = {                           # worst |f32 - ref64| / mass of the float32 composition on tolerance_cases()
    'transforms': 1.95e-6,      # (b3_shared_joints, scene 0, joint 1: an angle of 1.5626, 0.008 from pi / 2 under an identity parent,
    'posed_joints': 7.5e-8,     # so R[0][0] = c + (1 - c) k0^2 = 0.0086 is all mass and carries the 1.7e-8 that the angle's own
    'd_rotations': 5.4e-7,      # rounding leaves in cos; every other case is at 0.8e-7 to 5.6e-7)
    'd_joints': 9.6e-7,         # (both gradients: `smpl` through one output only; through both 4.0e-7 and 3.1e-7)
}
KERNEL = 4                        # the kernel's allowance over the float32 composition


def _comb():
    parents = []
    for link in range(20):            # link i is joint 2 i, its leaf joint 2 i + 1
        parents += [2 * (link - 1) if link else -1, 2 * link]
    return parents


SKELETONS = {
    'single': [-1],
    'pair': [-1, 0],
    'smpl': list(R.SMPL_PARENTS),
    'forest': [-1, -1, 0, 1, 1],
    'chain64': list(range(-1, 63)),                   # more levels than a wave has lanes: 64 joints are the one-wave workgroup,
    'chain65': list(range(-1, 64)),                   # 65 the four-wave one
    'star65': [-1] + [0] * 64,                        # a level and a child list of 64 entries
    'star66': [-1] + [0] * 65,                        # and of 65
    'comb': _comb(),                                  # a 20-link chain with a leaf on every link
    'tree256': [-1] + np.random.default_rng(77).integers(0, np.arange(1, 256)).tolist(),   # J = 256, parents[j] uniform in [0, j)
}

# name: (skeleton, scenes of the rotations, scenes of the joints, joints with an exact zero rotation, angles)
SHAPES = {
    'single': ('single', None, None, (), None),
    'pair': ('pair', None, None, (), None),
    'smpl': ('smpl', None, None, (0, 9, 23), None),              # a root, an inner joint, a leaf
    'forest': ('forest', None, None, (1, 2), None),              # the second root, a leaf
    'chain64': ('chain64', None, None, (), None),
    'chain65': ('chain65', None, None, (), None),
    'star65': ('star65', None, None, (), None),
    'star66': ('star66', None, None, (), None),
    'comb': ('comb', None, None, (0, 2, 39), None),
    'tree256': ('tree256', None, None, (), None),
    'smpl_wide': ('smpl', None, None, (), (4., 7.)),             # angles of 4 and 7 rad, alternating
    'b1_rotations': ('smpl', 1, None, (), None),                 # a batch of one: batched shapes in and out
    'b1_joints': ('smpl', None, 1, (), None),
    'b1_both': ('forest', 1, 1, (), None),
    'b3_shared_rotations': ('smpl', None, 3, (), None),
    'b3_shared_joints': ('smpl', 3, None, (0, 9, 23), None),
    'b3_per_scene': ('smpl', 3, 3, (), None),
    'b3_shared_joints_tree256': ('tree256', 3, None, (), None),  # the four-wave workgroup with rows in scratch
    'b3_shared_rotations_chain65': ('chain65', None, 3, (), None),
    'b70_shared_joints': ('smpl', 70, None, (), None),           # more scenes than a wave has lanes, and a reduce over 70 rows
}
CASES = list(SHAPES)


def _comb128():
    parents = []
    for link in range(128):           # as `comb`: link i is joint 2 i, its leaf joint 2 i + 1
        parents += [2 * (link - 1) if link else -1, 2 * link]
    return parents


# Skeletons of the four-wave workgroup that the cases above leave out: every level count, level width and child list at its limit
EXTRA_SKELETONS = {
    'chain256': list(range(-1, 255)),                 # 256 levels: s_lo filled to its last entry, 256 barriers
    'star256': [-1] + [0] * 255,                      # a child list of 255 entries
    'comb128': _comb128(),                            # 256 joints, 129 levels of width 2 (the ends: 1): boundaries at every even lane of waves 1-3
    'ladder3_255': [-1] * 3 + list(range(252)),       # parents[j] = j - 3: 85 levels of width 3, starts on every lane position mod 64
    'roots256': [-1] * 256,                           # one level, no child entries at all
    'forest200': [-1] * 70 + np.random.default_rng(79).integers(0, np.arange(70, 200)).tolist(),   # 70 roots, then parents[j] uniform in [0, j)
}
SKELETONS.update(EXTRA_SKELETONS)
_FOREST_INNER = min(q for q in EXTRA_SKELETONS['forest200'] if q >= 70)       # the first non-root joint that has a child

# Random inputs added after the F32 figures were measured: not part of tolerance_cases(); the float32 composition stays within
# the committed figures on them (test_extra_cases_stay_within_the_committed_figures), so the kernel's bound rests on the same
# ground.  name: (skeleton, scenes of the rotations, scenes of the joints, joints with an exact zero rotation, seed).  The
# reduce kernel sums every 42nd scene per slot: 42 scenes are one turn, 43 one row into the second, 85 / 86 into the third.
EXTRA_SHAPES = {
    'chain256': ('chain256', None, None, (0, 100, 255), 9100),                 # zero rotations at the root, an inner joint, the leaf
    'star256': ('star256', None, None, (), 9100),
    'comb128': ('comb128', None, None, (), 9100),
    'ladder3_255': ('ladder3_255', None, None, (), 9100),
    'roots256': ('roots256', None, None, (), 9101),                            # (seeds 9100, 9102: float32's own transforms at 1.19 and 2.67 x F32)
    'forest200': ('forest200', None, None, (3, _FOREST_INNER, 199), 9102),     # (9100, 9101: transforms at 1.05 and 1.56 x F32)
    'b42_shared_rotations': ('smpl', None, 42, (), 9100),
    'b43_shared_rotations': ('smpl', None, 43, (), 9100),
    'b85_shared_rotations': ('smpl', None, 85, (), 9100),
    'b43_shared_joints': ('smpl', 43, None, (), 9102),                         # (9100, 9101: posed_joints at 1.21 and 1.04 x F32)
    'b86_shared_joints': ('smpl', 86, None, (), 9101),                         # (9100: transforms at 1.09 x F32)
    # the four-wave backward with the reduce in its second turn.  11 008 joints under per-scene rotations: the float32 composition's
    # own posed_joints were at 1.02 to 2.5 x F32 for every seed from 9100 to 9297 (the forest likewise, and its transforms at 2 to 100 x)
    'b43_shared_joints_star256': ('star256', 43, None, (), 9298),
    'b3_shared_joints_chain65': ('chain65', 3, None, (), 9100),                # 191 lanes without a joint, rows in scratch
}
EXTRA_CASES = list(EXTRA_SHAPES)
SAME_BITS = ('chain256', 'star256', 'b85_shared_rotations')
PATTERN_CASES = ('b43_shared_rotations', 'b43_shared_joints')      # the shared operand is the rotations / the joints
# (case, scenes the mutated scene sum stops at): test_the_extra_cases_bite
SCENE_SUMS = (('b43_shared_rotations', 42), ('b85_shared_rotations', 84), ('b43_shared_joints', 42), ('b86_shared_joints', 85),
              ('b43_shared_joints_star256', 42))
GRAD_PATTERNS = list(itertools.product((False, True), repeat=2))   # requires_grad of (rotations, joints)
# (case, the output nobody used): the gradient through the other output alone
ONE_OUTPUT = [(name, unused) for name in ('smpl', 'b3_shared_joints') for unused in ('grad_posed_joints', 'grad_transforms')]


def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_CASE_CACHE = {}


def case(name):
    """The keyword arguments of kinematics_reference.compose for one comparison (the GPU runs get the same arrays)."""
    if name not in _CASE_CACHE:
        if name in EXTRA_SHAPES:
            (skeleton, rb, pb, zeros, seed), wide = EXTRA_SHAPES[name], None
        else:
            (skeleton, rb, pb, zeros, wide), seed = SHAPES[name], 8300 + CASES.index(name)
        parents = SKELETONS[skeleton]
        J = len(parents)
        rng = np.random.default_rng(seed)
        lead_r, lead_p = ((rb,) if rb else ()), ((pb,) if pb else ())
        lead = ((rb or pb,) if (rb or pb) else ())
        axes = rng.standard_normal(lead_r + (J, 3))
        axes /= np.linalg.norm(axes, axis=-1, keepdims=True)
        angles = rng.uniform(0.3, 3.0, lead_r + (J, 1))
        if wide:
            angles = np.broadcast_to(np.where(np.arange(J) % 2 == 0, wide[0], wide[1])[:, None], angles.shape)
        r = (axes * angles).astype(np.float32)
        for j in zeros:
            r[..., j, :] = 0.
        _CASE_CACHE[name] = dict(rotations=r, joints=rng.uniform(-1., 1., lead_p + (J, 3)).astype(np.float32), parents=parents,
                                 grad_transforms=rng.standard_normal(lead + (J, 4, 4)).astype(np.float32),      # column 3 included
                                 grad_posed_joints=rng.standard_normal(lead + (J, 3)).astype(np.float32))
    return dict(_CASE_CACHE[name])


def tolerance_cases():
    """The inputs the float32 figures are measured on: every random input of the comparisons below."""
    for name in CASES:
        yield case(name)
    for name, unused in ONE_OUTPUT:
        yield dict(case(name), **{unused: None})


_REFERENCES = {}


def reference(name):
    """the float64 restatement of a case, computed once and shared by the tests that need it"""
    if name not in _REFERENCES:
        _REFERENCES[name] = R.compose(**case(name))
    return _REFERENCES[name]


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


def run_fused(kw, dev, requires=(True, True)):
    """-> ((transforms, posed_joints), {gradient name: tensor or None}) of pose_skeleton on the arrays of `kw`; an output
    whose incoming gradient is None in `kw` is left out of the backward pass"""
    from dirt_amd import kinematics
    r = torch.from_numpy(kw['rotations']).to(dev).requires_grad_(requires[0])
    p = torch.from_numpy(kw['joints']).to(dev).requires_grad_(requires[1])
    skeleton = kinematics.Skeleton(kw['parents'], device=dev)
    T, q = kinematics.pose_skeleton(r, p, skeleton)
    used = [(out, torch.from_numpy(kw[g]).to(dev)) for out, g in ((T, 'grad_transforms'), (q, 'grad_posed_joints')) if kw.get(g) is not None]
    if T.requires_grad and used:
        torch.autograd.backward([o for o, _ in used], [g for _, g in used])
    return (T, q), {'d_rotations': r.grad, 'd_joints': p.grad}


def compare(kw, dev, what, requires=(True, True), factor=KERNEL, ref=None):
    ref = R.compose(**kw) if ref is None else ref
    (T, q), grads = run_fused(kw, dev, requires=requires)
    assert T.shape == ref['transforms'].shape and q.shape == ref['posed_joints'].shape
    assert T.requires_grad == q.requires_grad == any(requires)
    close(T, ref['transforms'], ref['mass_transforms'], factor * F32['transforms'], '%s transforms' % what)
    close(q, ref['posed_joints'], ref['mass_posed_joints'], factor * F32['posed_joints'], '%s posed_joints' % what)
    for k, operand, on in zip(R.GRAD_KINDS, ('rotations', 'joints'), requires):
        if not on:
            assert grads[k] is None, '%s: %s has a gradient nobody asked for' % (what, k)
        else:
            assert grads[k].shape == kw[operand].shape == ref[k].shape
            close(grads[k], ref[k], ref['mass_' + k], factor * F32[k], '%s %s' % (what, k))
    return (T, q), grads, ref


def brute_force_index(parents):
    J = len(parents)
    depth = []
    for j, q in enumerate(parents):
        depth.append(0 if q < 0 else depth[q] + 1)
    levels = [[j for j in range(J) if depth[j] == d] for d in range(max(depth) + 1 if J else 0)]
    children = [[c for c in range(J) if parents[c] == j] for j in range(J)]
    return ([j for level in levels for j in level], np.concatenate([[0], np.cumsum([len(x) for x in levels])]).astype(np.int64).tolist(),
            [c for x in children for c in x], np.concatenate([[0], np.cumsum([len(x) for x in children])]).astype(np.int64).tolist())


# ---------------------------------------------------------------------------------------------------------------- CPU tests

def test_committed_tolerances_are_not_below_the_float32_composition():
    """The F32 constants restate what `python -m tests.kinematics_reference` measures; the kernel's bound may not rest on a
    figure smaller than the float32 composition's own error (nor on one rounded up by more than a quarter)."""
    measured = R.measure_f32(tolerance_cases())
    print(measured)
    for k, v in measured.items():
        assert F32[k] >= v, '%s: committed %.3e, measured %.3e' % (k, F32[k], v)
        assert F32[k] <= 1.25 * v + 1e-12, '%s: committed %.3e is more than the measured %.3e (rounded up)' % (k, F32[k], v)


def test_the_restatement_is_the_loop_of_compose_calls():
    """The closed form of tests/kinematics_reference.py equals, in float64, the loop users write (rodrigues, two translations
    and up to three compose per joint: examples/fit_pose_fused.py, for a tree) to 1e-13; every float64 result is within its
    own mass; column 3 of the transforms has none; and the cases hold what their names say."""
    for name in ('smpl', 'chain65', 'forest', 'b3_shared_joints'):
        kw, r = case(name), reference(name)
        rd, pd = (torch.from_numpy(kw[k]).double() for k in ('rotations', 'joints'))
        T, q = R.loop(rd, pd, kw['parents'])
        assert float((T - r['transforms']).abs().max()) <= 1e-13 and float((q - r['posed_joints']).abs().max()) <= 1e-13, name
        for k in R.VALUE_KINDS + R.GRAD_KINDS:
            assert r[k].shape == r['mass_' + k].shape
            if k != 'transforms':   # (its column 3 has no mass: below)
                assert bool((r[k].abs() <= r['mass_' + k] * (1 + 1e-9) + 1e-300).all()), (name, k)
        m = r['mass_transforms']
        assert bool((m[..., 3] == 0).all()) and bool((m[..., :3] > 0).all())
        col = r['transforms'][..., 3]
        assert bool((col[..., :3] == 0).all()) and bool((col[..., 3] == 1).all())
        assert bool((r['transforms'][..., :3].abs() <= m[..., :3] * (1 + 1e-9)).all())
    # the gradient of column 3 is ignored
    kw = case('forest')
    other = dict(kw, grad_transforms=kw['grad_transforms'].copy())
    other['grad_transforms'][..., 3] += 5.
    a, b = reference('forest'), R.compose(**other)
    assert torch.equal(a['d_rotations'], b['d_rotations']) and torch.equal(a['d_joints'], b['d_joints'])
    from dirt_amd import kinematics
    for name, levels, widest_level, most_children in (('chain64', 64, 1, 1), ('chain65', 65, 1, 1), ('star65', 2, 64, 64), ('star66', 2, 65, 65),
                                                      ('comb', 21, 2, 2), ('single', 1, 1, 0), ('forest', 2, 3, 2)):
        s = kinematics.Skeleton(SKELETONS[name])
        assert s.num_levels == levels and int(s.level_offsets.diff().max()) == widest_level and int(s.child_offsets.diff().max()) == most_children, name
    tree = SKELETONS['tree256']
    assert len(tree) == 256 and tree[0] == -1 and all(0 <= q < j for j, q in enumerate(tree) if j)
    assert len(SKELETONS['smpl']) == 24 and len(SKELETONS['comb']) == 40
    for name in CASES:
        kw = case(name)
        for j in SHAPES[name][3]:
            assert not kw['rotations'][..., j, :].any()
        angles = np.linalg.norm(kw['rotations'], axis=-1)
        live = angles > 0
        assert (angles[live] >= 0.3 - 1e-6).all() and int((~live).sum()) == len(SHAPES[name][3]) * (SHAPES[name][1] or 1)
    assert sorted(set(np.round(np.linalg.norm(case('smpl_wide')['rotations'], axis=-1), 4).tolist())) == [4., 7.]


def test_extra_cases_stay_within_the_committed_figures():
    """EXTRA_CASES are not part of what F32 was measured on; the float32 composition's own error on each of them is within the
    committed figures all the same, so 4 x F32 allows the kernel there what it allows it on tolerance_cases().  A case that
    does not stay within them gets another seed (EXTRA_SHAPES names the seeds that were replaced), never a wider bound."""
    for name in EXTRA_CASES:
        measured = R.measure_f32([case(name)])
        print(name, ' '.join('%s %.2f' % (k, v / F32[k]) for k, v in measured.items()))
        for k, v in measured.items():
            assert v <= F32[k], '%s %s: committed %.3e, measured on this case %.3e' % (name, k, F32[k], v)


def test_the_extra_cases_hold_what_their_names_say():
    """The level counts, level widths, child lists and roots the extra skeletons are for, the zero rotations, and the scene
    counts around the reduce kernel's 42 slots: a change of KN_SLOTS or of the block sizes fails here instead of leaving the
    cases short of the paths they are for."""
    from dirt_amd import _lib, kinematics
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_kinematics.hip')).read()
    assert 'constexpr int KN_SLOTS = 42;' in source and '#define DIRT_KINEMATICS_SMALL_BLOCK 64' in source and _lib.KINEMATICS_MAX_JOINTS == 256
    #                              joints, levels, widest level, longest child list, roots
    for name, want in (('chain256', (256, 256, 1, 1, 1)), ('star256', (256, 2, 255, 255, 1)), ('comb128', (256, 129, 2, 2, 1)),
                       ('ladder3_255', (255, 85, 3, 1, 3)), ('roots256', (256, 1, 256, 0, 256)), ('forest200', (200, None, None, None, 70))):
        s = kinematics.Skeleton(SKELETONS[name])
        got = (s.num_joints, s.num_levels, int(s.level_offsets.diff().max()), int(s.child_offsets.diff().max()), int((s.parents < 0).sum()))
        assert all(w is None or g == w for g, w in zip(got, want)), (name, got)
        assert s.num_joints > 64        # the four-wave workgroup
    s = kinematics.Skeleton(SKELETONS['roots256'])
    assert s.child_entries.numel() == 0 and not s.child_entries.data_ptr() and s.child_offsets.tolist() == [0] * 257
    # level boundaries inside waves 1-3: the comb's at every even position from 64 on, the ladder's on every lane position mod 64
    lo = kinematics.Skeleton(SKELETONS['comb128']).level_offsets.tolist()
    assert lo[:3] == [0, 1, 3] and lo[-2:] == [255, 256] and sum(64 <= x < 256 for x in lo) == 96
    lo = kinematics.Skeleton(SKELETONS['ladder3_255']).level_offsets.tolist()
    assert lo == list(range(0, 256, 3)) and {x % 64 for x in lo if x >= 64} == set(range(64))
    forest = SKELETONS['forest200']
    assert forest[:70] == [-1] * 70 and all(0 <= q < j for j, q in enumerate(forest) if j >= 70) and kinematics.Skeleton(forest).num_levels > 2
    assert forest[3] == -1 and forest[_FOREST_INNER] >= 0 and _FOREST_INNER in forest and 199 not in forest
    for name in EXTRA_CASES:
        kw = case(name)
        skeleton, rb, pb, zeros, _ = EXTRA_SHAPES[name]
        J = len(SKELETONS[skeleton])
        assert kw['rotations'].shape == ((rb,) if rb else ()) + (J, 3) and kw['joints'].shape == ((pb,) if pb else ()) + (J, 3), name
        angles = np.linalg.norm(kw['rotations'], axis=-1)
        assert (angles[angles > 0] >= 0.3 - 1e-6).all() and sorted(np.nonzero(angles.reshape(-1, J).min(0) == 0)[0].tolist()) == sorted(zeros), name
    slots = 42
    turns = lambda scenes: -(-scenes // slots)   # noqa: E731
    assert [turns(EXTRA_SHAPES[n][2]) for n in ('b42_shared_rotations', 'b43_shared_rotations', 'b85_shared_rotations')] == [1, 2, 3]
    assert [turns(EXTRA_SHAPES[n][1]) for n in ('b3_shared_joints_chain65', 'b43_shared_joints', 'b86_shared_joints')] == [1, 2, 3]
    assert EXTRA_SHAPES['b43_shared_joints_star256'][:3] == ('star256', 43, None)


def _moved(mutated, ref, mass, kind):
    """whether some element of `mutated` lies beyond the bound the GPU comparison applies to `kind` around `ref`"""
    return R.worst_ratio(mutated, ref, mass) > KERNEL * F32[kind]


def test_the_extra_cases_bite():
    """What each extra case is for, left out of the float64 restatement (its inputs or its sums, never the kernel), moves some
    element past the bound the GPU test applies.
      - star256's root gathers 255 children; without the last one: the root's gradients with child 255's incoming gradients
        zeroed (the child's own rows change too; only the root's are looked at).
      - chain256 without its last level, backward: likewise, joint 254 without the block of joint 255; forward: joint 255 never
        composed with its parent, i.e. what it has as a root -- seen in d_joints[255], not in its own transform (below).
      - the scene sum of a shared operand stopped one row early (42 of 43, 84 of 85, 85 of 86): the per-scene rows are those
        of the same inputs with the shared operand repeated per scene, and the sum of all of them is the restatement's.
    Not expressible through the restatement: a lane without a joint writing somewhere (the C entry point test's sentinels
    check that), and a wrong barrier count, which shows as a race, not as a value of the composition."""
    for name, parent, child in (('star256', 0, 255), ('chain256', 254, 255)):
        kw, ref = case(name), reference(name)
        cut = dict(kw, grad_transforms=kw['grad_transforms'].copy(), grad_posed_joints=kw['grad_posed_joints'].copy())
        cut['grad_transforms'][child], cut['grad_posed_joints'][child] = 0., 0.
        mutated = R.compose(masses=False, **cut)
        for k in R.GRAD_KINDS:
            assert _moved(mutated[k][parent], ref[k][parent], ref['mass_' + k][parent], k), (name, k)
    # joint 255 as a root: its own transform moves by O(1), yet NOT past its bound -- the L1 mass of a transform grows with every
    # level (|R| has a norm of up to 1.7) and is beyond 1e70 at the end of this chain, so the values of the deep joints are bound
    # loosely.  What the walk left in LDS is bound tightly through d_joints all the same: d p[j] = S3[j] @ gq[j] + ... has the mass
    # of the actual |S3[j]| (the backward kernel recomputes the forward with the same walk), and that is where the mutation shows
    kw, ref = case('chain256'), reference('chain256')
    alone = R.compose(masses=False, **dict(kw, parents=kw['parents'][:255] + [-1]))
    assert float((alone['transforms'][255] - ref['transforms'][255]).abs().max()) > 1. and float(ref['mass_transforms'][255, :3, :3].min()) > 1e70
    assert float(ref['mass_d_joints'].max()) < 1e4
    assert _moved(alone['d_joints'][255], ref['d_joints'][255], ref['mass_d_joints'][255], 'd_joints')
    for k in R.VALUE_KINDS:
        assert torch.equal(alone[k][:255], ref[k][:255])
    for name, stop in SCENE_SUMS:
        kw, ref = case(name), reference(name)
        operand, k = ('rotations', 'd_rotations') if kw['rotations'].ndim == 2 else ('joints', 'd_joints')
        B = kw['grad_posed_joints'].shape[0]
        assert kw[operand].ndim == 2 and stop < B and -(-stop // 42) <= -(-B // 42)
        rows = R.compose(masses=False, **dict(kw, **{operand: np.broadcast_to(kw[operand], (B,) + kw[operand].shape).copy()}))[k]
        assert rows.shape == (B,) + tuple(ref[k].shape)
        assert R.worst_ratio(rows.sum(0), ref[k], ref['mass_' + k]) <= 1e-13, name
        assert _moved(rows[:stop].sum(0), ref[k], ref['mass_' + k], k), (name, stop)


def test_skeleton_is_the_brute_force_construction():
    from dirt_amd import kinematics
    rng = np.random.default_rng(21)
    tables = [SKELETONS[k] for k in SKELETONS] + [[], [-1, -1, -1], [-1] + rng.integers(0, np.arange(1, 50)).tolist()]
    for parents in tables:
        for given in (parents, torch.tensor(parents, dtype=torch.int64), torch.tensor(parents, dtype=torch.int32)):
            s = kinematics.Skeleton(given)
            order, level_offsets, child_entries, child_offsets = brute_force_index(parents)
            for name in s._TENSORS:
                t = getattr(s, name)
                assert t.dtype == torch.int32 and t.is_contiguous() and t.device.type == 'cpu', name
            assert s.parents.tolist() == list(parents) and s.order.tolist() == order and s.level_offsets.tolist() == level_offsets
            assert s.child_entries.tolist() == child_entries and s.child_offsets.tolist() == child_offsets
            assert s.num_joints == len(parents) and s.num_levels == len(level_offsets) - 1
            assert s.child_offsets.shape == (len(parents) + 1,) and s.order.shape == (len(parents),)
    s = kinematics.Skeleton([-1, -1, 0, 1, 1])
    assert s.order.tolist() == [0, 1, 2, 3, 4] and s.level_offsets.tolist() == [0, 2, 5]
    assert s.child_entries.tolist() == [2, 3, 4] and s.child_offsets.tolist() == [0, 1, 3, 3, 3, 3]
    s = kinematics.Skeleton([-1, 0, 1, 0, -1, 4])
    assert s.order.tolist() == [0, 4, 1, 3, 5, 2] and s.level_offsets.tolist() == [0, 2, 5, 6]
    assert s.child_entries.tolist() == [1, 3, 2, 5] and s.child_offsets.tolist() == [0, 2, 3, 3, 3, 4, 4]
    moved = s.to('cpu')
    assert isinstance(moved, kinematics.Skeleton) and moved.device.type == 'cpu' and torch.equal(moved.order, s.order)
    assert (moved.num_joints, moved.num_levels) == (6, 3)
    assert kinematics.Skeleton([-1] + [0] * 255).num_joints == 256


def test_refuses_bad_arguments():
    from dirt_amd import kinematics
    for bad, match in (([0], 'parents.0. = 0'), ([-1, 1], 'parents.1. = 1'), ([-1, 2, 0], 'parents.1. = 2'), ([-2], 'parents.0. = -2'),
                       ([-1, -2], 'parents.1. = -2'), ([-1] + [0] * 256, '257 joints, at most 256'), (torch.tensor([-1] + [0] * 256), '257 joints'),
                       ([-1, 0.], 'integer parents'), ([-1, True], 'integer parents'), (torch.tensor([-1., 0.]), 'integer tensor'),
                       (torch.zeros(2, 2, dtype=torch.int64), 'integer tensor'), (3, 'a sequence or an integer tensor'), (torch.tensor([-1, 1]), 'parents.1. = 1')):
        with pytest.raises(ValueError, match=match):
            kinematics.Skeleton(bad)
    skeleton = kinematics.Skeleton([-1, 0, 0])
    r, p = torch.zeros(3, 3), torch.zeros(3, 3)
    with pytest.raises(RuntimeError, match='runs on an MI355X only; there is no CPU fallback'):
        kinematics.pose_skeleton(r, p, skeleton)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        kinematics.pose_skeleton(r[None], p, skeleton)
    for args, match in (((torch.zeros(2, 3), p, skeleton), 'rotations must have shape'), ((r, torch.zeros(3, 4), skeleton), 'joints must have shape'),
                        ((torch.zeros(3), p, skeleton), 'rotations must have shape'), ((torch.zeros(1, 1, 3, 3), p, skeleton), 'rotations must have shape'),
                        ((r.numpy(), p, skeleton), 'rotations must have shape'), ((r, p.numpy(), skeleton), 'joints must have shape'),
                        ((r.double(), p, skeleton), 'rotations must be float32'), ((r, p.half(), skeleton), 'joints must be float32'),
                        ((r, p.to('meta'), skeleton), 'joints is on meta'), ((r.to('meta'), p.to('meta'), skeleton), 'Skeleton is on cpu'),
                        ((r, p, skeleton.to('meta')), 'Skeleton is on meta'), ((r, p, [-1, 0, 0]), 'expects a Skeleton'),
                        ((torch.zeros(2, 3, 3), torch.zeros(4, 3, 3), skeleton), '2 scenes of rotations, 4 of joints'),
                        ((torch.zeros(1, 3).expand(65536, 3, 3), p, skeleton), 'at most 65535')):
        with pytest.raises(ValueError, match=match):
            kinematics.pose_skeleton(*args)
    assert kinematics._check_arguments(r, p, skeleton) == (1, 3, False)
    assert kinematics._check_arguments(r[None], p, skeleton) == (1, 3, True)
    assert kinematics._check_arguments(r, p[None].repeat(5, 1, 1), skeleton) == (5, 3, True)
    assert kinematics._check_arguments(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), skeleton) == (2, 3, True)


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    for s in ('dirt_kinematics_scratch_bytes', 'dirt_kinematics_forward', 'dirt_kinematics_backward'):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    assert '#define DIRT_KINEMATICS_MAX_JOINTS %d' % _lib.KINEMATICS_MAX_JOINTS in header and '#define DIRT_ABI_VERSION 4' in header
    assert _lib.KINEMATICS_MAX_JOINTS == 256 == _lib.SKIN_LDS_BONES and lib.dirt_abi_version() == 4
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    good = dict(r=one, rs=2, p=one, ps=1, par=one, order=one, lo=one, levels=3, B=2, J=24, flags=0)

    def fwd(T=one, q=one, **over):
        a = dict(good, **over)
        return lib.dirt_kinematics_forward(a['r'], a['rs'], a['p'], a['ps'], a['par'], a['order'], a['lo'], a['levels'], T, q, a['B'], a['J'], a['flags'], None)

    def bwd(ce=one, co=one, gT=one, gq=one, gr=one, gp=one, scratch=one, nbytes=1 << 20, **over):
        a = dict(good, **over)
        return lib.dirt_kinematics_backward(a['r'], a['rs'], a['p'], a['ps'], a['par'], a['order'], a['lo'], a['levels'], ce, co, gT, gq, gr, gp,
                                            scratch, nbytes, a['B'], a['J'], a['flags'], None)

    bad = [dict(r=None), dict(p=None), dict(par=None), dict(order=None), dict(lo=None), dict(J=257), dict(J=-1), dict(B=-1), dict(B=65536),
           dict(rs=0), dict(rs=3), dict(ps=0), dict(ps=5), dict(levels=0), dict(levels=25), dict(levels=-1), dict(flags=1), dict(flags=1 << 31)]
    for over in bad:
        assert fwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_kinematics_forward'), over
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_kinematics_backward'), over
    # backward alone: the inverted index, and the scratch a shared operand's rows need (here: the joints of two scenes)
    for over in (dict(co=None), dict(ce=None), dict(scratch=None), dict(nbytes=8), dict(nbytes=4 * 6 * 2 * 24 - 1), dict(scratch=ctypes.c_void_p(18))):
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_kinematics_backward'), over
    with pytest.raises(ValueError, match='dirt_kinematics_backward.*dirt_kinematics_scratch_bytes'):
        _lib.check(bwd(nbytes=8))
    # no scenes or no joints: a success that launches nothing, whatever the pointers; nothing wanted likewise
    nothing = dict(r=None, p=None, par=None, order=None, lo=None, levels=0)
    assert fwd(T=None, q=None, B=0, rs=1, ps=1, **nothing) == 0 and fwd(J=0, **nothing) == 0 and fwd(T=None, q=None) == 0
    assert bwd(ce=None, co=None, gT=None, gq=None, gr=None, gp=None, scratch=None, nbytes=0, J=0, **nothing) == 0
    assert bwd(gr=None, gp=None, scratch=None, nbytes=0, gT=None, gq=None, ce=None, co=None) == 0
    assert lib.dirt_last_error() == b''
    # scratch: one row of six floats (d r, d p) per scene and joint
    assert lib.dirt_kinematics_scratch_bytes(1, 24) == 4 * 6 * 24 and lib.dirt_kinematics_scratch_bytes(32, 55) == 4 * 6 * 32 * 55
    assert lib.dirt_kinematics_scratch_bytes(65535, 256) == 4 * 6 * 65535 * 256
    assert lib.dirt_kinematics_scratch_bytes(0, 5) == 0 and lib.dirt_kinematics_scratch_bytes(5, 0) == 0
    assert lib.dirt_kinematics_scratch_bytes(-1, 5) == 0 and lib.dirt_kinematics_scratch_bytes(5, -1) == 0
    assert lib.dirt_kinematics_scratch_bytes(65536, 5) == 0 and lib.dirt_kinematics_scratch_bytes(1, 257) == 0


def test_the_module_is_exported_under_both_package_names():
    import dirt
    import dirt_amd
    import dirt.kinematics
    assert dirt.kinematics is dirt_amd.kinematics and dirt_amd.pose_skeleton is dirt_amd.kinematics.pose_skeleton
    assert dirt_amd.Skeleton is dirt_amd.kinematics.Skeleton
    from dirt_amd import build
    assert 'dirt_kinematics.hip' in build.SOURCES
    res = {k: v for k, v in build.kernel_resources().items() if 'kinematics_' in k}
    assert len(res) == 5 and all(v['scratch'] == 0 for v in res.values()), res
    assert all(v['lds'] <= 14352 for v in res.values())      # 256 joints x 12 floats + level offsets + child entries: far below 64 KB
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_kinematics.hip')).read()
    assert 'atomicAdd' not in source and 'atomic_' not in source and '__sinf' not in source and '__cosf' not in source
    assert "Forward kinematics is the caller's" not in open(os.path.join(ROOT, 'dirt_amd', 'skinning.py')).read()


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_values_and_gradients_against_the_restatement(gpu, name):
    (T, q), grads, _ = compare(case(name), gpu, name, ref=reference(name))
    if name.startswith('b1'):
        kw = case(name)
        J = len(kw['parents'])
        assert T.shape == (1, J, 4, 4) and q.shape == (1, J, 3)
        assert grads['d_rotations'].shape == kw['rotations'].shape and grads['d_joints'].shape == kw['joints'].shape


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['b3_shared_joints', 'b3_per_scene'])
@pytest.mark.parametrize('requires', GRAD_PATTERNS, ids=[''.join(n for n, on in zip('rp', r) if on) or 'none' for r in GRAD_PATTERNS])
def test_every_pattern_of_requires_grad(gpu, name, requires):
    compare(case(name), gpu, '%s requires_grad=%s' % (name, requires), requires=requires, ref=reference(name))


@pytest.mark.gpu
@pytest.mark.parametrize('name', EXTRA_CASES)
def test_extra_cases_against_the_restatement(gpu, name):
    """The four-wave workgroup at its limits (256 levels, a child list of 255, level boundaries inside waves 1-3, a forest,
    256 roots without a child entry) and scene counts of one, two and three turns of the reduce kernel's 42 slots, for either
    shared operand and with the four-wave backward: values, both gradients, both outputs used."""
    (T, q), grads, ref = compare(case(name), gpu, name, ref=reference(name))
    if name == 'roots256':      # no child entries (a NULL pointer at the C entry point): the gradients are the restatement's all the same
        assert all(bool(grads[k].abs().min() > 0) for k in R.GRAD_KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize('name', PATTERN_CASES)
@pytest.mark.parametrize('requires', GRAD_PATTERNS, ids=[''.join(n for n, on in zip('rp', r) if on) or 'none' for r in GRAD_PATTERNS])
def test_every_pattern_of_requires_grad_at_43_scenes(gpu, name, requires):
    """One operand shared by 43 scenes, the other per scene: the shared one wanted and the other too (half of every scratch row
    unused, the other gradient stored directly), the shared one alone, and the per-scene one alone (no reduce, no scratch)."""
    compare(case(name), gpu, '%s requires_grad=%s' % (name, requires), requires=requires, ref=reference(name))


@pytest.mark.gpu
@pytest.mark.parametrize('name', SAME_BITS)
def test_two_runs_of_the_extra_cases_give_the_same_bits(gpu, name):
    kw = case(name)
    (o1, g1), (o2, g2) = run_fused(kw, gpu), run_fused(kw, gpu)
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1])
    for k in R.GRAD_KINDS:
        assert torch.equal(g1[k], g2[k]) and bool(g1[k].abs().max() > 0), k


SENTINEL = -1234.5
PAD = 64     # floats in front and behind: 256 bytes, the alignment of the allocations the wrapper makes


def _padded(count, dev):
    """-> (buffer of PAD + count + PAD sentinels, the address of its middle, which keeps the buffer's own 256-byte alignment)"""
    buf = torch.full((count + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + 4 * PAD


def _middle(buf, what):
    """the floats between the paddings, after checking that both paddings still hold the sentinel"""
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), '%s: a write outside the output' % what
    return buf[PAD:-PAD]


def _c_operands(kw, dev):
    from dirt_amd import kinematics
    r, p = (torch.from_numpy(kw[k]).to(dev) for k in ('rotations', 'joints'))
    skeleton = kinematics.Skeleton(kw['parents'], device=dev)
    return r, p, skeleton, kinematics._operands(r, p) + kinematics._index_operands(skeleton)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['chain65', 'b3_shared_joints'])
def test_the_c_forward_with_one_output(gpu, name):
    """dirt_kinematics_forward with transforms = NULL, then with posed_joints = NULL (the wrapper always passes both): the
    output asked for equals the wrapper's to the bit, and the 64 floats in front of it and behind it are untouched -- with
    65 joints, 191 lanes of the workgroup have no joint and must write nothing."""
    from dirt_amd import _lib, rasterise_ops as ops
    lib = _lib.load()
    kw = case(name)
    (T, q), _ = run_fused(kw, gpu, requires=(False, False))
    r, p, skeleton, operands = _c_operands(kw, gpu)
    B, J = (kw['rotations'].shape[0] if kw['rotations'].ndim == 3 else 1), len(kw['parents'])
    for what, want, width in (('posed_joints alone', q, 3), ('transforms alone', T, 16)):
        buf, address = _padded(B * J * width, gpu)
        with ops._on_device(gpu):
            rc = lib.dirt_kinematics_forward(*operands, None if width == 3 else address, address if width == 3 else None, B, J, 0,
                                             ops._stream_handle(gpu))
        assert rc == 0, lib.dirt_last_error()
        torch.cuda.synchronize()
        assert torch.equal(_middle(buf, what), want.reshape(-1)), what


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['chain65', 'b3_shared_joints_chain65'])
def test_the_c_backward_writes_inside_its_outputs_only(gpu, name):
    """dirt_kinematics_backward on 65 joints (191 lanes without one), one scene and three scenes with shared joints: both
    gradients equal the wrapper's to the bit, and the paddings around them -- and around the scratch the shared joints' rows
    go to -- are untouched."""
    from dirt_amd import _lib, rasterise_ops as ops
    lib = _lib.load()
    kw = case(name)
    _, grads = run_fused(kw, gpu)
    r, p, skeleton, operands = _c_operands(kw, gpu)
    B, J = (kw['rotations'].shape[0] if kw['rotations'].ndim == 3 else 1), len(kw['parents'])
    gT, gq = (torch.from_numpy(kw[g]).to(gpu) for g in ('grad_transforms', 'grad_posed_joints'))
    nbytes = lib.dirt_kinematics_scratch_bytes(B, J) if B > 1 else 0
    assert nbytes == (4 * 6 * B * J if B > 1 else 0)
    (gr, gr_at), (gp, gp_at), (scratch, scratch_at) = _padded(r.numel(), gpu), _padded(p.numel(), gpu), _padded(nbytes // 4, gpu)
    with ops._on_device(gpu):
        rc = lib.dirt_kinematics_backward(*operands, skeleton.child_entries.data_ptr(), skeleton.child_offsets.data_ptr(), gT.data_ptr(), gq.data_ptr(),
                                          gr_at, gp_at, scratch_at if nbytes else None, nbytes, B, J, 0, ops._stream_handle(gpu))
    assert rc == 0, lib.dirt_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_middle(gr, 'grad_rotations'), grads['d_rotations'].reshape(-1))
    assert torch.equal(_middle(gp, 'grad_joints'), grads['d_joints'].reshape(-1))
    rows = _middle(scratch, 'scratch')
    if nbytes:      # rotations per scene: stored directly, so columns 0-2 of every scratch row stay as they were
        rows = rows.reshape(B, J, 6)
        assert bool((rows[..., :3] == SENTINEL).all()) and bool((rows[..., 3:] != SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize('name, unused', ONE_OUTPUT)
def test_a_gradient_through_one_output_only(gpu, name, unused):
    """An output nobody used contributes nothing: the other's gradient alone, against the restatement without it."""
    kw = dict(case(name), **{unused: None})
    compare(kw, gpu, '%s without %s' % (name, unused))


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
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + 3,), 7., device=dev)
    buf[..., :t.shape[-1]] = t
    view = buf[..., :t.shape[-1]]
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _run_presented(kw, dev, how):
    from dirt_amd import kinematics
    leaves = [_presented(kw[k], how, dev).detach().requires_grad_(True) for k in ('rotations', 'joints')]
    T, q = kinematics.pose_skeleton(leaves[0], leaves[1], kinematics.Skeleton(kw['parents'], device=dev))
    torch.autograd.backward([T, q], [_presented(kw[g], how, dev) for g in ('grad_transforms', 'grad_posed_joints')])
    return (T, q), leaves


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['smpl', 'b3_shared_joints_tree256'])
def test_misaligned_and_non_contiguous_operands(gpu, name):
    """The same values as contiguous views 4 bytes past a 16-byte boundary (the kernels' 12- and 16-byte accesses to rows that
    are only 4-byte aligned) and as non-contiguous views (the wrapper's .contiguous() branches), the incoming gradients
    likewise: the kernels see the same numbers in the same order, so the outputs and both gradients equal the plain run's to
    the bit, and every leaf's .grad has the leaf's shape."""
    kw = case(name)
    plain, plain_leaves = _run_presented(kw, gpu, 'plain')
    assert all(bool(l.grad.abs().max() > 0) for l in plain_leaves)
    for how in ('misaligned', 'strided'):
        outs, leaves = _run_presented(kw, gpu, how)
        assert torch.equal(plain[0], outs[0]) and torch.equal(plain[1], outs[1]), how
        for k, a, b in zip(R.GRAD_KINDS, plain_leaves, leaves):
            assert b.grad.shape == b.shape and torch.equal(a.grad, b.grad), (how, k)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_backward_is_reentrant(gpu):
    from dirt_amd import kinematics
    for name in ('smpl', 'star66', 'b3_shared_joints_tree256', 'b70_shared_joints', 'b3_per_scene'):
        kw = case(name)
        (o1, g1), (o2, g2) = run_fused(kw, gpu), run_fused(kw, gpu)
        assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1]), name
        for k in R.GRAD_KINDS:
            assert torch.equal(g1[k], g2[k]), (name, k)     # bit for bit: fixed-order sums, no atomics
    # backward twice over one forward (retain_graph=True); the node saves its two inputs and nothing else
    kw = case('b3_shared_joints')
    _, g1 = run_fused(kw, gpu)
    r, p = (torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('rotations', 'joints'))
    T, q = kinematics.pose_skeleton(r, p, kinematics.Skeleton(kw['parents'], device=gpu))
    saved = T.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == r.data_ptr() and saved[1].data_ptr() == p.data_ptr()
    go = [torch.from_numpy(kw[g]).to(gpu) for g in ('grad_transforms', 'grad_posed_joints')]
    a = torch.autograd.grad([T, q], [r, p], go, retain_graph=True)
    b = torch.autograd.grad([T, q], [r, p], go, retain_graph=True)
    for x, y, k in zip(a, b, R.GRAD_KINDS):
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr(), k
        assert torch.equal(x, g1[k]), k


@pytest.mark.gpu
def test_a_captured_step_replays_to_the_bits_of_eager(gpu):
    """pose_skeleton makes no host synchronisation: a step (stage, loss, gradients) is captured with torch.cuda.graph on one
    stream, without branches, and its replay, after the rotations changed in place, returns the loss and gradients of the eager
    step to the bit."""
    from dirt_amd import kinematics
    kw = case('b3_shared_joints')
    r, p = (torch.from_numpy(kw[k]).to(gpu) for k in ('rotations', 'joints'))
    skeleton = kinematics.Skeleton(kw['parents'], device=gpu)
    target = torch.from_numpy(kw['grad_posed_joints']).to(gpu)

    def step():
        leaves = [t.detach().requires_grad_(True) for t in (r, p)]
        T, q = kinematics.pose_skeleton(*leaves, skeleton)
        loss = ((q - target) ** 2).mean() + (T ** 2).sum() * 1e-3
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
        r += 0.01 * torch.from_numpy(np.random.default_rng(5).standard_normal(r.shape).astype(np.float32)).to(gpu)
    graph.replay()
    loss_e, grads_e = step()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for a, b in zip(grads_g, grads_e):
        assert torch.equal(a, b) and bool(a.abs().max() > 0)


@pytest.mark.gpu
def test_the_chain_of_three_stages_equals_the_stages_run_apart(gpu):
    """pose_skeleton -> skin_vertices -> vertex_stage in one autograd graph (posed joints used beside) against the three stages
    run apart, each on detached inputs and fed the gradient the next one returned: the same kernels on the same numbers, so
    the outputs and the gradients to the rotations and the joints agree to the bit."""
    from dirt_amd import geometry, kinematics, skinning
    from tests import skin_reference
    kw = case('b3_shared_joints')
    rng = np.random.default_rng(8400)
    V, F, J = 300, 500, len(kw['parents'])
    rest = torch.from_numpy(rng.uniform(-1., 1., (V, 3)).astype(np.float32)).to(gpu)
    idx, w = skin_reference.random_weights(rng, V, 4, J)
    skin = skinning.SkinWeights(torch.from_numpy(idx).to(gpu), torch.from_numpy(w).to(gpu), J)
    topology = geometry.MeshTopology(torch.from_numpy(rng.integers(0, V, (F, 3)).astype(np.int32)).to(gpu), V)
    skeleton = kinematics.Skeleton(kw['parents'], device=gpu)
    vp = torch.from_numpy((np.eye(4) + rng.uniform(-0.2, 0.2, (4, 4))).astype(np.float32)).to(gpu)
    g_clip, g_normals = (torch.from_numpy(rng.standard_normal((3, V, n)).astype(np.float32)).to(gpu) for n in (4, 3))
    g_q = torch.from_numpy(kw['grad_posed_joints']).to(gpu)

    def leaves():
        return [torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('rotations', 'joints')]

    r, p = leaves()
    T, q = kinematics.pose_skeleton(r, p, skeleton)
    posed = skinning.skin_vertices(rest, skin, T)
    clip, _, normals = geometry.vertex_stage(posed, topology, None, vp)
    torch.autograd.backward([clip, normals, q], [g_clip, g_normals, g_q])

    r2, p2 = leaves()
    T2, q2 = kinematics.pose_skeleton(r2, p2, skeleton)
    T_leaf = T2.detach().requires_grad_(True)
    posed2 = skinning.skin_vertices(rest, skin, T_leaf)
    posed_leaf = posed2.detach().requires_grad_(True)
    clip2, _, normals2 = geometry.vertex_stage(posed_leaf, topology, None, vp)
    torch.autograd.backward([clip2, normals2], [g_clip, g_normals])
    posed2.backward(posed_leaf.grad)
    torch.autograd.backward([T2, q2], [T_leaf.grad, g_q])

    for a, b in ((T, T2), (q, q2), (posed, posed2), (clip, clip2), (normals, normals2), (r.grad, r2.grad), (p.grad, p2.grad)):
        assert torch.equal(a, b) and bool(a.abs().max() > 0)
    assert r.grad.shape == (3, J, 3) and p.grad.shape == (J, 3)


@pytest.mark.gpu
def test_the_torch_loop_agrees(gpu):
    """The kernel against the loop users write, in float32 on the GPU (rodrigues / translation / compose per joint, generalised
    from examples/fit_pose_fused.py to the SMPL tree): both are float32 evaluations of one composition -- torch's within F32
    of the float64 one, the kernel within 4 x that -- so they are within 5 x of each other, by the mass of the terms."""
    name = 'b3_shared_joints'
    kw, ref = case(name), reference(name)
    (T, q), grads = run_fused(kw, gpu)
    r2, p2 = (torch.from_numpy(kw[k]).to(gpu).requires_grad_(True) for k in ('rotations', 'joints'))
    T2, q2 = R.loop(r2, p2, kw['parents'])
    torch.autograd.backward([T2, q2], [torch.from_numpy(kw[g]).to(gpu) for g in ('grad_transforms', 'grad_posed_joints')])
    # column 3 of the loop's product is 0 and 1 as well: sums of exact zeros, and 1 * 1
    close(T, T2.detach().cpu().numpy(), ref['mass_transforms'], 5 * F32['transforms'], 'torch loop: transforms')
    close(q, q2.detach().cpu().numpy(), ref['mass_posed_joints'], 5 * F32['posed_joints'], 'torch loop: posed_joints')
    close(grads['d_rotations'], r2.grad.cpu().numpy(), ref['mass_d_rotations'], 5 * F32['d_rotations'], 'torch loop: d_rotations')
    close(grads['d_joints'], p2.grad.cpu().numpy(), ref['mass_d_joints'], 5 * F32['d_joints'], 'torch loop: d_joints')


@pytest.mark.gpu
def test_the_body_pose_fitting_example_descends(gpu):
    """examples/fit_body_pose_fused.py: pose_skeleton -> skin_vertices -> vertex_stage -> rasterise_deferred with shade_gbuffer,
    an image loss plus a key-point loss on the projected posed joints, for a few steps of gradient descent on the joint
    rotations: the losses are finite and the loop ends below where it began."""
    losses = _load_example('fit_body_pose_fused').main(steps=12)
    assert len(losses) == 12 and all(np.isfinite(losses)) and losses[-1] < losses[0]
