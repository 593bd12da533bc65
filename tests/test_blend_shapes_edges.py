"""Edges of blend shapes (dirt_blend.hip, dirt_amd/blendshapes.py) that tests/test_blend_shapes.py leaves out: the C entry
points in every combination of outputs and incoming gradients include/dirt_hip.h allows, every output in a buffer with
sentinels around it and the scratch full of garbage; non-finite values, which must stay with the terms the specification
gives them (the sparse sums of the header of dirt_blend.hip, not the dense restatement's); the largest batch, B = 65535,
to the bit; the gradients of a scene alone and in a batch; the wrapper's empty calls on the GPU.

The cases are the smallest that reach each path (test_the_extra_cases_hold_what_their_names_say); the tolerances are those
of tests/test_blend_shapes.py, KERNEL = 4 x the committed float32 figures F32, which the float32 composition's own error on
every input used here stays within (test_extra_cases_stay_within_the_committed_figures)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import blend_reference as R
from tests.test_blend_shapes import F32, _random, case, compare, run_fused, shapes_of
from tests.test_kinematics import PAD, SENTINEL, _middle, _padded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = R.VALUE_KINDS + R.GRAD_KINDS
SOURCES = ('both', 'vertices', 'joints')

# name: ((V, K, Ks, J, scenes of the template, scenes of the coefficients), seed).  3 V = 258: 65 live lanes of 256, the last
# quad holding two elements, one slab; K = 9: two ranges of BL_KR = 8, the second with one live direction; Ks = 4 inside the
# first; J = 5: two joint workgroups, three of the second's four waves without a joint; B = 5: the second tile holds one live
# scene and three dead slots.
EXTRA = {
    'c_one': ((86, 9, 4, 5, None, None), 8800),
    'c_b5': ((86, 9, 4, 5, 5, 5), 8801),
    'c_b5_shared_c': ((86, 9, 4, 5, 5, None), 8802),
    'c_b5_shared_t': ((86, 9, 4, 5, None, 5), 8803),
}
EXTRA_CASES = list(EXTRA)
MOST = 65535                      # the documented maximum of B, and exactly the limit of gridDim.y


def extra_case(name, source='both'):
    """As test_blend_shapes.case: the keyword arguments of blend_reference.compose; source: the outputs the gradient arrives from"""
    shape, seed = EXTRA[name]
    kw = _random(*shape, None, seed=seed)
    if source == 'vertices':
        kw['grad_joints'] = None
    if source == 'joints':
        kw['grad_vertices'] = None
    return kw


def gradient_case():
    """Two slabs and three ranges, five scenes of both operands"""
    return _random(342, 17, 9, 24, 5, 5, None, seed=8805)


def most_scenes_case():
    """exact_case's values at B = 65535 scenes of V = 2, K = 3, Ks = 2, J = 1, every operand and gradient per scene: the template
    and the gradients integers in -3 .. 3, the directions in -2 .. 2, the coefficients and the regressor's two weights in
    {0.25, +-0.5, 1, 2}: joint_directions are multiples of 1/4 and every product and sum a multiple of 1/64 far below
    2^24 / 64, exact in float32 in any order."""
    rng = np.random.default_rng(8804)
    B, V, K, J = MOST, 2, 3, 1
    values = np.asarray([0.25, 0.5, -0.5, 1., 2.], np.float32)
    return dict(template=rng.integers(-3, 4, (B, V, 3)).astype(np.float32), coefficients=rng.choice(values, (B, K)),
                directions=rng.integers(-2, 3, (K, V, 3)).astype(np.float32), regressor=rng.choice(values, (J, V)), joint_shapes=2,
                grad_vertices=rng.integers(-3, 4, (B, V, 3)).astype(np.float32), grad_joints=rng.integers(-3, 4, (B, J, 3)).astype(np.float32))


def sizes_of(kw):
    """-> (B, V, K, Ks, J, scenes of the template, scenes of the coefficients) as the C ABI takes them"""
    K, V = kw['directions'].shape[:2]
    J = 0 if kw['regressor'] is None else kw['regressor'].shape[0]
    t, c = kw['template'], kw['coefficients']
    B = t.shape[0] if t.ndim == 3 else c.shape[0] if c.ndim == 2 else 1
    return B, V, K, kw['joint_shapes'], J, B if t.ndim == 3 else 1, B if c.ndim == 2 else 1


# ------------------------------------------------------------------------------------------- non-finite values: the expectation

CLEAN, NONFINITE, NAN, PINF = 0, 1, 2, 3     # per element: the bits of the clean run; not finite; NaN; +inf
POISONS = ('template', 'coefficients', 'grad_vertices', 'grad_joints', 'directions')


def sparse_specification(kw):
    """The specification in the header of dirt_blend.hip, term by term in float64 numpy: the joints and the template's gradient
    over the regressor's NON-ZEROS only, the joint term over k < Ks only -- so a non-finite value reaches exactly the sums
    that hold a term with it (the dense restatement multiplies the regressor's zeros by it and spreads NaN over every joint)."""
    t, c, D = (np.asarray(kw[k], np.float64) for k in ('template', 'coefficients', 'directions'))
    reg, Ks = np.asarray(kw['regressor'], np.float64), kw['joint_shapes']
    B, V, K, _, J, _, _ = sizes_of(kw)
    jd = R.joint_directions(kw['regressor'], kw['directions'], Ks).double().numpy()
    tb, cb = np.broadcast_to(t, (B, V, 3)), np.broadcast_to(c, (B, K))
    gv = np.zeros((B, V, 3)) if kw['grad_vertices'] is None else np.asarray(kw['grad_vertices'], np.float64).reshape(B, V, 3)
    gj = np.zeros((B, J, 3)) if kw['grad_joints'] is None else np.asarray(kw['grad_joints'], np.float64).reshape(B, J, 3)
    with np.errstate(invalid='ignore'):
        vertices, joints, dt, dc = tb.copy(), np.zeros((B, J, 3)), gv.copy(), np.zeros((B, K))
        for k in range(K):
            vertices += cb[:, k, None, None] * D[k]
            dc[:, k] = (D[k].reshape(-1) * gv.reshape(B, -1)).sum(1)
            if k < Ks:
                dc[:, k] += (jd[k].reshape(-1) * gj.reshape(B, -1)).sum(1)
        for j, v in zip(*np.nonzero(reg)):
            joints[:, j] += reg[j, v] * tb[:, v]
            dt[:, v] += reg[j, v] * gj[:, j]
        for k in range(Ks):
            joints += cb[:, k, None, None] * jd[k]
    return {'vertices': vertices, 'joints': joints, 'd_template': dt if t.ndim == 3 else dt.sum(0), 'd_coefficients': dc if c.ndim == 2 else dc.sum(0)}


def poison_variants(which):
    """-> [(label, clean keyword arguments, the same with one value replaced, {kind: int array of CLEAN / NONFINITE / NAN / PINF
    per element})].  The set of a poison -- the elements that are not CLEAN -- comes from the sparse structure: the regressor's
    non-zeros and k < Ks.  The vertices and joints are chosen from the data: a vertex some joint names, one none names, the
    joint with the longest row.  All in scene 4, the lone live scene of the second tile, unless the issue of the case is
    another tile."""
    out = []

    def add(label, clean, change, expect):
        dirty = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
        change(dirty)
        B, V, K, Ks, J, ts, cs = sizes_of(clean)
        want = {'vertices': np.zeros((B, V, 3), np.int8), 'joints': np.zeros((B, J, 3), np.int8),
                'd_template': np.zeros(clean['template'].shape, np.int8), 'd_coefficients': np.zeros(clean['coefficients'].shape, np.int8)}
        expect(want)
        out.append((label, clean, dirty, want))

    base = extra_case('c_b5')
    reg, Ks = base['regressor'], base['joint_shapes']
    named = (reg != 0).any(0)
    if which == 'template':
        v = int(np.flatnonzero(named)[0])
        rows = np.flatnonzero(reg[:, v])

        def expect(want):
            want['vertices'][4, v, 0] = PINF
            want['joints'][4, rows, 0] = NONFINITE
        add('template[4, %d, 0] = +inf' % v, base, lambda kw: kw['template'].__setitem__((4, v, 0), np.inf), expect)
    if which == 'coefficients':
        for k in (2, 6):
            def expect(want, k=k):
                want['vertices'][1] = NAN
                if k < Ks:
                    want['joints'][1] = NAN
            add('coefficients[1, %d] = NaN' % k, base, lambda kw, k=k: kw['coefficients'].__setitem__((1, k), np.nan), expect)
    if which == 'grad_vertices':
        for name in ('c_b5', 'c_b5_shared_c'):
            clean = extra_case(name)
            v = int(np.flatnonzero(~(clean['regressor'] != 0).any(0))[0])

            def expect(want, v=v, shared=clean['coefficients'].ndim == 1):
                want['d_template'][4, v, 1] = NAN
                want['d_coefficients'][() if shared else 4] = NAN
            add('%s: grad_vertices[4, %d, 1] = NaN' % (name, v), clean, lambda kw, v=v: kw['grad_vertices'].__setitem__((4, v, 1), np.nan), expect)
    if which == 'grad_joints':
        j = int(np.argmax((reg != 0).sum(1)))
        column = np.flatnonzero(reg[j])

        def expect(want):
            want['d_template'][4, column, 2] = NONFINITE
            want['d_coefficients'][4, :Ks] = NONFINITE
        add('grad_joints[4, %d, 2] = +inf' % j, base, lambda kw: kw['grad_joints'].__setitem__((4, j, 2), np.inf), expect)
    if which == 'directions':
        clean = extra_case('c_b5')
        clean['coefficients'][:, 6] = 0.75
        clean['grad_vertices'][:, 0, 0] = 1.5

        def expect(want):
            want['vertices'][:, 0, 0] = PINF
            want['d_coefficients'][:, 6] = PINF
        add('directions[6, 0, 0] = +inf', clean, lambda kw: kw['directions'].__setitem__((6, 0, 0), np.inf), expect)
    return out


def check_poisoned(label, kind, got, clean, want):
    got, clean = (np.ascontiguousarray(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)).reshape(want.shape) for x in (got, clean))
    what = '%s: %s' % (label, kind)
    assert np.isfinite(clean).all(), what
    if got.dtype == np.float32:
        same = got.view(np.uint32) == clean.view(np.uint32)
    else:
        same = got == clean
    assert same[want == CLEAN].all(), '%s: %d elements outside the set differ from the clean run' % (what, int((~same[want == CLEAN]).sum()))
    assert not np.isfinite(got[want != CLEAN]).any(), '%s: a finite element inside the set' % what
    assert np.isnan(got[want == NAN]).all(), '%s: not NaN' % what
    assert (got[want == PINF] == np.inf).all(), '%s: not +inf' % what


# ---------------------------------------------------------------------------------------------------------------- CPU tests

def test_extra_cases_stay_within_the_committed_figures():
    """The inputs of this file are not part of what F32 was measured on; the float32 composition's own error on each of them --
    the four extra cases with the gradient arriving from both outputs, the vertices alone and the joints alone, the clean
    inputs of the non-finite cases (the directions' case changes a coefficient column and a gradient) and the five scenes of
    the gradient test -- is within the committed figures all the same, so 4 x F32 allows the kernel here what it allows it
    on tolerance_cases().  A case that does not stay within them gets another seed, never a wider bound."""
    cases = [('%s from %s' % (name, source), extra_case(name, source)) for name in EXTRA_CASES for source in SOURCES]
    cases += [(label, clean) for which in POISONS for label, clean, _, _ in poison_variants(which)]
    cases += [('gradient case', gradient_case())]
    worst = {k: 0. for k in KINDS}
    for what, kw in cases:
        measured = R.measure_f32([kw])
        for k, v in measured.items():
            worst[k] = max(worst[k], v)
            assert v <= F32[k], '%s %s: committed %.3e, measured on this case %.3e' % (what, k, F32[k], v)
    print(' '.join('%s %.3e' % kv for kv in worst.items()))


def test_the_extra_cases_hold_what_their_names_say():
    """The constants the extra cases bracket are those of the source, and every case reaches what it is for."""
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_blend.hip')).read()
    const = {name: int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1)) for name in ('BL_BLOCK', 'BL_QUAD', 'BL_S', 'BL_KR', 'BL_SLOTS')}
    assert const == {'BL_BLOCK': 256, 'BL_QUAD': 4, 'BL_S': 4, 'BL_KR': 8, 'BL_SLOTS': 32}
    for name in EXTRA_CASES:
        (V, K, Ks, J, tb, cb), _ = EXTRA[name]
        assert 3 * V == 258 == 64 * const['BL_QUAD'] + 2 and 3 * V <= const['BL_BLOCK'] * const['BL_QUAD']      # 65 live lanes, a quad of two, one slab
        assert -(-K // const['BL_KR']) == 2 and K % const['BL_KR'] == 1 and 0 < Ks < const['BL_KR']
        assert -(-J // 4) == 2 and J % 4 == 1
        assert (tb or cb) in (None, const['BL_S'] + 1)
        kw = extra_case(name)
        assert sizes_of(kw) == (tb or cb or 1, V, K, Ks, J, tb or 1, cb or 1)
        assert not (kw['directions'] == 0).any()
        named = (kw['regressor'] != 0).any(0)
        assert named.any() and not named.all() and (kw['regressor'] != 0).any(1).all()      # a vertex some joint names, one none names, no empty row
    assert {(EXTRA[n][0][4] is not None, EXTRA[n][0][5] is not None) for n in EXTRA_CASES} == {(False, False), (True, True), (True, False), (False, True)}
    V, K, Ks, J, tb, cb = 342, 17, 9, 24, 5, 5
    assert sizes_of(gradient_case()) == (5, V, K, Ks, J, 5, 5) and -(-3 * V // 1024) == 2 and -(-K // const['BL_KR']) == 3 and const['BL_KR'] < Ks
    assert sizes_of(case('k0_b3'))[2:4] == (0, 0) and sizes_of(case('k0_b3'))[0] == 3 and sizes_of(case('j0_b2'))[4] == 0 and sizes_of(case('j0_b2'))[0] == 2


def test_the_largest_batch_is_exact_in_float32():
    """B = 65535 is the most blend_check admits; on most_scenes_case() the float32 composition equals the float64 one
    exactly, every value a multiple of 1/64 far below 2^24 / 64: the GPU test compares to the bit."""
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_blend.hip')).read()
    assert 'B > %d ' % MOST in source
    kw = most_scenes_case()
    assert sizes_of(kw) == (MOST, 2, 3, 2, 1, MOST, MOST) and (kw['regressor'] != 0).all()
    ref = R.compose(**kw)
    ref32 = R.compose(dtype=torch.float32, masses=False, **kw)
    for k in KINDS:
        assert 2 ** 24 > 64 * float(ref['mass_' + k].max()), k
        assert bool((64 * ref[k] == (64 * ref[k]).round()).all()) and torch.equal(ref32[k].double(), ref[k]), k
        assert bool(ref[k][-1].abs().sum() > 0) and len(np.unique(ref[k].numpy().reshape(MOST, -1), axis=0)) > 1000, k    # the last scene is no zero; the scenes differ


@pytest.mark.parametrize('which', POISONS)
def test_the_influence_sets_are_strict_and_those_of_the_specification(which):
    """Every set of the non-finite cases is neither empty nor everything, and is what the specification gives when it is
    evaluated term by term over the sparse structure (sparse_specification, float64): outside the set the poisoned
    evaluation equals the clean one exactly, inside it is not finite, NaN or +inf where the case says so.  The sparse
    evaluation itself agrees with the dense restatement on the clean inputs."""
    variants = poison_variants(which)
    assert len(variants) == {'coefficients': 2, 'grad_vertices': 2}.get(which, 1)
    for label, clean, dirty, want in variants:
        assert sum(int((clean[k] != dirty[k]).sum()) for k in clean if isinstance(clean[k], np.ndarray)) == 1, label    # one value replaced
        inside, total = sum(int((w != CLEAN).sum()) for w in want.values()), sum(w.size for w in want.values())
        assert 0 < inside < total, label
        for k, w in want.items():
            assert not (w != CLEAN).all() or (k == 'd_coefficients' and 'shared_c' in label), (label, k)
        spec_clean, spec_dirty, ref = sparse_specification(clean), sparse_specification(dirty), R.compose(**clean)
        for k in KINDS:
            assert np.allclose(spec_clean[k], ref[k].numpy(), rtol=1e-12, atol=1e-12), (label, k)
            check_poisoned(label + ' (specification)', k, spec_dirty[k], spec_clean[k], want[k])
        assert not (clean['directions'] == 0).any() and np.isfinite(R.joint_directions(dirty['regressor'], dirty['directions'], dirty['joint_shapes']).numpy()).all()
    if which == 'directions':
        # the test bites: the 191 dead lanes of the slab read quad 0 of the row with a zero gradient; without `&& live` one of them adds 0 x inf
        with np.errstate(invalid='ignore'):
            assert np.isnan(np.float32(0.) * dirty['directions'][6, 0, 0] + np.float32(np.inf))
    if which == 'coefficients':
        # the test bites: a joint term bounded by K instead of Ks would add c[1, 6] x (a finite value) = NaN to joints[1]
        assert variants[1][2]['joint_shapes'] <= 6 < variants[1][2]['directions'].shape[0] and (variants[1][3]['joints'] == CLEAN).all()


# ---------------------------------------------------------------------------------------------------------------- GPU tests

def _device_operands(kw, dev):
    return shapes_of(kw, dev), torch.from_numpy(kw['template']).to(dev), torch.from_numpy(kw['coefficients']).to(dev)


def _c_forward(dev, kw, shapes, t, c, vertices_at, joints_at, directions=True, regressor=True):
    """dirt_blend_forward with the operands as _BlendShapes.forward passes them; directions / regressor False: NULL instead"""
    from dirt_amd import _lib, rasterise_ops as ops
    from dirt_amd._stage import ptr
    lib = _lib.load()
    B, V, K, Ks, J, ts, cs = sizes_of(kw)
    with ops._on_device(dev):
        rc = lib.dirt_blend_forward(ptr(t), ts, ptr(c) if directions else None, cs, ptr(shapes.packed) if directions else None, shapes.stride,
                                    shapes.row_offsets.data_ptr() if regressor else None, ptr(shapes.row_vertices) if regressor else None,
                                    ptr(shapes.row_weights) if regressor else None, ptr(shapes.joint_directions) if regressor else None, vertices_at,
                                    joints_at, B, V, K, Ks, J, 0, ops._stream_handle(dev))
    assert rc == 0 and lib.dirt_last_error() == b'', lib.dirt_last_error()
    torch.cuda.synchronize()


def _c_backward(dev, kw, shapes, gv, gj, template_at, coefficients_at, scratch_at, nbytes, columns=True, directions=True, joint_directions=True):
    """dirt_blend_backward with the operands as _BlendShapes.backward passes them; columns / directions False: NULL instead"""
    from dirt_amd import _lib, rasterise_ops as ops
    from dirt_amd._stage import ptr
    lib = _lib.load()
    B, V, K, Ks, J, ts, cs = sizes_of(kw)
    with ops._on_device(dev):
        rc = lib.dirt_blend_backward(ts, cs, ptr(shapes.packed) if directions else None, shapes.stride, shapes.column_offsets.data_ptr() if columns else None,
                                     ptr(shapes.column_joints) if columns else None, ptr(shapes.column_weights) if columns else None,
                                     ptr(shapes.joint_directions) if joint_directions else None, ptr(gv), ptr(gj), template_at, coefficients_at, scratch_at,
                                     nbytes, B, V, K, Ks, J, 0, ops._stream_handle(dev))
    assert rc == 0 and lib.dirt_last_error() == b'', lib.dirt_last_error()
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('name', EXTRA_CASES)
def test_the_c_forward_with_one_output(gpu, name):
    """dirt_blend_forward with vertices = NULL (the joint workgroups then start at blockIdx.x = 0), with joints = NULL (no joint
    workgroup) and with both (the wrapper's call): the output asked for equals the wrapper's to the bit -- which is within
    4 x F32 of the restatement -- and the 64 floats in front of it and behind it still hold the sentinel.  It bites: 3 V =
    258, so the last live lane's quad holds two elements and a store_quad without its tail branch writes two floats past the
    output; 191 lanes of the slab and three waves of the second joint workgroup have nothing and must write nothing; with
    five scenes the second tile computes three dead slots (a repeat of scene 4), and a forward that stored them would write
    3 x 258 floats behind the vertices, over the padding."""
    kw = extra_case(name)
    vertices, joints, _, _ = compare(kw, gpu, name, requires=(False, False))
    shapes, t, c = _device_operands(kw, gpu)
    for what, want_vertices, want_joints in (('joints alone', False, True), ('vertices alone', True, False), ('both', True, True)):
        (vbuf, vertices_at), (jbuf, joints_at) = _padded(vertices.numel(), gpu), _padded(joints.numel(), gpu)
        _c_forward(gpu, kw, shapes, t, c, vertices_at if want_vertices else None, joints_at if want_joints else None)
        got_vertices, got_joints = _middle(vbuf, '%s: vertices' % what), _middle(jbuf, '%s: joints' % what)
        assert torch.equal(got_vertices, vertices.reshape(-1)) if want_vertices else bool((got_vertices == SENTINEL).all()), what
        assert torch.equal(got_joints, joints.reshape(-1)) if want_joints else bool((got_joints == SENTINEL).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize('name', EXTRA_CASES)
def test_the_c_backward_in_every_combination_the_header_allows(gpu, name):
    """dirt_blend_backward for grad_template alone (no scratch, no column index needed by anything else), grad_coefficients
    alone (column_* NULL) and both, with both incoming gradients, either one NULL, and both NULL.  Wherever the wrapper can
    make the same call (requires_grad and the output used) the results equal its to the bit, and the wrapper's are within
    4 x F32 of the restatement; with both incoming NULL every output given is exactly zero: fully written.  Every output
    and the scratch -- exactly dirt_blend_scratch_bytes(B, V, K) bytes -- lie between 64 sentinels that must survive.  The
    scratch is first full of the sentinel, then of NaN: the same bits both times, so the second launch reads no row this
    call did not write (a reduce that read one row too many, or the dead slots' rows of another tile, would carry the NaN
    into d c), and afterwards no float of it holds what it was filled with: with one slab every row is written, also when
    grad_vertices = NULL launches slab 0 alone."""
    from dirt_amd import _lib
    lib = _lib.load()
    B, V, K, Ks, J, ts, cs = sizes_of(extra_case(name))
    nbytes = lib.dirt_blend_scratch_bytes(B, V, K)
    assert nbytes == 4 * 32 * -(-B // 4) * -(-K // 8) * -(-3 * V // 1024)
    kw_both = extra_case(name)
    shapes, t, c = _device_operands(kw_both, gpu)
    for source in SOURCES + ('none',):
        kw = extra_case(name, source) if source != 'none' else dict(kw_both, grad_vertices=None, grad_joints=None)
        gv, gj = (None if kw[k] is None else torch.from_numpy(kw[k]).to(gpu) for k in ('grad_vertices', 'grad_joints'))
        for requires in ((True, False), (False, True), (True, True)):
            what = '%s from %s, outputs %s' % (name, source, requires)
            grads = compare(kw, gpu, what, requires=requires)[2] if source != 'none' else None
            results = []
            for fill in (SENTINEL, float('nan')):
                (tbuf, template_at), (cbuf, coefficients_at), (sbuf, scratch_at) = _padded(t.numel(), gpu), _padded(c.numel(), gpu), _padded(nbytes // 4, gpu)
                sbuf[PAD:-PAD] = fill
                _c_backward(gpu, kw, shapes, gv, gj, template_at if requires[0] else None, coefficients_at if requires[1] else None,
                            scratch_at if requires[1] else None, nbytes if requires[1] else 0, columns=requires[0])
                got = [_middle(b, '%s: %s' % (what, k)).clone() for b, k in ((tbuf, 'grad_template'), (cbuf, 'grad_coefficients'))]
                rows = _middle(sbuf, what + ': scratch')
                if requires[1]:
                    assert not bool((rows == SENTINEL).any()) and not bool(rows.isnan().any()), '%s: a row of the scratch was not written' % what
                else:
                    assert bool((rows == SENTINEL).all() if fill == SENTINEL else rows.isnan().all()), '%s: scratch nobody passed was written' % what
                results.append(got)
            for k, on, first, second in zip(R.GRAD_KINDS, requires, *results):
                assert torch.equal(first, second), '%s: %s depends on what the scratch held' % (what, k)
                if not on:
                    assert bool((first == SENTINEL).all()), '%s: %s was not asked for' % (what, k)
                elif source == 'none':
                    assert bool((first == 0).all()), '%s: %s is not zero' % (what, k)
                else:
                    assert torch.equal(first, grads[k].reshape(-1)), '%s: %s differs from the wrapper' % (what, k)


@pytest.mark.gpu
def test_sizes_the_c_entry_points_ignore(gpu):
    """K = 0 (directions = NULL, coefficients = NULL): the forward still copies the template and regresses the joints, the
    backward still writes grad_template, and a grad_coefficients buffer that is passed all the same is left untouched.
    J = 0: non-NULL joints and grad_joints pointers are ignored -- the output buffer keeps its sentinels, the gradients are
    those of the wrapper, which passes NULL for both.  The wrapper's results on these two cases are compared with the
    restatement by tests/test_blend_shapes.py."""
    kw = case('k0_b3')
    assert sizes_of(kw)[2] == 0
    vertices, joints, grads = run_fused(kw, gpu, requires=(True, False))
    assert torch.equal(vertices.cpu(), torch.from_numpy(kw['template']))
    shapes, t, c = _device_operands(kw, gpu)
    (vbuf, vertices_at), (jbuf, joints_at) = _padded(vertices.numel(), gpu), _padded(joints.numel(), gpu)
    _c_forward(gpu, kw, shapes, t, c, vertices_at, joints_at, directions=False)
    assert torch.equal(_middle(vbuf, 'K = 0: vertices'), vertices.reshape(-1)) and torch.equal(_middle(jbuf, 'K = 0: joints'), joints.reshape(-1))
    gv, gj = (torch.from_numpy(kw[k]).to(gpu) for k in ('grad_vertices', 'grad_joints'))
    (tbuf, template_at), (cbuf, coefficients_at) = _padded(t.numel(), gpu), _padded(9, gpu)
    _c_backward(gpu, kw, shapes, gv, gj, template_at, coefficients_at, None, 0, directions=False, joint_directions=False)
    assert torch.equal(_middle(tbuf, 'K = 0: grad_template'), grads['d_template'].reshape(-1))
    assert bool((_middle(cbuf, 'K = 0: grad_coefficients') == SENTINEL).all())

    kw = case('j0_b2')
    assert sizes_of(kw)[4] == 0
    vertices, joints, grads = run_fused(kw, gpu)
    assert joints.shape == (2, 0, 3)
    shapes, t, c = _device_operands(kw, gpu)
    B, V, K = sizes_of(kw)[:3]
    (vbuf, vertices_at), (jbuf, joints_at) = _padded(vertices.numel(), gpu), _padded(2 * 4 * 3, gpu)
    _c_forward(gpu, kw, shapes, t, c, vertices_at, joints_at, regressor=False)
    assert torch.equal(_middle(vbuf, 'J = 0: vertices'), vertices.reshape(-1)) and bool((_middle(jbuf, 'J = 0: joints') == SENTINEL).all())
    _c_forward(gpu, kw, shapes, t, c, None, joints_at, regressor=False)                        # nothing to compute: a success without a launch
    assert bool((_middle(jbuf, 'J = 0: joints alone') == SENTINEL).all())
    from dirt_amd import _lib
    nbytes = _lib.load().dirt_blend_scratch_bytes(B, V, K)
    gv = torch.from_numpy(kw['grad_vertices']).to(gpu)
    (tbuf, template_at), (cbuf, coefficients_at), (sbuf, scratch_at) = _padded(t.numel(), gpu), _padded(c.numel(), gpu), _padded(nbytes // 4, gpu)
    _c_backward(gpu, kw, shapes, gv, jbuf[PAD:-PAD], template_at, coefficients_at, scratch_at, nbytes, columns=False, joint_directions=False)
    assert torch.equal(_middle(tbuf, 'J = 0: grad_template'), grads['d_template'].reshape(-1))
    assert torch.equal(_middle(cbuf, 'J = 0: grad_coefficients'), grads['d_coefficients'].reshape(-1))
    _middle(sbuf, 'J = 0: scratch')


@pytest.mark.gpu
@pytest.mark.parametrize('which', POISONS)
def test_non_finite_values_stay_with_their_own_terms(gpu, which):
    """One value of the inputs replaced by +inf or NaN: the outputs whose sum holds a term with it -- by the sparse
    specification: the regressor's non-zeros, k < Ks; computed in poison_variants and held against the specification on the
    CPU by test_the_influence_sets_are_strict_and_those_of_the_specification -- are not finite, NaN or +inf where that is
    determined, and EVERY other element of all four results has the bits of the clean run, which is compared with the
    restatement first.  It bites: a forward that stored, or took a joint from, the dead slots of scene 4's tile differently
    would show in scene 4 or past it; coefficients[1, 6] = NaN and grad_joints = +inf reach joints[1] and d c[4, k >= Ks] if
    the joint term is bounded by K instead of Ks; directions[6, 0, 0] = +inf must give d c[b, 6] = +inf, not NaN: the 191
    dead lanes of the slab read that very quad with a zero gradient, and 0 x inf is NaN without the `live` guard of
    blend_coefficient_sum_kernel; a template backward or a sum kernel that let a NaN of scene 4 into the dead slots' rows
    or into another scene shows in rows 0 to 3."""
    for label, clean, dirty, want in poison_variants(which):
        inside, total = sum(int((w != CLEAN).sum()) for w in want.values()), sum(w.size for w in want.values())
        assert 0 < inside < total, label
        vertices, joints, grads, _ = compare(clean, gpu, label + ' (clean)')
        v2, j2, g2 = run_fused(dirty, gpu)
        for k, a, b in (('vertices', v2, vertices), ('joints', j2, joints), ('d_template', g2['d_template'], grads['d_template']),
                        ('d_coefficients', g2['d_coefficients'], grads['d_coefficients'])):
            check_poisoned(label, k, a, b, want[k])


@pytest.mark.gpu
def test_65535_scenes_exactly(gpu):
    """B = 65535, the documented maximum and exactly the limit of gridDim.y, which the forward's tiles, the template backward
    and the coefficient reduce all use: every sum of most_scenes_case() is exact in float32 in any order (checked on the CPU
    by test_the_largest_batch_is_exact_in_float32), so all four results equal the float64 composition to the bit for every
    one of the 65535 scenes -- a scene left out, computed from another scene's operands or written to another row cannot
    hide under a tolerance."""
    compare(most_scenes_case(), gpu, 'B = %d' % MOST, factor=0.)


@pytest.mark.gpu
def test_a_scenes_gradients_have_the_same_bits_alone_and_in_a_batch(gpu):
    """The backward's sums have the same per-scene order in a tile of four scenes and for a scene alone (the forward has this
    test in tests/test_blend_shapes.py): d_template[b] and d_coefficients[b] of a batch of five equal the gradients of scene
    b run alone, to the bit, with the gradient arriving from both outputs (two slabs, three ranges) and from the joints
    alone (slab 0 alone).  The batch itself is compared with the restatement."""
    for source in ('both', 'joints'):
        kw = gradient_case()
        if source == 'joints':
            kw['grad_vertices'] = None
        _, _, grads, _ = compare(kw, gpu, 'five scenes from %s' % source)
        for b in range(5):
            one = {k: (v[b] if isinstance(v, np.ndarray) and k in ('template', 'coefficients', 'grad_vertices', 'grad_joints') else v) for k, v in kw.items()}
            _, _, alone = run_fused(one, gpu)
            for k in R.GRAD_KINDS:
                assert alone[k].shape == grads[k].shape[1:] and torch.equal(alone[k], grads[k][b]), (source, b, k)
                assert bool(alone[k].abs().max() > 0), (source, b, k)


@pytest.mark.gpu
def test_empty_calls_on_the_gpu(gpu):
    """No scenes (of both operands; of the coefficients with a shared template) and no vertices, through the wrapper on the
    device: nothing is launched, the outputs and the gradients have the shapes of the rule, and what is an empty sum is
    exactly zero."""
    from dirt_amd import blendshapes
    V, K, J = 86, 9, 5
    kw = extra_case('c_one')
    shapes = shapes_of(kw, gpu)
    t, c = (torch.zeros(0, V, 3, device=gpu).requires_grad_(True), torch.zeros(0, K, device=gpu).requires_grad_(True))
    vertices, joints = blendshapes.blend_shapes(t, c, shapes)
    assert vertices.shape == (0, V, 3) and joints.shape == (0, J, 3)
    (vertices.sum() + joints.sum()).backward()
    assert t.grad.shape == (0, V, 3) and c.grad.shape == (0, K)

    t = torch.from_numpy(kw['template']).to(gpu).requires_grad_(True)
    c = torch.zeros(0, K, device=gpu).requires_grad_(True)
    vertices, joints = blendshapes.blend_shapes(t, c, shapes)
    assert vertices.shape == (0, V, 3) and joints.shape == (0, J, 3)
    (vertices.sum() + joints.sum()).backward()
    assert t.grad.shape == (V, 3) and bool((t.grad == 0).all()) and c.grad.shape == (0, K)

    empty = blendshapes.BlendShapes(torch.zeros(K, 0, 3, device=gpu), torch.zeros(J, 0, device=gpu))
    t = torch.zeros(0, 3, device=gpu).requires_grad_(True)
    c = torch.from_numpy(kw['coefficients']).to(gpu).requires_grad_(True)
    vertices, joints = blendshapes.blend_shapes(t, c, empty)
    assert vertices.shape == (0, 3) and joints.shape == (J, 3) and bool((joints == 0).all())
    (vertices.sum() + joints.sum()).backward()
    assert t.grad.shape == (0, 3) and c.grad.shape == (K,) and bool((c.grad == 0).all())
    torch.cuda.synchronize()
