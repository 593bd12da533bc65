"""`shade_gbuffer(..., colors=<tensor>)` (the ALBEDO instantiations of dirt_shade.hip, dirt_shade_albedo_forward / _backward)
against the restatement of tests/shade_reference.py.  The restatement needs no new code: external colours `a` beside a
G-buffer `g` of Cg channels give what `R.compose(np.concatenate([g, a], 1), lights, dict(layout, colors=Cg), ...)` gives --
`out` is the pixels, `d_gbuffer[:, :Cg]` is d gbuffer, `d_gbuffer[:, Cg:]` is d colours, with their masses.

Every comparison is per element, |gpu - ref64| <= 4 x (float32 figure) x (L1 mass of the element's terms), as in
tests/test_shade.py, whose helpers do the comparing.  The float32 figures are those of the float32 composition on THIS file's
random inputs (`tolerance_cases()`), measured on the CPU with `R.measure_f32` and committed below;
test_committed_figures_hold_on_this_files_inputs measures them again.  Produced by

    python -m tests.test_shade_albedo
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import shade_reference as R
from tests import test_shade as T

F32 = {                     # worst |f32 - ref64| / mass of the float32 composition on tolerance_cases(), per kind of result
    'pixels': 5.59e-6, 'd_colors': 5.62e-6,
    'd_normals': 1.55e-4, 'd_positions': 1.54e-4,     # the conditioning of pow(cos, s), as tests/test_shade.py says of its figures
    'd_mask': 7.71e-7, 'd_params': 1.94e-6}
KERNEL = T.KERNEL

# name -> (Cg, where normals / positions / mask sit): the G-buffer has no colour channels
ALAYOUTS = {
    'n3': (3, dict(normals=0, positions=None, mask=None)),         # normals only
    'm0': (4, dict(normals=1, positions=None, mask=0)),            # the mask at channel 0: what oc = -1 would take for a colour
    'm3': (4, dict(normals=0, positions=None, mask=3)),            # ... and the normals there
    'uv6': (6, dict(normals=3, positions=None, mask=0)),           # the textured examples': mask, (u, v), normal; 1-2 hold noise
    'p7': (7, dict(normals=4, positions=1, mask=0)),
    'w257': (257, dict(normals=254, positions=100, mask=30)),      # the normals straddle channel 256 (the copy-out walk's Cg > 256 regime)
}
SPEC_POINT = ('specular_directional', 'diffuse_point')
COUNT_SETS = dict(T.COUNT_SETS)
COUNT_SETS[3] = T.MIXED3
# (parameter gradients, d gbuffer, d colours) wanted: every (PARAMS, GBUF) that ALBEDO instantiates with the colours wanted, and
# the one with both where they are not
WANTED = {'PGC': (True, True, True), 'PC': (True, False, True), 'GC': (False, True, True), 'C': (False, False, True), 'PG': (True, True, False)}
COUNT_VARIANTS = [(n, v) for n in sorted(COUNT_SETS) for v in WANTED]
LAYOUT_LIGHTS = {'n3': T.KINDS[:1] * 2, 'm0': T.KINDS[:1] * 2, 'm3': T.KINDS[:1] * 2, 'uv6': T.KINDS[:1] * 2, 'p7': SPEC_POINT, 'w257': T.MIXED3}
LAYOUT_CASES = [(name, clamp) for name in ALAYOUTS for clamp in (None, (0., 1.))]
SCENE_CASES = [(px, per_scene) for px in (1024, 1025) for per_scene in (False, True)]

CASES = {}
for _n in sorted(COUNT_SETS):
    CASES['lights%d' % _n] = dict(seed=7000 + _n, kinds=COUNT_SETS[_n], double_sided=[bool(k % 2) for k in range(_n)], layout='p7')
for _i, (_name, _clamp) in enumerate(LAYOUT_CASES):
    CASES['%s_%s' % (_name, 'clamp' if _clamp else 'noclamp')] = dict(
        seed=7100 + _i, kinds=LAYOUT_LIGHTS[_name], double_sided=[False, True, False][:len(LAYOUT_LIGHTS[_name])], layout=_name, clamp=_clamp)
for _i, (_px, _per_scene) in enumerate(SCENE_CASES):
    CASES['b3x%d_%s' % (_px, 'per_scene' if _per_scene else 'shared')] = dict(
        seed=7200 + _i, kinds=T.MIXED3, double_sided=[False, True, False], layout='p7', shape={1024: (32, 32), 1025: (25, 41)}[_px], batch=3,
        per_scene=_per_scene)
for _i, _clamp in enumerate((None, (0., 1.))):
    CASES['non_finite_%s' % ('clamp' if _clamp else 'noclamp')] = dict(
        seed=7300 + _i, kinds=T.MIXED3, double_sided=[False, True, False], layout='p7', shape=(300,), clamp=_clamp)
# seeds that were replaced by the first of seed + 50, + 100, ... whose first draw stays under draw_off_kinks' 5 % cap
REPLACED_SEEDS = {}   # (none of the seeds above needed it)
for _name, _seed in REPLACED_SEEDS.items():
    CASES[_name]['seed'] = _seed
_MADE = {}


class Case:
    """tests/test_shade.py's Case with the colours beside the G-buffer: drawn off the kinks as ONE G-buffer of Cg + 3 channels with
    the colours last (the restatement's input), handed to the kernel as its first Cg channels and an image of 3."""

    def __init__(self, seed, kinds, layout, double_sided=True, shape=(1027,), batch=None, per_scene=False, clamp=(0., 1.)):
        rng = np.random.default_rng(seed)
        self.cg, narrow = ALAYOUTS[layout]
        self.layout = dict(narrow)                       # what shade_gbuffer is given, beside colors=<tensor>
        self.wide = dict(narrow, colors=self.cg)         # what the restatement is given
        self.shape = ((batch,) if batch else ()) + tuple(shape)
        self.n = n = int(np.prod(self.shape))
        b = batch if per_scene else None
        self.lights = R.random_lights(rng, kinds, double_sided, batch=b)
        self.lights = [(r[0], r[1], (r[2] / max(1, len(kinds))).astype(np.float32)) + tuple(r[3:]) for r in self.lights]
        vshape = (3,) if b is None else (b, 3)
        cam = rng.standard_normal(vshape)
        self.kw = dict(ambient=rng.uniform(0., 0.3, vshape).astype(np.float32), background=rng.uniform(0., 1., vshape).astype(np.float32),
                       camera_position=(4. * cam / np.linalg.norm(cam, axis=-1, keepdims=True)).astype(np.float32), clamp=clamp)
        self.idx = np.repeat(np.arange(batch), n // batch) if per_scene else None
        both, self.share = R.draw_off_kinks(rng, n, self.cg + 3, self.wide, self.lights, self.kw, scene_index=self.idx)
        self.g, self.a = np.ascontiguousarray(both[:, :self.cg]), np.ascontiguousarray(both[:, self.cg:])
        self.go = rng.standard_normal((n, 3)).astype(np.float32)

    def both(self):
        return np.concatenate([self.g, self.a], 1)

    def reference(self, masses=True, **over):
        return R.compose(over.get('both', self.both()), self.lights, self.wide, grad_out=self.go, scene_index=self.idx, masses=masses, **self.kw)

    def measure(self):
        return (self.both(), self.lights, self.wide, self.kw, self.go, self.idx)


def case_of(name):
    """-> (the Case of CASES[name], its float64 restatement), made once and shared by the tests that need them"""
    if name not in _MADE:
        case = Case(**CASES[name])
        _MADE[name] = (case, case.reference())
    return _MADE[name]


def tolerance_cases():
    """The inputs the float32 figures are measured on: every random input of the comparisons below."""
    for name in CASES:
        yield case_of(name)[0].measure()


def shade(case, dev, g, a, params_grad=True):
    """-> (shade_gbuffer's pixels with every parameter a GPU tensor, {name: parameter})"""
    from dirt_amd import shading
    named = {}

    def leaf(name, x):
        named[name] = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dev).requires_grad_(params_grad)
        return named[name]

    lights = []
    for i, rec in enumerate(case.lights):
        vec, col = leaf('light%d.vector' % i, rec[1]), leaf('light%d.color' % i, rec[2])
        extra = (leaf('light%d.shininess' % i, rec[3]),) if rec[0] == 'specular_directional' else ()
        lights.append((rec[0], vec, col) + extra + (rec[-1],))
    kw = {k: leaf(k, case.kw[k]) for k in ('ambient', 'background', 'camera_position')}
    return shading.shade_gbuffer(g, lights, colors=a, clamp=case.kw['clamp'], **case.layout, **kw), named


def run(case, dev, want=(True, True, True)):
    """-> (pixels, d gbuffer, d colours, {name: parameter gradient}); `want`: (parameters, G-buffer, colours) as leaves"""
    want_p, want_g, want_c = want
    g = torch.from_numpy(case.g).to(dev).reshape(case.shape + (case.cg,)).requires_grad_(want_g)
    a = torch.from_numpy(case.a).to(dev).reshape(case.shape + (3,)).requires_grad_(want_c)
    out, named = shade(case, dev, g, a, want_p)
    out.backward(torch.from_numpy(case.go).to(dev).reshape(out.shape))
    return out, g.grad, a.grad, {k: t.grad for k, t in named.items()}


def close_gbuffer(dg, ref, case, factor, what, rows=slice(None)):
    """d gbuffer attribute by attribute, each with its own figure; every channel no attribute uses must be exactly 0"""
    dg = np.asarray(dg.detach().cpu(), dtype=np.float64).reshape(-1, case.cg)[rows]
    used = np.zeros(case.cg, bool)
    for name, sl in R.attribute_slices(case.layout).items():
        T.close(dg[:, sl], ref['d_gbuffer'][rows, sl], ref['mass_gbuffer'][rows, sl], factor * F32['d_' + name], '%s d_%s' % (what, name))
        used[sl] = True
    assert not dg[:, ~used].any(), what + ': a channel no attribute uses received a gradient'


def check(case, ref, res, what, want=(True, True, True)):
    out, dg, da, dp = res
    want_p, want_g, want_c = want
    cg = case.cg
    T.close(out, ref['out'], ref['mass_out'], KERNEL * F32['pixels'], what + ' pixels')
    if want_g:
        assert dg.shape == case.shape + (cg,)
        close_gbuffer(dg, ref, case, KERNEL, what)
    else:
        assert dg is None
    if want_c:
        assert da.shape == case.shape + (3,)
        T.close(da, ref['d_gbuffer'][:, cg:], ref['mass_gbuffer'][:, cg:], KERNEL * F32['d_colors'], what + ' d_colors')
    else:
        assert da is None
    assert set(dp) == set(ref['d_params'])
    for k, ref_k in ref['d_params'].items():
        if want_p:
            T.close(dp[k], ref_k, ref['mass_params'][k], KERNEL * F32['d_params'], what + ' d_' + k)
        else:
            assert dp[k] is None, k


# ---------------------------------------------------------------------------------------------------------------- CPU tests

def test_shade_gbuffer_refuses_bad_tensor_colours():
    from dirt_amd import shading
    g = torch.zeros(4, 5, 6)

    def check_arguments(colors, normals=3, positions=None, mask=0):
        return shading._check_arguments(g, [], colors, normals, positions, mask, (0., 0., 0.), None, (0., 0., 0.), None)

    for colors, text in (
            (torch.zeros(4, 5, 4), "colors as a tensor must have shape [4, 5, 3] (the G-buffer's [4, 5, 6] with 3 channels), got [4, 5, 4]"),
            (torch.zeros(20, 3), "colors as a tensor must have shape [4, 5, 3] (the G-buffer's [4, 5, 6] with 3 channels), got [20, 3]"),
            (torch.zeros(4, 5, 3, dtype=torch.int32), 'colors as a tensor must be floating-point, got torch.int32'),
            (torch.zeros(4, 5, 3, device='meta'), 'colors is on meta, the G-buffer on cpu'),
            (4., 'colors must be the index of a G-buffer channel, got 4.0'),
            (None, 'colors must be the index of a G-buffer channel, got None'),
            (True, 'colors must be the index of a G-buffer channel, got True')):
        with pytest.raises(ValueError) as e:
            check_arguments(colors)
        assert str(e.value) == text
    # the offsets' first entry is -1, and nothing is reserved for colours: normals and mask may sit anywhere, channel 0 included
    result = check_arguments(torch.zeros(4, 5, 3, dtype=torch.float64))
    assert len(result) == 8 and result[0] == [-1, 3, -1, 0]
    assert check_arguments(torch.zeros(4, 5, 3), normals=0, mask=5)[0] == [-1, 0, -1, 5]
    assert check_arguments(torch.zeros(4, 5, 3), normals=0, positions=3, mask=None)[0] == [-1, 0, 3, -1]
    with pytest.raises(ValueError) as e:
        check_arguments(torch.zeros(4, 5, 3), normals=0, mask=2)
    assert str(e.value) == 'mask (channel 2) overlaps normals (channel 0)'
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        shading.shade_gbuffer(g, [], colors=torch.zeros(4, 5, 3), normals=3)


def test_rows_read_in_place():
    """The rule the colours share with the (u, v) pairs of the texture look-ups: the last axis dense, the pixels a constant stride
    of at least the row's width apart -> the tensor itself and that stride; anything else -> a contiguous copy."""
    from dirt_amd import _stage, texture
    rgba = torch.arange(2 * 3 * 5 * 4, dtype=torch.float32).reshape(2, 3, 5, 4)
    for view, offset in ((rgba[..., :3], 0), (rgba[..., 1:4], 1)):
        src, stride = _stage.rows_in_place(view, 3)
        assert stride == 4 and src.data_ptr() == rgba.data_ptr() + 4 * offset
    dense = torch.zeros(7, 3)
    assert _stage.rows_in_place(dense, 3)[1] == 3 and _stage.rows_in_place(dense, 3)[0] is dense
    g = torch.zeros(6, 7, 10)
    src, stride = _stage.rows_in_place(g[..., 4:7], 3)
    assert stride == 10 and src.data_ptr() == g.data_ptr() + 16
    for copied in (rgba.transpose(1, 2)[..., :3], rgba[:, ::2, :, :3], torch.zeros(3, 7).t()):
        src, stride = _stage.rows_in_place(copied, copied.shape[-1])
        assert src.is_contiguous() and stride == copied.shape[-1] and torch.equal(src, copied)
    uv = g[..., 1:3]
    assert texture._pairs_in_place(uv)[1] == 10 and texture._pairs_in_place(uv)[0].data_ptr() == g.data_ptr() + 4


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def _entry_points(lib, one):
    good = dict(scenes=1, pixels=64, cg=7, cs=3, on=4, op=1, om=0, ps=1, nl=2, kinds=0 | (1 << 2), sided=0, lo=0., hi=1., flags=3)

    def fwd(g=one, c=one, p=one, o=one, **over):
        a = dict(good, **over)
        return lib.dirt_shade_albedo_forward(g, c, p, o, a['scenes'], a['pixels'], a['cg'], a['cs'], a['on'], a['op'], a['om'], a['ps'], a['nl'],
                                             a['kinds'], a['sided'], a['lo'], a['hi'], a['flags'], None)

    def bwd(g=one, c=one, p=one, go=one, gg=one, gc=one, gp=one, scratch=one, nbytes=1 << 20, **over):
        a = dict(good, **over)
        return lib.dirt_shade_albedo_backward(g, c, p, go, gg, gc, gp, scratch, nbytes, a['scenes'], a['pixels'], a['cg'], a['cs'], a['on'], a['op'],
                                              a['om'], a['ps'], a['nl'], a['kinds'], a['sided'], a['lo'], a['hi'], a['flags'], None)

    return fwd, bwd


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    fwd, bwd = _entry_points(lib, one)
    bad = [(dict(scenes=-1), 'negative sizes (scenes=-1 pixels=64)'), (dict(pixels=-5), 'negative sizes (scenes=1 pixels=-5)'),
           (dict(cg=0), '0 G-buffer channels, 1..1024'), (dict(cg=1025), '1025 G-buffer channels, 1..1024'),
           (dict(cs=2), "color_stride=2, a pixel's colour is 3 floats"), (dict(c=None), 'colors is NULL'),
           (dict(kinds=3), 'light 0 has unknown kind 3'), (dict(op=-1), 'light 1 needs positions, the G-buffer has none'),
           (dict(lo=2., hi=1.), 'clamp bounds lo=2 > hi=1'), (dict(ps=2), 'param_scenes=2 is neither 1 nor scenes=1'),
           (dict(on=5), 'normals at channel 5 does not fit in 7 channels'), (dict(om=3), 'mask (channel 3) overlaps positions (channel 1)'),
           (dict(g=None), 'gbuffer / params / out is NULL'), (dict(nl=9), '9 lights, at most 8'),
           (dict(flags=1), 'light 1 is specular and needs a camera position (DIRT_SHADE_HAS_CAMERA)')]
    for over, text in bad:
        assert fwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().decode() == 'dirt_shade_albedo_forward: ' + text
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().decode() == 'dirt_shade_albedo_backward: ' + text.replace('/ out is', '/ grad_out is')
    assert bwd(scratch=None) == _lib.E_INVALID_ARGUMENT and bwd(nbytes=8) == _lib.E_INVALID_ARGUMENT
    assert lib.dirt_last_error().decode() == 'dirt_shade_albedo_backward: scratch is NULL or smaller than dirt_shade_scratch_bytes (8 < 100)'
    # three channels of normals are the smallest G-buffer, the mask may sit at channel 0; zero pixels (or scenes) and "no gradient
    # wanted" are successes that launch nothing, whatever the pointers
    assert fwd(cg=3, on=0, op=-1, om=-1, nl=0, kinds=0, pixels=0) == 0 and fwd(cg=2, on=0, op=-1, om=-1, nl=0, kinds=0, pixels=0) == _lib.E_INVALID_ARGUMENT
    assert lib.dirt_last_error().decode() == 'dirt_shade_albedo_forward: normals at channel 0 does not fit in 2 channels'
    assert fwd(g=None, c=None, p=None, o=None, pixels=0) == 0 and fwd(scenes=0, ps=0) == 0 and lib.dirt_last_error() == b''
    assert bwd(g=None, c=None, p=None, go=None, gg=None, gc=None, gp=None, scratch=None, nbytes=0, pixels=0) == 0
    assert bwd(gg=None, gc=None, gp=None, scratch=None, nbytes=0) == 0 and lib.dirt_last_error() == b''
    assert bwd(g=None, c=None, p=None, go=None, gg=None, gc=None, gp=None) == 0     # nothing wanted: before the pointers are looked at
    assert bwd(gg=None, gp=None, c=None) == _lib.E_INVALID_ARGUMENT                   # the colours' gradient alone still needs the colours
    with pytest.raises(ValueError, match='dirt_shade_albedo_backward: colors is NULL'):
        _lib.check(bwd(c=None))


def test_the_channel_entry_points_still_refuse_no_colour_channels(lib):
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)
    assert lib.dirt_shade_forward(one, one, one, 1, 64, 10, -1, 7, 1, 0, 1, 0, 0, 0, 0., 1., 3, None) == _lib.E_INVALID_ARGUMENT
    assert lib.dirt_last_error().decode() == 'dirt_shade_forward: colors at channel -1 does not fit in 10 channels'
    assert lib.dirt_shade_backward(one, one, one, one, one, one, 1 << 20, 1, 64, 10, -1, 7, 1, 0, 1, 0, 0, 0, 0., 1., 3, None) == _lib.E_INVALID_ARGUMENT
    assert lib.dirt_last_error().decode() == 'dirt_shade_backward: colors at channel -1 does not fit in 10 channels'
    # and a mask at channel 0 beside colours at 1 is what it was
    assert lib.dirt_shade_forward(one, one, one, 1, 0, 7, 1, 4, -1, 0, 1, 0, 0, 0, 0., 1., 1, None) == 0


def test_both_translation_units_are_built_and_declared():
    from dirt_amd import build, _lib
    assert 'dirt_shade.hip' in build.SOURCES and 'dirt_shade_albedo.hip' in build.SOURCES
    assert 'dirt_shade_albedo_forward' in _lib.SYMBOLS and 'dirt_shade_albedo_backward' in _lib.SYMBOLS
    header = open(os.path.join(T.ROOT, 'include', 'dirt_hip.h')).read()
    assert 'int dirt_shade_albedo_forward(' in header and 'int dirt_shade_albedo_backward(' in header


def test_committed_figures_hold_on_this_files_inputs():
    """The float32 composition's own error on every case of this file stays within the committed F32 figures, and under 5 % of
    each case's first draw was rejected (draw_off_kinks asserts it too: a seed that fails it is replaced, REPLACED_SEEDS)."""
    for name in CASES:
        case, _ = case_of(name)
        assert case.share < 0.05, name
        measured = R.measure_f32([case.measure()])
        print(name, ' '.join('%s %.2f' % (k, v / F32[k]) for k, v in measured.items()))
        for k, v in measured.items():
            assert v <= F32[k], '%s %s: committed %.3e, measured on this case %.3e' % (name, k, F32[k], v)


def test_the_cases_hold_what_their_names_say():
    source = open(os.path.join(T.ROOT, 'dirt_amd', 'csrc', 'dirt_shade.hip')).read()
    assert 'constexpr int SHADE_BLOCK = 256;' in source and 'constexpr int SHADE_ITER = 4;' in source
    assert sorted(COUNT_SETS) == list(range(9)) and all(len(v) == n for n, v in COUNT_SETS.items())
    assert all(set(v) == set(T.KINDS) for n, v in COUNT_SETS.items() if n >= 3)
    # every (PARAMS, GBUF) of ALBEDO with the colours wanted, and both without them
    assert {w[:2] for w in WANTED.values() if w[2]} == {(True, True), (True, False), (False, True), (False, False)} and (True, True, False) in WANTED.values()
    for n in COUNT_SETS:
        case, ref = case_of('lights%d' % n)
        assert case.n == 1027 and T.lib_blocks(1027) == 2 and len(case.lights) == n and case.g.shape == (1027, 7) and case.a.shape == (1027, 3)
    for name, clamp in LAYOUT_CASES:
        case, ref = case_of('%s_%s' % (name, 'clamp' if clamp else 'noclamp'))
        assert case.kw['clamp'] == clamp and case.cg == ALAYOUTS[name][0] and bool(R.off_kinks(ref, clamp).all())
        unused = np.ones(case.cg, bool)
        for sl in R.attribute_slices(case.layout).values():
            unused[sl] = False
        assert unused.sum() == {'n3': 0, 'm0': 0, 'm3': 0, 'uv6': 2, 'p7': 0, 'w257': 250}[name]
        assert not unused.any() or bool(np.abs(case.g[:, unused]).min() > 0)                    # noise in every unused channel
    assert ALAYOUTS['m0'][1]['mask'] == 0 and ALAYOUTS['m3'][1]['normals'] == 0 and ALAYOUTS['uv6'][1] == dict(normals=3, positions=None, mask=0)
    assert ALAYOUTS['w257'][1]['normals'] < 256 < ALAYOUTS['w257'][1]['normals'] + 3
    assert {r[0] for r in case_of('p7_clamp')[0].lights} == set(SPEC_POINT)
    assert [case_of('b3x%d_%s' % (px, 'per_scene' if s else 'shared'))[0].shape for px, s in SCENE_CASES] == [(3, 32, 32)] * 2 + [(3, 25, 41)] * 2
    assert T.lib_blocks(1024) == 1 and T.lib_blocks(1025) == 2


def test_scenes_colours_differ_enough_to_show_a_neighbours():
    """The scene cases with the colours of two neighbouring scenes swapped in the restatement: every scene's pixels, and of the
    1025-pixel scenes the last pixel alone (the one a workgroup of one pixel shades), move far past the bound the GPU test
    applies (6e5 to 8e5 x and 9e3 to 3e5 x) -- a kernel that reads scene 0's colours for every scene cannot pass."""
    for px, per_scene in SCENE_CASES:
        case, ref = case_of('b3x%d_%s' % (px, 'per_scene' if per_scene else 'shared'))
        for a, b in ((0, 1), (1, 2)):
            both = case.both()
            rows_a, rows_b = slice(a * px, (a + 1) * px), slice(b * px, (b + 1) * px)
            both[rows_a, case.cg:], both[rows_b, case.cg:] = case.a[rows_b], case.a[rows_a]
            swapped = case.reference(masses=False, both=both)
            for rows in (rows_a, rows_b):
                margin = R.worst_ratio(swapped['out'][rows], ref['out'][rows], ref['mass_out'][rows]) / (KERNEL * F32['pixels'])
                last = slice(rows.stop - 1, rows.stop)
                margin_last = R.worst_ratio(swapped['out'][last], ref['out'][last], ref['mass_out'][last]) / (KERNEL * F32['pixels'])
                print('%d px, scenes %d and %d swapped: pixels move by %.0f x the bound, the last pixel by %.0f x' % (px, a, b, margin, margin_last))
                assert margin > 1000. and (margin_last > 10. or px == 1024)     # (1025: the last pixel is a workgroup of its own)


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('n, variant', COUNT_VARIANTS, ids=['%d-%s' % nv for nv in COUNT_VARIANTS])
def test_light_counts_with_the_wanted_gradients(gpu, n, variant):
    """shade_backward_kernel<NL, PARAMS, GBUF, ALBEDO = true> for every NL and every pattern of wanted gradients it is launched for
    (the colours' alone, <NL, false, false, true>, needs neither the LDS tile, the reduce launch nor scratch), on 1027 pixels: one
    full workgroup and three pixels, two rows for the reduce.  A gradient not wanted comes back None."""
    case, ref = case_of('lights%d' % n)
    check(case, ref, run(case, gpu, WANTED[variant]), '%d lights, %s' % (n, variant), WANTED[variant])


@pytest.mark.gpu
@pytest.mark.parametrize('name, clamp', LAYOUT_CASES, ids=['%s-%s' % (n, 'clamp' if c else 'noclamp') for n, c in LAYOUT_CASES])
def test_layouts_against_the_restatement(gpu, name, clamp):
    """Three channels of normals alone; the mask, then the normals, at channel 0 (where a colour offset of -1 would have put the
    colours' gradient); the textured examples' six channels with noise in (u, v), which comes back as exact zeros; positions
    under a specular and a point light; 257 channels with the normals across channel 256."""
    case, ref = case_of('%s_%s' % (name, 'clamp' if clamp else 'noclamp'))
    check(case, ref, run(case, gpu), name)


@pytest.mark.gpu
@pytest.mark.parametrize('px, per_scene', SCENE_CASES, ids=['%d-%s' % (p, 'per_scene' if s else 'shared') for p, s in SCENE_CASES])
def test_scenes_read_their_own_colours(gpu, px, per_scene):
    case, ref = case_of('b3x%d_%s' % (px, 'per_scene' if per_scene else 'shared'))
    check(case, ref, run(case, gpu), '3 x %d pixels' % px)


@pytest.mark.gpu
def test_strided_colours_are_read_in_place(gpu, monkeypatch):
    """The first and the last three channels of an RGBA image (stride 4; the second 4 bytes off 16-byte alignment): the pointer
    the C ABI receives is the image's own.  A transposed one is copied.  d colours is dense [..., 3] for all of them."""
    from dirt_amd import _stage
    case, ref = case_of('uv6_clamp')
    seen = []
    call = _stage.call

    def spy(function, dev, *arguments, **kw):
        seen.append((function, arguments))
        return call(function, dev, *arguments, **kw)

    monkeypatch.setattr(_stage, 'call', spy)
    lib = __import__('dirt_amd')._lib.load()
    go = torch.from_numpy(case.go).to(gpu)
    for first in (0, 1):
        rgba = torch.full((case.n, 4), 1.e30, device=gpu)
        rgba[:, first:first + 3] = torch.from_numpy(case.a).to(gpu)
        rgba.requires_grad_(True)
        assert rgba.data_ptr() % 16 == 0
        g = torch.from_numpy(case.g).to(gpu).requires_grad_(True)
        del seen[:]
        out, named = shade(case, gpu, g, rgba[:, first:first + 3])
        (d_rgba,) = torch.autograd.grad(out, [rgba], go, retain_graph=True)
        out.backward(go)
        forward = [a for f, a in seen if f is lib.dirt_shade_albedo_forward]
        backward = [a for f, a in seen if f is lib.dirt_shade_albedo_backward]
        assert len(forward) == 1 and forward[0][1] == rgba.data_ptr() + 4 * first and forward[0][7] == 4
        assert len(backward) == 2 and all(a[1] == rgba.data_ptr() + 4 * first and a[12] == 4 for a in backward)
        assert torch.equal(d_rgba, rgba.grad) and not d_rgba[:, 3 - 3 * first].any()
        check(case, ref, (out, g.grad, rgba.grad[:, first:first + 3], {k: t.grad for k, t in named.items()}), 'rgba[..., %d:%d]' % (first, first + 3))
    # [3, N] transposed: the last axis is not dense -> a contiguous copy, the same numbers
    planes = torch.from_numpy(np.ascontiguousarray(case.a.T)).to(gpu).requires_grad_(True)
    g = torch.from_numpy(case.g).to(gpu).requires_grad_(True)
    del seen[:]
    out, named = shade(case, gpu, g, planes.t())
    out.backward(go)
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_albedo_forward]
    assert forward[7] == 3 and forward[1] != planes.data_ptr() and planes.grad.shape == (3, case.n)
    check(case, ref, (out, g.grad, planes.grad.t(), {k: t.grad for k, t in named.items()}), 'transposed colours')


@pytest.mark.gpu
def test_the_same_bits_as_the_channel_path(gpu):
    """The sample's 10-channel G-buffer lit from its own channels 4-6 as a tensor (read in place, stride 10) and as colors=4: both
    instantiations share every expression after the load, so pixels, d normals / positions / mask and every parameter gradient
    are equal bit for bit; d colours is channels 4-6 of the channel path's d gbuffer, which the tensor path leaves exactly zero."""
    from dirt_amd import shading
    case = T.Case(7400, SPEC_POINT, double_sided=[False, True], layout='c10', shape=(1027,))
    go = torch.from_numpy(case.go).to(gpu)
    results = []
    for tensor_colours in (True, False):
        g = torch.from_numpy(case.g).to(gpu).requires_grad_(True)
        c = g[..., 4:7].detach().requires_grad_(True) if tensor_colours else None
        named = {}

        def leaf(name, x):
            named[name] = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(gpu).requires_grad_(True)
            return named[name]

        lights = [(r[0], leaf('light%d.vector' % i, r[1]), leaf('light%d.color' % i, r[2])) +
                  ((leaf('light%d.shininess' % i, r[3]),) if r[0] == 'specular_directional' else ()) + (r[-1],) for i, r in enumerate(case.lights)]
        kw = {k: leaf(k, case.kw[k]) for k in ('ambient', 'background', 'camera_position')}
        out = shading.shade_gbuffer(g, lights, colors=c if tensor_colours else 4, normals=7, positions=1, mask=0, clamp=case.kw['clamp'], **kw)
        out.backward(go)
        results.append((out.detach(), g.grad, c.grad if tensor_colours else None, {k: t.grad for k, t in named.items()}))
    (oa, ga, ca, pa), (ob, gb, _, pb) = results
    assert torch.equal(oa, ob) and bool(oa.abs().max() > 0)
    for name, sl in (('mask', slice(0, 1)), ('positions', slice(1, 4)), ('normals', slice(7, 10))):
        assert torch.equal(ga[:, sl], gb[:, sl]) and bool(gb[:, sl].abs().max() > 0), name
    assert ca.shape == (1027, 3) and torch.equal(ca, gb[:, 4:7]) and bool(ca.abs().max() > 0)
    assert not ga[:, 4:7].any()
    for k in pb:
        assert torch.equal(pa[k], pb[k]), k


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_backward_is_reentrant(gpu):
    case, _ = case_of('lights3')
    (o1, g1, a1, p1), (o2, g2, a2, p2) = run(case, gpu), run(case, gpu)
    assert torch.equal(o1, o2) and torch.equal(g1, g2) and torch.equal(a1, a2) and bool(a1.abs().max() > 0)
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k      # fixed-order sums, no atomics
    # backward twice over one forward (retain_graph=True, as _RasteriseDeferred.backward calls it)
    g = torch.from_numpy(case.g).to(gpu).requires_grad_(True)
    a = torch.from_numpy(case.a).to(gpu).requires_grad_(True)
    out, named = shade(case, gpu, g, a)
    inputs = [g, a] + list(named.values())
    go = torch.from_numpy(case.go).to(gpu)
    first = torch.autograd.grad(out, inputs, go, retain_graph=True)
    second = torch.autograd.grad(out, inputs, go, retain_graph=True)
    assert all(torch.equal(x, y) for x, y in zip(first, second)) and first[1].data_ptr() != second[1].data_ptr()
    assert torch.equal(first[1], a1)


@pytest.mark.gpu
@pytest.mark.parametrize('clamp', [None, (0., 1.)], ids=['noclamp', 'clamp'])
def test_non_finite_colours_stay_in_their_pixel(gpu, clamp):
    """A NaN and an inf in one pixel's colour: its own pixel, d gbuffer row and d colours row are non-finite exactly where the
    composition's are, every other pixel's are what they are without them, and the parameter gradients are non-finite where the
    restatement's are (`close` compares the places) and within the bound elsewhere."""
    name = 'non_finite_%s' % ('clamp' if clamp else 'noclamp')
    case, clean = case_of(name)
    victim = 137
    spoilt = Case(**CASES[name])
    spoilt.a[victim, 0], spoilt.a[victim, 2] = float('nan'), float('inf')
    assert np.array_equal(np.delete(spoilt.a, victim, 0), np.delete(case.a, victim, 0)) and np.array_equal(spoilt.g, case.g)
    ref = spoilt.reference()
    out, dg, da, dp = run(spoilt, gpu)
    out, cg = out.detach(), case.cg
    others = np.arange(case.n) != victim
    T.close(out[others], clean['out'][others], clean['mass_out'][others], KERNEL * F32['pixels'], 'other pixels')
    close_gbuffer(dg, clean, case, KERNEL, 'other pixels', rows=others)
    T.close(da[others], clean['d_gbuffer'][others, cg:], clean['mass_gbuffer'][others, cg:], KERNEL * F32['d_colors'], 'other pixels d_colors')
    assert np.array_equal(np.isfinite(out[victim].cpu().numpy()), np.isfinite(ref['out'][victim].numpy()))
    assert not np.isfinite(out[victim].cpu().numpy()).all()
    assert np.array_equal(np.isfinite(dg[victim].cpu().numpy()), np.isfinite(ref['d_gbuffer'][victim, :cg].numpy()))
    assert np.array_equal(np.isfinite(da[victim].cpu().numpy()), np.isfinite(ref['d_gbuffer'][victim, cg:].numpy()))
    for k, ref_k in ref['d_params'].items():
        T.close(dp[k], ref_k, ref['mass_params'][k], KERNEL * F32['d_params'], 'd_' + k)


@pytest.mark.gpu
@pytest.mark.parametrize('pixels', [1, 255, 256, 257, 1027])
def test_the_c_abi_writes_nothing_outside_its_outputs(gpu, lib, pixels):
    """dirt_shade_albedo_forward / _backward with `out`, `grad_colors` and `grad_gbuffer` inside buffers filled with a sentinel: the
    margins on both sides are intact, every element between them is written, and the results are the wrapper's bit for bit."""
    from dirt_amd import rasterise_ops as ops, shading
    margin, sentinel, cg, scenes = 2048, -7777.25, 6, 2
    gen = torch.Generator(device='cpu').manual_seed(pixels)
    g = torch.rand(scenes, pixels, cg, generator=gen).to(gpu)
    rgba = torch.rand(scenes, pixels, 4, generator=gen).to(gpu)
    go = torch.randn(scenes, pixels, 3, generator=gen).to(gpu)
    block = torch.tensor([[.4, .4, .4, 0., 0., .3, 0., 0., 0., .6, -.2, -.7, .6, .5, .4, 0., 0.]], device=gpu)
    n = scenes * pixels
    guarded = {k: torch.full((2 * margin + n * w,), sentinel, device=gpu) for k, w in (('out', 3), ('gc', 3), ('gg', cg))}
    inner = {k: t[margin:t.numel() - margin] for k, t in guarded.items()}
    gp = torch.full((1, 17), sentinel, device=gpu)
    nbytes = lib.dirt_shade_scratch_bytes(scenes, pixels, 1)
    scratch = torch.empty(nbytes // 4, device=gpu)
    stream = ops._stream_handle(gpu)
    tail = (scenes, pixels, cg, 4, 3, -1, 0, 1, 1, 0, 1, 0., 1., 1, stream)
    with ops._on_device(gpu):
        rc = lib.dirt_shade_albedo_forward(g.data_ptr(), rgba.data_ptr() + 4, block.data_ptr(), inner['out'].data_ptr(), *tail)
        assert rc == 0, lib.dirt_last_error()
        rc = lib.dirt_shade_albedo_backward(g.data_ptr(), rgba.data_ptr() + 4, block.data_ptr(), go.data_ptr(), inner['gg'].data_ptr(),
                                            inner['gc'].data_ptr(), gp.data_ptr(), scratch.data_ptr(), nbytes, *tail)
        assert rc == 0, lib.dirt_last_error()
    torch.cuda.synchronize()
    for k, t in guarded.items():
        assert bool((t[:margin] == sentinel).all()) and bool((t[-margin:] == sentinel).all()), k + ': written outside'
        assert not bool((inner[k] == sentinel).any()), k + ': not written whole'
    assert not bool((gp == sentinel).any())
    gl, cl = g.clone().requires_grad_(True), rgba[..., 1:4].clone().requires_grad_(True)
    direction = block[0, 9:12].clone().requires_grad_(True)
    out = shading.shade_gbuffer(gl.reshape(scenes, pixels, 1, cg), [shading.diffuse_directional_light(direction, (.6, .5, .4), True)],
                                colors=cl.reshape(scenes, pixels, 1, 3), normals=3, mask=0, ambient=(.4, .4, .4), background=(0., 0., .3))
    out.backward(go.reshape(out.shape))
    assert torch.equal(out.detach().reshape(-1), inner['out']) and torch.equal(gl.grad.reshape(-1), inner['gg'])
    assert torch.equal(cl.grad.reshape(-1), inner['gc']) and torch.equal(direction.grad, gp[0, 9:12])


def _textured_fused_shader(gbuffer, texture, light_direction):
    return T._load_example('textured_fused').shader_fn(gbuffer, texture, light_direction)


def _element_rule(a, b, what):
    """test_rasterise_deferred_with_the_fused_shader's rule for gradients no mass is at hand for: elements agree at 1e-3 relative or
    are both below 1e-7; the share excluded is capped at 1 % per tensor, and the tensor is not all zero"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    agree = ((a - b).abs() <= 1e-3 * torch.maximum(a.abs(), b.abs())) | ((a.abs() < 1e-7) & (b.abs() < 1e-7))
    share = 1. - float(agree.double().mean())
    print('%s: %d of %d elements excluded' % (what, int((~agree).sum()), agree.numel()))
    assert share <= 0.01, (what, share)
    assert bool(a.abs().max() > 0), what


TEXTURED_WIDE = dict(colors=6, normals=3, positions=None, mask=0)


def _textured_restatement(gbuffer, unlit, light, pixels):
    """the restatement of the textured examples' shader on a rasterised G-buffer with the sampled colours appended, under the
    gradient of mean(pixels ** 2)"""
    both = np.concatenate([gbuffer.reshape(-1, 6).cpu().numpy(), unlit.reshape(-1, 3).cpu().numpy()], 1)
    go = (2. / pixels.numel()) * pixels.reshape(-1, 3).cpu().numpy()
    return R.compose(both, [('diffuse_directional', light.cpu().numpy(), (.6, .6, .6), True)], TEXTURED_WIDE, ambient=(.4, .4, .4),
                     background=(0., 0., .3), clamp=None, grad_out=go)


@pytest.mark.gpu
def test_rasterise_deferred_with_the_textured_fused_shader(gpu):
    """End to end on the cube of examples/textured.py: rasterise_deferred with the shader of examples/textured_fused.py against the
    same call with examples/textured.py's torch shader.  Pixels and the light's gradient by the mass rule at 5 x the float32
    figures (two float32 implementations of one composition: 1 x and 4 x); the texture's gradient has been through the look-up's
    backward and the vertices' through the rasteriser's, where no mass is at hand: the element rule."""
    import dirt_amd
    from dirt_amd import texture as tex
    ex = T._load_example('textured')
    results = []
    for fn in (ex.shader_fn, _textured_fused_shader):
        vertices, uvs, faces = (torch.from_numpy(a).to(gpu) for a in ex.build_cube())
        vertices.requires_grad_(True)
        texture = torch.from_numpy(ex.checker_texture()).to(gpu).requires_grad_(True)
        light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=gpu), dim=0).requires_grad_(True)
        clip, attributes = ex.geometry(vertices, uvs, faces)
        background = torch.zeros([ex.frame_height, ex.frame_width, 6], device=gpu)
        pixels = dirt_amd.rasterise_deferred(vertices=clip, vertex_attributes=attributes, faces=faces, background_attributes=background,
                                             shader_fn=fn, shader_additional_inputs=[texture, light])
        (pixels ** 2).mean().backward()
        results.append((pixels.detach(), vertices.grad, texture.grad, light.grad))
    gbuffer = dirt_amd.rasterise(background, clip.detach(), attributes.detach(), faces)
    unlit = tex.sample_texture_uv(texture.detach(), gbuffer[..., 1:3])
    (pa, va, ta, la), (pb, vb, tb, lb) = results
    ref = _textured_restatement(gbuffer, unlit, light.detach(), pa)
    T.close(pb.reshape(-1, 3), pa.reshape(-1, 3).cpu().numpy(), ref['mass_out'], 5 * F32['pixels'], 'textured: pixels')
    T.close(lb[None], la[None].cpu().numpy(), ref['mass_params']['light0.vector'], 5 * F32['d_params'], 'textured: d_light')
    _element_rule(ta, tb, 'textured: d_texture')
    _element_rule(va, vb, 'textured: d_vertices')


@pytest.mark.gpu
def test_rasterise_batch_deferred_with_a_texture_per_scene(gpu):
    """Two views, each with its own texture looked up with the trilinear filter (mask and (u, v) read in place from the batched
    G-buffer), lit from the look-up's output: against the shader of examples/textured_batch.py."""
    import dirt_amd
    from dirt_amd import shading, texture as tex
    ex = T._load_example('textured_batch')
    height, width = 120, 160

    def fused(gbuffer, textures, light_direction):
        unlit = tex.sample_texture_uv_batch(textures, gbuffer[..., 1:3], filter='trilinear', mask=gbuffer[..., 0])
        return shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(light_direction, (.6, .6, .6), True)], colors=unlit, normals=3,
                                     mask=0, ambient=(.4, .4, .4), background=(0., 0., .3), clamp=None)

    vertices, uvs, faces = (torch.from_numpy(a).to(gpu) for a in ex.textured.build_cube())
    clip, attributes, faces_b = ex.geometry(vertices, uvs, faces, [0.6, 1.1], height, width)
    background = torch.zeros([2, height, width, 6], device=gpu)
    results = []
    for fn in (ex.shader_fn, fused):
        textures = torch.from_numpy(ex.target_textures(2)).to(gpu).requires_grad_(True)
        light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=gpu), dim=0).requires_grad_(True)
        pixels = dirt_amd.rasterise_batch_deferred(vertices=clip, vertex_attributes=attributes, faces=faces_b, background_attributes=background,
                                                   shader_fn=fn, shader_additional_inputs=[textures, light])
        (pixels ** 2).mean().backward()
        results.append((pixels.detach(), textures.grad, light.grad))
    gbuffer = dirt_amd.rasterise_batch(background, clip, attributes, faces_b)
    unlit = tex.sample_texture_uv_batch(textures.detach(), gbuffer[..., 1:3], filter='trilinear', mask=gbuffer[..., 0])
    (pa, ta, la), (pb, tb, lb) = results
    ref = _textured_restatement(gbuffer, unlit, light.detach(), pa)
    T.close(pb.reshape(-1, 3), pa.reshape(-1, 3).cpu().numpy(), ref['mass_out'], 5 * F32['pixels'], 'batch: pixels')
    T.close(lb[None], la[None].cpu().numpy(), ref['mass_params']['light0.vector'], 5 * F32['d_params'], 'batch: d_light')
    _element_rule(ta, tb, 'batch: d_textures')
    assert bool(ta[0].abs().max() > 0) and bool(ta[1].abs().max() > 0) and not torch.equal(ta[0], ta[1])


@pytest.mark.gpu
def test_graphed_step_captures_a_textured_fused_loss(gpu):
    """A GraphedStep whose loss looks a texture up at two channels of the rasterised frame and lights the result as tensor colours
    captures -- neither call makes a host synchronisation -- and its replay returns the eager loss."""
    import dirt_amd
    from dirt_amd import shading, texture as tex
    from tests import scenes
    s = scenes.rand_scene(200, 96, 128, 10, 41, 0.05, 0.3)
    bg, v, vc, f = (torch.from_numpy(s[k][None].copy()).to(gpu) for k in ('background', 'vertices', 'vertex_colors', 'faces'))
    texture = torch.from_numpy(T._load_example('textured').checker_texture(64)).to(gpu)
    direction = torch.tensor([0.6, -0.64, -0.48], device=gpu)
    lights = [shading.diffuse_directional_light(direction, (.6, .6, .6), True),
              shading.specular_directional_light(direction, (1., 1., 1.), 6., False)]

    def loss_fn(px):
        unlit = tex.sample_texture_uv(texture, px[..., 1:3])
        return (shading.shade_gbuffer(px, lights, colors=unlit, normals=7, positions=4, mask=0, ambient=(.2, .2, .2), background=(0., 0., .3),
                                      camera_position=(0.5, 1.5, 3.)) ** 2).mean()

    step = dirt_amd.GraphedStep(bg, v, vc, f, loss_fn=loss_fn)
    for _ in range(2):
        loss, (gb, gv, gvc) = step()
    leaves = [t.detach().clone().requires_grad_(True) for t in (bg, v, vc)]
    eager = loss_fn(dirt_amd.rasterise_batch(leaves[0], leaves[1], leaves[2], f))
    eager.backward()
    torch.cuda.synchronize()
    assert float((loss - eager).detach().abs()) <= 1e-6 * float(eager.detach().abs())
    assert bool(gb.abs().max() > 0) and bool(gvc.abs().max() > 0)
    agree = (gb - leaves[0].grad).abs() <= 1e-4 * torch.maximum(gb.abs(), leaves[0].grad.abs()) + 1e-9   # (the look-up's d uv: float atomics)
    assert float(agree.float().mean()) >= 0.99


@pytest.mark.gpu
def test_the_fused_example_renders_the_textured_examples_image(gpu):
    """examples/textured_fused.py runs; its image is examples/textured.py's to one 8-bit level on every pixel (tests/test_gpu_fullsize.py
    demands every pixel of the textured example); the losses of its descent on the texture fall."""
    ex, fused = T._load_example('textured'), T._load_example('textured_fused')
    image, losses = fused.main(steps=4, device=gpu, quiet=True)
    vertices, uvs, faces = (torch.from_numpy(a).to(gpu) for a in ex.build_cube())
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=gpu), dim=0)
    want = ex.render(vertices, uvs, faces, torch.from_numpy(ex.checker_texture()).to(gpu), light)
    assert image.shape == want.shape == (ex.frame_height, ex.frame_width, 3)
    assert bool(((image - want).abs() <= 1. / 255.).all())
    covered = (want - torch.tensor([0., 0., 0.3], device=gpu)).abs().sum(-1) > 1e-6
    assert 0.1 < float(covered.float().mean()) < 0.7
    assert len(losses) == 4 and bool(np.all(np.diff(losses) < 0.)) and losses[-1] > 0.


if __name__ == '__main__':
    print(R.measure_f32(tolerance_cases()))
