"""`dirt_amd.shading.shade_gbuffer` (dirt_shade.hip) against the restatement of tests/shade_reference.py: the functions of
dirt_amd/lighting.py composed on the CPU in float64, gradients by torch's autograd.  Every comparison is per element,
|gpu - ref64| <= tol * (L1 mass of the element's terms) (+ float32's underflow floor, shade_reference.UNDERFLOW_FLOOR); an element of zero mass must equal the reference exactly;
non-finite values must sit in the same places.

The tolerances are measured, not chosen: the float32 composition (the same lighting functions, CPU, float32, torch
autograd -- the implementation users had before the kernel) is run on `tolerance_cases()`, the inputs of the tests below,
and its worst |f32 - ref64| / mass per kind of result is F32_*; the kernel, which may reorder a pixel's sums and use the
hardware's reciprocal, gets 4 x that.  Produced by

    python -m tests.shade_reference
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import shade_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32_PIXELS = 7.04e-6       # worst |f32 - ref64| / mass of the float32 composition on tolerance_cases(): pixels
F32_D_GBUFFER = {          # ... d gbuffer, by attribute.  The mass counts the two halves of d (t / |t|) / d t and of
    'colors': 7.11e-6,     # d ((n . l) n) / d n apart (shade_reference._SplitTorch): they cancel at a specular highlight.  What is
    'normals': 2.89e-4,    # left in the normals' and positions' figures is the conditioning of pow(cos, s): the cosine's rounding,
    'positions': 2.89e-4,  # relative to a small cosine, times s - 1 (up to 31 here); both are set by the same pixels.
    'mask': 1.71e-6}
F32_D_PARAMS = 9.19e-7     # ... parameter gradients
KERNEL = 4                 # the kernel's allowance over the float32 composition

KINDS = ('diffuse_directional', 'specular_directional', 'diffuse_point')
LAYOUTS = {   # name -> (Cg, layout): 9 without a mask, the sample's 10, 13 and 16 with the attributes in shuffled order
    'c9': (9, dict(colors=0, normals=3, positions=6, mask=None)),
    'c10': (10, dict(R.SAMPLE_LAYOUT)),
    'c13': (13, dict(colors=9, normals=1, positions=5, mask=4)),
    'c16': (16, dict(colors=12, normals=2, positions=7, mask=15)),
    # wider than 16 (EXTRA_CASES): the backward's copy-out walks (pixel, channel) in steps of (256 / Cg, 256 % Cg) -- Cg < 256,
    # Cg == 256 and Cg > 256 are three regimes -- and its s_src fill loop takes a second turn above 256 channels
    'c17': (17, dict(colors=14, normals=3, positions=8, mask=0)),              # the mask first, colours in the last three channels
    'c255': (255, dict(colors=100, normals=252, positions=7, mask=50)),
    'c256': (256, dict(colors=253, normals=0, positions=128, mask=200)),
    'c257': (257, dict(colors=10, normals=254, positions=100, mask=30)),       # the normals straddle channel 256, in the last three
    'c1024': (1024, dict(colors=600, normals=1020, positions=255, mask=1023)),  # the positions straddle channel 256; the mask last
    # without positions: the smallest legal layouts, and one with five channels no attribute uses
    'c6': (6, dict(colors=0, normals=3, positions=None, mask=None)),
    'c7': (7, dict(colors=4, normals=0, positions=None, mask=3)),
    'c12': (12, dict(colors=2, normals=7, positions=None, mask=11)),
}


def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Case:
    """Inputs of one comparison: a G-buffer whose pixels stay off the kinks, lights, the other parameters, grad_out."""

    def __init__(self, seed, kinds, double_sided=True, layout='c10', shape=(4099,), batch=None, per_scene=False, mask=True,
                 clamp=(0., 1.), band=None):
        rng = np.random.default_rng(seed)
        self.cg, layout = LAYOUTS[layout]
        self.layout = dict(layout)
        if not mask:
            self.layout['mask'] = None
        self.shape = ((batch,) if batch else ()) + tuple(shape)
        n = int(np.prod(self.shape))
        b = batch if per_scene else None
        self.lights = R.random_lights(rng, kinds, double_sided, batch=b)
        # keep a good share of the pixels inside the clamp: the lights' colours share the range
        self.lights = [(r[0], r[1], (r[2] / max(1, len(kinds))).astype(np.float32)) + tuple(r[3:]) for r in self.lights]
        vshape = (3,) if b is None else (b, 3)
        cam = rng.standard_normal(vshape)
        self.kw = dict(ambient=rng.uniform(0., 0.3, vshape).astype(np.float32), background=rng.uniform(0., 1., vshape).astype(np.float32),
                       camera_position=(4. * cam / np.linalg.norm(cam, axis=-1, keepdims=True)).astype(np.float32), clamp=clamp)
        self.idx = np.repeat(np.arange(batch), n // batch) if per_scene else None
        self.n = n
        self.band = band   # (first pixel, pixels): the restatement runs on this part only; grad_out is zero elsewhere
        if band is None:
            self.g, self.share = R.draw_off_kinks(rng, n, self.cg, self.layout, self.lights, self.kw, scene_index=self.idx)
            self.go = rng.standard_normal((n, 3)).astype(np.float32)
        else:
            self.g = R.random_gbuffer(rng, n, self.cg, self.layout)
            lo, cnt = band
            self.g[lo:lo + cnt], self.share = R.draw_off_kinks(rng, cnt, self.cg, self.layout, self.lights, self.kw)
            self.go = np.zeros((n, 3), np.float32)
            self.go[lo:lo + cnt] = rng.standard_normal((cnt, 3))

    def reference(self, dtype=torch.float64, masses=True):
        lo, cnt = self.band if self.band is not None else (0, self.n)
        return R.compose(self.g[lo:lo + cnt], self.lights, self.layout, grad_out=self.go[lo:lo + cnt], scene_index=self.idx, dtype=dtype,
                         masses=masses, **self.kw)

    def measure(self):
        lo, cnt = self.band if self.band is not None else (0, self.n)
        return (self.g[lo:lo + cnt], self.lights, self.layout, self.kw, self.go[lo:lo + cnt], self.idx)


MIXED3 = ('diffuse_directional', 'specular_directional', 'diffuse_point')
MIXED8 = MIXED3 + ('specular_directional', 'diffuse_point', 'diffuse_directional', 'specular_directional', 'diffuse_directional')
LIGHT_SETS = {'dd': KINDS[:1], 'sd': KINDS[1:2], 'dp': KINDS[2:], 'mixed3': MIXED3, 'mixed8': MIXED8}

LIGHT_CASES = [(name, ds, mask, clamp) for name in LIGHT_SETS for ds in (False, True) for mask in (False, True) for clamp in (None, (0., 1.))]
SHAPE_CASES = {
    'c9': dict(layout='c9'), 'c13': dict(layout='c13'), 'c16': dict(layout='c16'),
    '1x1': dict(shape=(1, 1)), '1x257': dict(shape=(1, 257)), '33x17': dict(shape=(33, 17)), '640x480': dict(shape=(480, 640)),
    'batch_shared': dict(shape=(33, 47), batch=3), 'batch_per_scene': dict(shape=(33, 47), batch=3, per_scene=True),
    'batch_per_scene_large': dict(shape=(70, 61), batch=2, per_scene=True, layout='c16'),
}


def light_case(name, ds, mask, clamp):
    seed = 1000 + 16 * list(LIGHT_SETS).index(name) + 8 * ds + 4 * mask + 2 * (clamp is not None)
    sided = ds if name != 'mixed8' else [bool((k + ds) % 2) for k in range(8)]   # mixed sidedness in the 8-light set
    return Case(seed, LIGHT_SETS[name], double_sided=sided, mask=mask, clamp=clamp)


def shape_case(name):
    return Case(2000 + list(SHAPE_CASES).index(name), MIXED3, double_sided=[False, True, False], **SHAPE_CASES[name])


def band_case():
    return Case(3000, MIXED3, double_sided=[False, False, True], layout='c16', shape=(2048, 2048), band=(1000 * 2048 + 512, 64 * 2048))


def non_finite_case(clamp):
    return Case(4000, MIXED3, double_sided=[False, True, False], shape=(300,), clamp=clamp)


# Random inputs added after the F32_* figures were measured: not part of tolerance_cases(); the float32 composition stays within
# the committed figures on them (test_extra_cases_stay_within_the_committed_figures), so the kernel's bound rests on the same
# ground.  name -> the arguments of Case, the seed first.  A flat frame of 1027 pixels is one full backward workgroup (1024
# pixels) and a second with three, so the reduce adds two rows; 259 pixels are a full pass of 256 and three more.
COUNT_SETS = {0: (), 1: KINDS[1:2], 2: ('specular_directional', 'diffuse_point'), 4: MIXED8[:4], 5: MIXED8[:5], 6: MIXED8[:6], 7: MIXED8[:7],
              8: MIXED8}      # every set of three or more lights holds all three kinds
WANTED = {'both': (True, True), 'params': (True, False), 'gbuffer': (False, True)}     # (parameter gradients, d gbuffer)
COUNT_VARIANTS = [(n, v) for n in COUNT_SETS for v in WANTED if v != 'both' or n not in (1, 8)]   # 1 and 8 lights with both: LIGHT_CASES
WIDE = ('c17', 'c255', 'c256', 'c257', 'c1024')
EXTRA_CASES = {}
for _n, _kinds in COUNT_SETS.items():
    EXTRA_CASES['lights%d' % _n] = dict(seed=5000 + _n, kinds=_kinds, double_sided=[bool(k % 2) for k in range(_n)], shape=(1027,))
for _i, _name in enumerate(WIDE):
    EXTRA_CASES[_name] = dict(seed=5100 + _i, kinds=MIXED3, double_sided=[False, True, False], layout=_name, shape=(259,) if _name == 'c1024' else (1027,))
for _i, (_name, _n, _clamp) in enumerate((l, n, c) for l in ('c6', 'c7', 'c12') for n in (1, 3) for c in (None, (0., 1.))):
    EXTRA_CASES['%s_dd%d_%s' % (_name, _n, 'clamp' if _clamp else 'noclamp')] = dict(
        seed=5200 + _i, kinds=KINDS[:1] * _n, double_sided=[False, True, False][:_n], layout=_name, shape=(1027,), clamp=_clamp)
for _i, (_px, _per_scene) in enumerate((p, s) for p in (1024, 1025) for s in (False, True)):   # a backward workgroup never spans two scenes
    EXTRA_CASES['b3x%d_%s' % (_px, 'per_scene' if _per_scene else 'shared')] = dict(
        seed=5300 + _i, kinds=MIXED3, double_sided=[False, True, False], shape={1024: (32, 32), 1025: (25, 41)}[_px], batch=3, per_scene=_per_scene)
# seeds that were replaced (by the first of seed + 50, + 100 that held), and what the first seed gave
for _name, _seed in (('lights0', 5050),              # 5000: 8.2 % of the first draw rejected (an ambient of 0.006 keeps dark pixels at the clamp's edge)
                     ('lights8', 5058),              # 5008: float32's own parameter gradients at 1.15 x F32_D_PARAMS
                     ('c255', 5151),                 # 5101: ... at 1.02 x
                     ('c1024', 5154),                # 5104: ... at 1.89 x
                     ('b3x1025_per_scene', 5353)):   # 5303: ... at 1.14 x
    EXTRA_CASES[_name]['seed'] = _seed
NO_POSITIONS = [k for k in EXTRA_CASES if k[:2] in ('c6', 'c7') or k.startswith('c12')]
BOUNDARY = [k for k in EXTRA_CASES if k.startswith('b3x')]
SAME_BITS = ('c1024', 'lights7')
_EXTRA = {}


def extra_case(name):
    """-> (the Case of EXTRA_CASES[name], its float64 restatement), made once and shared by the tests that need them"""
    if name not in _EXTRA:
        kw = dict(EXTRA_CASES[name])
        case = Case(kw.pop('seed'), kw.pop('kinds'), **kw)
        _EXTRA[name] = (case, case.reference())
    return _EXTRA[name]


def sample_frame(seed, n):
    """A frame of the sample's layout under the sample's lights, off the kinks -> (gbuffer, lights, kw, grad_out, view, light).
    No uncovered pixels: the sample's background has two channels exactly at the clamp's lower edge."""
    ex = _load_example('deferred')
    rng = np.random.default_rng(seed)
    view = ex.matrices.compose(ex.matrices.translation(torch.tensor([0., -1.5, -3.5])), ex.matrices.rodrigues(torch.tensor([-0.3, 0., 0.])))
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5]), dim=0)
    lights, kw = R.sample_lights(light.numpy(), torch.linalg.inv(view)[3, :3].numpy())
    g, _ = R.draw_off_kinks(rng, n, 10, R.SAMPLE_LAYOUT, lights, kw, covered=0.9)
    return g, lights, kw, rng.standard_normal((n, 3)).astype(np.float32), view, light


def tolerance_cases():
    """The inputs the float32 figures are measured on: every random input of the comparisons below -- the light and shape
    cases, the 2048 x 2048 frame by its band, the non-finite test's frame before its pixel is spoilt, and the two frames of the
    sample's layout.  The hand-made kink pixels are not part: they are a few exactly representable values."""
    for args in LIGHT_CASES:
        yield light_case(*args).measure()
    for name in SHAPE_CASES:
        yield shape_case(name).measure()
    yield band_case().measure()
    for clamp in (None, (0., 1.)):
        yield non_finite_case(clamp).measure()
    for seed, n in ((5, 5000), (6, 480 * 640)):
        g, lights, kw, go, _, _ = sample_frame(seed, n)
        yield (g, lights, R.SAMPLE_LAYOUT, kw, go, None)


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
    err = np.maximum(err - R.UNDERFLOW_FLOOR, 0.)   # float32's underflow, not the kernel's error (tests/shade_reference.py)
    ratio = float((err[pos] / mass[pos]).max()) if pos.any() else 0.
    print('%-60s worst |gpu - ref64| / mass = %.3e (tol %.3e)' % (what, ratio, tol))
    assert ratio <= tol, '%s: |gpu - ref64| / mass = %.3e > %.3e at element %d' % (what, ratio, tol, int(np.argmax(np.where(pos, err / np.where(pos, mass, 1.), 0.))))
    return ratio


def close_gbuffer(got, ref, mass, layout, factor, what):
    """d gbuffer attribute by attribute, each with its own measured figure; the channels no attribute uses must be exactly 0"""
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64).reshape(np.shape(ref))
    ref, mass = np.asarray(ref, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    used = np.zeros(ref.shape[-1], bool)
    for name, sl in R.attribute_slices(layout).items():
        close(got[:, sl], ref[:, sl], mass[:, sl], factor * F32_D_GBUFFER[name], '%s d_%s' % (what, name))
        used[sl] = True
    assert not got[:, ~used].any(), what + ': a channel no attribute uses received a gradient'


def run_fused(case, dev, g=None, grad=True, params_grad=True, g_grad=True):
    """-> (out, d gbuffer or None, {name: gradient}) of shade_gbuffer with every parameter a GPU tensor"""
    from dirt_amd import shading
    if g is None:
        g = torch.from_numpy(case.g).to(dev).reshape(case.shape + (case.cg,))
    g = g.detach().requires_grad_(g_grad)
    named = {}

    def T(name, x):
        named[name] = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dev).requires_grad_(params_grad)
        return named[name]

    lights = []
    for i, rec in enumerate(case.lights):
        vec, col = T('light%d.vector' % i, rec[1]), T('light%d.color' % i, rec[2])
        extra = (T('light%d.shininess' % i, rec[3]),) if rec[0] == 'specular_directional' else ()
        lights.append((rec[0], vec, col) + extra + (rec[-1],))
    kw = {k: T(k, case.kw[k]) for k in ('ambient', 'background', 'camera_position')}
    out = shading.shade_gbuffer(g, lights, clamp=case.kw['clamp'], **case.layout, **kw)
    if not grad:
        return out, None, named
    out.backward(torch.from_numpy(case.go).to(dev).reshape(out.shape))
    return out, g.grad, {k: t.grad for k, t in named.items()}


def compare(case, dev, what, g=None):
    ref = case.reference()
    out, dg, dp = run_fused(case, dev, g=g)
    lo, cnt = case.band if case.band is not None else (0, case.n)
    out, dg = out.reshape(-1, 3), dg.reshape(-1, case.cg)
    close(out[lo:lo + cnt], ref['out'], ref['mass_out'], KERNEL * F32_PIXELS, what + ' pixels')
    close_gbuffer(dg[lo:lo + cnt], ref['d_gbuffer'], ref['mass_gbuffer'], case.layout, KERNEL, what)
    if case.band is not None:   # grad_out is zero outside the band: so is d gbuffer, exactly
        assert not dg[:lo].any() and not dg[lo + cnt:].any()
    for k, want in ref['d_params'].items():
        close(dp[k], want, ref['mass_params'][k], KERNEL * F32_D_PARAMS, what + ' d_' + k)
    return out, dg, dp


def compare_extra(name, dev, what, params_grad=True, g_grad=True):
    """an extra case against its shared restatement, with the parameter gradients and / or d gbuffer wanted"""
    case, ref = extra_case(name)
    out, dg, dp = run_fused(case, dev, params_grad=params_grad, g_grad=g_grad)
    close(out.reshape(-1, 3), ref['out'], ref['mass_out'], KERNEL * F32_PIXELS, what + ' pixels')
    if g_grad:
        close_gbuffer(dg.reshape(-1, case.cg), ref['d_gbuffer'], ref['mass_gbuffer'], case.layout, KERNEL, what)
    else:
        assert dg is None
    assert set(dp) == set(ref['d_params'])
    for k, want in ref['d_params'].items():
        if params_grad:
            close(dp[k], want, ref['mass_params'][k], KERNEL * F32_D_PARAMS, what + ' d_' + k)
        else:
            assert dp[k] is None, k
    return out, dg, dp


# ---------------------------------------------------------------------------------------------------------------- CPU tests

def test_restatement_in_float32_is_the_sample_shader():
    """The restatement with the sample's lights, run in float32, equals examples/deferred.py::shader_fn on a CPU G-buffer of
    the sample's layout: pixels and all gradients to the last few ulps."""
    ex = _load_example('deferred')
    g, lights, kw, go, view, light = sample_frame(5, 5000)
    r32 = R.compose(g, lights, R.SAMPLE_LAYOUT, grad_out=go, dtype=torch.float32, masses=False, **kw)
    gt, lt, vt = torch.from_numpy(g).requires_grad_(True), light.clone().requires_grad_(True), view.clone().requires_grad_(True)
    px = ex.shader_fn(gt, vt, lt)
    px.backward(torch.from_numpy(go))
    r64 = R.compose(g, lights, R.SAMPLE_LAYOUT, grad_out=go, dtype=torch.float64, **kw)
    # two float32 evaluations of one composition, each within F32_* of the float64 one (they differ in the order of three
    # additions and in torch's pow for a python-number exponent): within 2 x F32_* of each other
    assert R.worst_ratio(px.detach(), r32['out'], r64['mass_out']) <= 2 * F32_PIXELS
    for name, sl in R.attribute_slices(R.SAMPLE_LAYOUT).items():
        assert R.worst_ratio(gt.grad[:, sl], r32['d_gbuffer'][:, sl], r64['mass_gbuffer'][:, sl]) <= 2 * F32_D_GBUFFER[name], name
    d_light = r32['d_params']['light0.vector'] + r32['d_params']['light1.vector']
    m_light = r64['mass_params']['light0.vector'] + r64['mass_params']['light1.vector']
    assert R.worst_ratio(lt.grad[None], d_light, m_light) <= 2 * F32_D_PARAMS
    # the view matrix receives the camera position's gradient through inv(): compare that
    (d_cam_view,) = torch.autograd.grad(torch.linalg.inv(vt)[3, :3], vt, r32['d_params']['camera_position'][0])
    assert torch.allclose(vt.grad, d_cam_view, rtol=1e-4, atol=1e-7)
    assert bool((px.detach() != r32['out']).float().mean() < 0.5)   # and most pixels agree exactly


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    good = dict(scenes=1, pixels=64, cg=10, oc=4, on=7, op=1, om=0, ps=1, nl=2, kinds=0 | (1 << 2), sided=0, lo=0., hi=1., flags=3)

    def fwd(g=one, p=one, o=one, **over):
        a = dict(good, **over)
        return lib.dirt_shade_forward(g, p, o, a['scenes'], a['pixels'], a['cg'], a['oc'], a['on'], a['op'], a['om'], a['ps'], a['nl'], a['kinds'],
                                      a['sided'], a['lo'], a['hi'], a['flags'], None)

    def bwd(g=one, p=one, go=one, gg=one, gp=one, scratch=one, nbytes=1 << 20, **over):
        a = dict(good, **over)
        return lib.dirt_shade_backward(g, p, go, gg, gp, scratch, nbytes, a['scenes'], a['pixels'], a['cg'], a['oc'], a['on'], a['op'], a['om'],
                                       a['ps'], a['nl'], a['kinds'], a['sided'], a['lo'], a['hi'], a['flags'], None)

    bad = [dict(g=None), dict(p=None), dict(o=None), dict(scenes=-1), dict(pixels=-5), dict(cg=0), dict(oc=8), dict(on=-1), dict(oc=6),
           dict(op=2), dict(om=5), dict(om=10), dict(op=9), dict(nl=9), dict(nl=-1), dict(op=-1), dict(flags=1), dict(kinds=3), dict(ps=2),
           dict(lo=2., hi=1.)]
    for over in bad:
        assert fwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_shade_forward'), over
    for over in bad:
        over = {('go' if k == 'o' else k): v for k, v in over.items()}
        assert bwd(**over) == _lib.E_INVALID_ARGUMENT, over
        assert lib.dirt_last_error().startswith(b'dirt_shade_backward'), over
    assert bwd(scratch=None) == _lib.E_INVALID_ARGUMENT and bwd(nbytes=8) == _lib.E_INVALID_ARGUMENT
    assert bwd(scratch=ctypes.c_void_p(18)) == _lib.E_INVALID_ARGUMENT
    with pytest.raises(ValueError, match='dirt_shade_backward'):
        _lib.check(bwd(nbytes=8))
    # zero pixels (or scenes): a success that launches nothing, whatever the pointers
    assert fwd(g=None, p=None, o=None, pixels=0) == 0 and fwd(scenes=0, ps=0) == 0
    assert bwd(g=None, p=None, go=None, gg=None, gp=None, scratch=None, nbytes=0, pixels=0) == 0
    assert lib.dirt_last_error() == b''
    # scratch: one row of 9 + 8 lights floats per workgroup of 1024 pixels and scene
    assert lib.dirt_shade_scratch_bytes(1, 2048 * 2048, 2) == 4096 * 25 * 4
    assert lib.dirt_shade_scratch_bytes(3, 1025, 8) == 3 * 2 * 73 * 4
    assert lib.dirt_shade_scratch_bytes(1, 0, 0) == 0 and lib.dirt_shade_scratch_bytes(-1, 5, 0) == 0 and lib.dirt_shade_scratch_bytes(1, 5, 9) == 0


def test_shade_gbuffer_refuses_bad_arguments():
    from dirt_amd import shading
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        shading.shade_gbuffer(torch.zeros(4, 4, 10), [], colors=4, normals=7)
    g = torch.zeros(4, 4, 10)   # the checks behind the device check, called directly: they look at shape and device only

    def check(g, lights, colors, normals, positions=None, mask=None, ambient=(0., 0., 0.), camera_position=None, background=(0., 0., 0.),
              clamp=(0., 1.)):
        return shading._check_arguments(g, list(lights), colors, normals, positions, mask, ambient, camera_position, background, clamp)

    d, c = (0., 0., -1.), (1., 1., 1.)
    ok = dict(colors=4, normals=7, positions=1, mask=0)
    for kw, lights, match in (
            (dict(ok, colors=8), [], 'does not fit'), (dict(ok, mask=10), [], 'does not fit'), (dict(ok, normals=-1), [], 'does not fit'),
            (dict(ok, positions=3), [], 'overlaps'), (dict(ok, mask=5), [], 'overlaps'), (dict(ok, colors=4.), [], 'index of a G-buffer channel'),
            (ok, [('diffuse_directional', d, c, True)] * 9, 'at most 8'),
            (ok, [('lambert', d, c, True)], 'expected a record'), (ok, [('diffuse_directional', d, c)], 'has 4 fields'),
            (ok, [('specular_directional', d, c, 6., True)], 'needs camera_position'),
            (dict(ok, positions=None), [('diffuse_point', d, c, True)], 'needs the `positions`'),
            (ok, [('diffuse_directional', (0., 1.), c, True)], '3 numbers'),
            (ok, [('diffuse_directional', torch.zeros(2, 3), c, True)], 'must have shape'),
            (dict(ok, clamp=(1., 0.)), [], 'lo <= hi'), (dict(ok, clamp=3.), [], 'clamp must be'),
            (dict(ok, ambient=(1., 2.)), [], '3 numbers')):
        with pytest.raises(ValueError, match=match):
            check(g, lights, **kw)
    assert check(g, [('diffuse_directional', d, c, True)], **ok)[0] == [4, 7, 1, 0]
    with pytest.raises(ValueError, match='expects gbuffer'):
        shading.shade_gbuffer(torch.zeros(5), [], colors=0, normals=3)


def test_the_module_is_exported_under_both_package_names():
    import dirt
    import dirt_amd
    import dirt.shading
    assert dirt.shading is dirt_amd.shading and callable(dirt_amd.shading.shade_gbuffer)
    from dirt_amd import build
    assert 'dirt_shade.hip' in build.SOURCES


def test_test_data_stays_off_the_kinks():
    """Drawn pixels are rejected against the float64 restatement; under 5 % of a first draw may be (Case asserts it)."""
    for case in (light_case('mixed8', True, True, (0., 1.)), shape_case('c16')):
        assert case.share < 0.05
        assert bool(R.off_kinks(case.reference(masses=False), case.kw['clamp']).all())


def test_extra_cases_stay_within_the_committed_figures():
    """EXTRA_CASES are not part of what F32_* was measured on; the float32 composition's own error on each of them is within the
    committed figures all the same, so 4 x F32_* allows the kernel there what it allows it on tolerance_cases().  A case that
    does not stay within them gets another seed, never a wider bound.  (Case itself asserts draw_off_kinks' cap: under 5 % of
    a first draw rejected.)"""
    committed = dict({'d_' + k: v for k, v in F32_D_GBUFFER.items()}, pixels=F32_PIXELS, d_params=F32_D_PARAMS)
    for name in EXTRA_CASES:
        case, _ = extra_case(name)
        assert case.share < 0.05
        measured = R.measure_f32([case.measure()])
        print(name, ' '.join('%s %.2f' % (k, v / committed[k]) for k, v in measured.items()))
        for k, v in measured.items():
            assert v <= committed[k], '%s %s: committed %.3e, measured on this case %.3e' % (name, k, committed[k], v)


def test_the_extra_cases_hold_what_their_names_say():
    """The light sets, the three regimes of the copy-out walk, the attributes that straddle channel 256 or sit in the last three
    channels, the layouts without positions and the scenes that end on a workgroup boundary: a change of SHADE_BLOCK or
    SHADE_ITER fails here instead of leaving the cases short of the paths they are for."""
    from dirt_amd import _lib
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_shade.hip')).read()
    assert 'constexpr int SHADE_BLOCK = 256;' in source and 'constexpr int SHADE_ITER = 4;' in source
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    assert '#define DIRT_SHADE_MAX_CHANNELS 1024' in header and _lib.SHADE_MAX_LIGHTS == 8
    assert sorted(COUNT_SETS) == [0, 1, 2, 4, 5, 6, 7, 8] and all(len(v) == n for n, v in COUNT_SETS.items())
    assert all(set(v) == set(KINDS) for n, v in COUNT_SETS.items() if n >= 3) and set(COUNT_SETS[2]) == set(KINDS[1:])
    # every instantiation <NL, PARAMS, GBUF> is launched: 3 lights by test_only_the_needed_gradients and the shape cases, 1 and 8
    # with both gradients by the light cases, the rest here
    launched = {(n, WANTED[v]) for n, v in COUNT_VARIANTS} | {(3, w) for w in WANTED.values()} | {(1, (True, True)), (8, (True, True))}
    assert launched == {(n, w) for n in range(9) for w in WANTED.values()}
    for name in EXTRA_CASES:
        case, ref = extra_case(name)
        kw = EXTRA_CASES[name]
        assert len(case.lights) == len(kw['kinds']) and [bool(r[-1]) for r in case.lights] == list(kw['double_sided'])
        assert case.g.shape == (case.n, case.cg) and bool(R.off_kinks(ref, case.kw['clamp']).all())
        if kw['kinds'] and len(kw['kinds']) > 1 and not name.startswith('c'):
            assert len({bool(r[-1]) for r in case.lights}) == 2, name     # mixed sidedness
    assert extra_case('lights0')[0].lights == [] and not extra_case('lights0')[1]['d_params']['camera_position'].any()
    assert not extra_case('lights0')[1]['mass_params']['camera_position'].any()
    regimes = {name: (256 // LAYOUTS[name][0], 256 % LAYOUTS[name][0]) for name in WIDE}
    assert regimes == {'c17': (15, 1), 'c255': (1, 1), 'c256': (1, 0), 'c257': (0, 256), 'c1024': (0, 256)}
    for name in WIDE:
        cg, layout = LAYOUTS[name]
        spans = R.attribute_slices(layout)
        assert any(sl.stop == cg for sl in spans.values()), name                                        # an attribute in the last channels
        if cg > 256:
            assert any(sl.start < 256 < sl.stop for sl in spans.values()), name                       # one straddles channel 256
        assert extra_case(name)[0].n == (259 if cg == 1024 else 1027)
        unused = np.ones(cg, bool)
        for sl in spans.values():
            unused[sl] = False
        assert bool(np.abs(extra_case(name)[0].g[:, unused]).min() > 0)                                  # noise in every unused channel
    assert LAYOUTS['c17'][1]['mask'] == 0 and LAYOUTS['c1024'][1]['mask'] == 1023
    for name in NO_POSITIONS:
        case, ref = extra_case(name)
        assert case.layout['positions'] is None and 'positions' not in R.attribute_slices(case.layout)
        assert all(r[0] == 'diffuse_directional' for r in case.lights) and len(case.lights) in (1, 3)
    assert len(NO_POSITIONS) == 12 and {extra_case(n)[0].cg for n in NO_POSITIONS} == {6, 7, 12}
    assert {extra_case(n)[0].kw['clamp'] for n in NO_POSITIONS} == {None, (0., 1.)}
    assert [extra_case(n)[0].shape for n in BOUNDARY] == [(3, 32, 32), (3, 32, 32), (3, 25, 41), (3, 25, 41)] and 25 * 41 == 1025
    assert lib_blocks(1024) == 1 and lib_blocks(1025) == 2 and lib_blocks(1027) == 2


def lib_blocks(pixels):
    """backward workgroups (rows of partial sums) per scene, from the scratch size the library asks for"""
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load().dirt_shade_scratch_bytes(1, pixels, 0) // (4 * 9)


def test_per_scene_blocks_differ_enough_to_show_a_neighbours():
    """The per-scene boundary cases with the blocks of two neighbouring scenes swapped in the restatement: pixels and d gbuffer move
    past the bound the GPU test applies, by the margins printed (found on the CPU: a scene's pixels move by 3e4 to 2e6 x the bound
    for every pair of scenes, its last pixel alone -- the one a workgroup of one pixel shades -- by 1e4 to 2e5 x), and the scenes' parameter gradients are more
    than 10 x the bound apart, so a row of partial sums added to a neighbour's total would show."""
    for name in BOUNDARY:
        if not name.endswith('per_scene'):
            continue
        case, ref = extra_case(name)
        for a, b in ((0, 1), (1, 2)):
            perm = np.arange(3)
            perm[[a, b]] = perm[[b, a]]
            swapped = R.compose(case.g, case.lights, case.layout, grad_out=case.go, scene_index=perm[case.idx], masses=False, **case.kw)
            px = case.n // 3
            for scene in (a, b):
                rows = slice(scene * px, (scene + 1) * px)
                margin = R.worst_ratio(swapped['out'][rows], ref['out'][rows], ref['mass_out'][rows]) / (KERNEL * F32_PIXELS)
                # the last pixel of the scene alone: the one a workgroup of one pixel shades
                last = slice((scene + 1) * px - 1, (scene + 1) * px)
                margin_last = R.worst_ratio(swapped['out'][last], ref['out'][last], ref['mass_out'][last]) / (KERNEL * F32_PIXELS)
                print('%s: scenes %d and %d swapped, scene %d: pixels move by %.0f x the bound, its last pixel by %.0f x' % (name, a, b, scene, margin, margin_last))
                assert margin > 1000. and margin_last > 10.
                dg = max(R.worst_ratio(swapped['d_gbuffer'][rows, sl], ref['d_gbuffer'][rows, sl], ref['mass_gbuffer'][rows, sl]) / (KERNEL * F32_D_GBUFFER[attr])
                         for attr, sl in R.attribute_slices(case.layout).items())
                assert dg > 10., (name, scene, dg)
                # a row of partial sums added to the neighbour's total: the scenes' parameter gradients are as far apart
                other = b if scene == a else a
                for k, want in ref['d_params'].items():
                    moved = R.worst_ratio(want[other], want[scene], ref['mass_params'][k][scene]) / (KERNEL * F32_D_PARAMS)
                    assert moved > 10., (name, k, scene, moved)


def test_c_entry_points_take_1024_channels_and_refuse_1025(lib):
    """DIRT_SHADE_MAX_CHANNELS: 1025 channels are refused by both entry points, 1024 pass the checks (zero pixels: a success
    that launches nothing, so no device is needed), attributes in the last channels included."""
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)

    def fwd(cg, pixels=0, on=7):
        return lib.dirt_shade_forward(one, one, one, 1, pixels, cg, 4, on, 1, 0, 1, 2, 0 | (1 << 2), 0, 0., 1., 3, None)

    def bwd(cg, pixels=0, on=7):
        return lib.dirt_shade_backward(one, one, one, one, one, one, 1 << 20, 1, pixels, cg, 4, on, 1, 0, 1, 2, 0 | (1 << 2), 0, 0., 1., 3, None)

    for f, who in ((fwd, b'dirt_shade_forward'), (bwd, b'dirt_shade_backward')):
        for pixels in (0, 64):
            assert f(1025, pixels) == _lib.E_INVALID_ARGUMENT
            assert lib.dirt_last_error().startswith(who) and b'1025 G-buffer channels' in lib.dirt_last_error()
        assert f(1024) == 0 and lib.dirt_last_error() == b''
        assert f(1024, on=1021) == 0 and f(1024, on=1022) == _lib.E_INVALID_ARGUMENT and f(1024, 64, on=1022) == _lib.E_INVALID_ARGUMENT
        assert f(2 ** 20) == _lib.E_INVALID_ARGUMENT and f(0) == _lib.E_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('n, variant', COUNT_VARIANTS, ids=['%d-%s' % nv for nv in COUNT_VARIANTS])
def test_light_counts_with_the_wanted_gradients(gpu, n, variant):
    """shade_backward_kernel<NL, PARAMS, GBUF> for the NL no other test launches (0, 2, 4, 5, 6, 7: both gradients, the parameters'
    alone, the G-buffer's alone) and for 1 and 8 lights with one of the two: each instantiation has its own register array,
    its own parameter slots and its own pad slots in the wave reduction.  The parameters are GPU leaves where wanted."""
    params_grad, g_grad = WANTED[variant]
    _, _, dp = compare_extra('lights%d' % n, gpu, '%d lights, %s' % (n, variant), params_grad=params_grad, g_grad=g_grad)
    if n == 0 and params_grad:     # ambient and background only: nothing reaches the camera
        assert not dp['camera_position'].any()


@pytest.mark.gpu
@pytest.mark.parametrize('name', WIDE)
def test_wide_gbuffers_against_the_restatement(gpu, name):
    """17 to 1024 channels with the attributes shuffled, across channel 256 and in the last channels: the three regimes of the
    backward's copy-out walk (Cg < 256, == 256, > 256) and the second turn of its s_src fill loop; the noise in the channels no
    attribute uses comes back as exact zeros in d gbuffer."""
    compare_extra(name, gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', NO_POSITIONS)
def test_layouts_without_positions(gpu, name):
    """positions=None (offset -1: load_pixel zeroes p, shade_source skips the attribute) on 6, 7 and 12 channels under one and
    three diffuse directional lights, with and without the clamp."""
    compare_extra(name, gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', BOUNDARY)
def test_scenes_that_end_on_a_workgroup_boundary(gpu, name):
    """Three scenes of exactly 1024 pixels (no partial workgroup) and of 1025 (a last workgroup with one pixel), with one
    parameter block per scene -- the blocks differ enough that a neighbour's would show
    (test_per_scene_blocks_differ_enough_to_show_a_neighbours) -- and with a shared one, whose reduce adds scenes x workgroups rows."""
    compare_extra(name, gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', SAME_BITS)
def test_two_runs_of_the_extra_cases_give_the_same_bits(gpu, name):
    case, _ = extra_case(name)
    (o1, dg1, dp1), (o2, dg2, dp2) = run_fused(case, gpu), run_fused(case, gpu)
    assert torch.equal(o1, o2) and torch.equal(dg1, dg2) and bool(dg1.abs().max() > 0)
    for k in dp1:
        assert torch.equal(dp1[k], dp2[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('name,ds,mask,clamp', LIGHT_CASES, ids=['%s-%s-%s-%s' % (n, 'double' if d else 'single', 'mask' if m else 'nomask',
                                                                                      'clamp' if c else 'noclamp') for n, d, m, c in LIGHT_CASES])
def test_light_kinds_against_the_restatement(gpu, name, ds, mask, clamp):
    compare(light_case(name, ds, mask, clamp), gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(SHAPE_CASES))
def test_layouts_and_shapes_against_the_restatement(gpu, name):
    compare(shape_case(name), gpu, name)


@pytest.mark.gpu
def test_a_2048x2048x16_frame_against_the_restatement_on_a_band(gpu):
    """The restatement runs on a 64-row band of the frame; grad_out is zero outside it, so that the parameter gradients of the
    whole frame are the band's and d gbuffer is exactly zero elsewhere."""
    compare(band_case(), gpu, '2048x2048x16')


@pytest.mark.gpu
def test_non_contiguous_and_misaligned_gbuffers(gpu):
    case = shape_case('33x17')
    wide = torch.zeros(33, 17, 14, device=gpu)
    wide[..., 2:12] = torch.from_numpy(case.g).to(gpu).reshape(33, 17, 10)
    compare(case, gpu, 'non-contiguous', g=wide[..., 2:12])
    flat = torch.zeros(33 * 17 * 10 + 1, device=gpu)
    flat[1:] = torch.from_numpy(case.g).to(gpu).reshape(-1)
    view = flat[1:].view(33, 17, 10)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    compare(case, gpu, 'misaligned', g=view)


def _constructed(dev, rows, lights, kw, go=None, layout=R.SAMPLE_LAYOUT, tensors=()):
    """fused and restated results on hand-made pixels (rows of the sample's layout); `tensors`: parameter names made GPU leaves"""
    from dirt_amd import shading
    g_np = np.asarray(rows, dtype=np.float32)
    go_np = np.ones((len(g_np), 3), np.float32) if go is None else np.asarray(go, np.float32)
    ref = R.compose(g_np, lights, layout, grad_out=go_np, **kw)
    g = torch.from_numpy(g_np).to(dev).requires_grad_(True)
    named = {}

    def T(name, x):
        if name not in tensors:
            return x
        named[name] = torch.tensor(np.asarray(x, dtype=np.float32), device=dev, requires_grad=True)
        return named[name]

    gl = [(r[0], T('light%d.vector' % i, r[1]), T('light%d.color' % i, r[2])) + ((T('light%d.shininess' % i, r[3]),) if len(r) == 5 else ()) + (r[-1],)
          for i, r in enumerate(lights)]
    gkw = {k: (T(k, v) if k != 'clamp' and v is not None else v) for k, v in kw.items()}
    out = shading.shade_gbuffer(g, gl, **layout, **gkw)
    out.backward(torch.from_numpy(go_np).to(dev))
    return ref, out, g.grad, {k: t.grad for k, t in named.items()}


def _check_constructed(ref, out, dg, dp, what):
    close(out, ref['out'], ref['mass_out'], KERNEL * F32_PIXELS, what + ' pixels')
    close_gbuffer(dg, ref['d_gbuffer'], ref['mass_gbuffer'], R.SAMPLE_LAYOUT, KERNEL, what)
    for k, v in dp.items():
        close(v, ref['d_params'][k], ref['mass_params'][k], KERNEL * F32_D_PARAMS, what + ' d_' + k)


@pytest.mark.gpu
@pytest.mark.parametrize('double_sided', [False, True])
def test_kink_background_pixels(gpu, double_sided):
    """The commonest pixel of a real frame: all attributes zero, so every cosine is exactly 0.  max(x, 0) passes the gradient
    there, abs gives 0; the mask still receives lit - background."""
    d = np.asarray([0.6, -0.64, -0.48], np.float32)
    lights = [('diffuse_directional', d, (1., 0.5, 0.25), double_sided), ('specular_directional', d, (1., 1., 1.), 6., double_sided),
              ('diffuse_point', (2., 1., -1.), (0.3, 0.3, 0.9), double_sided)]
    kw = dict(ambient=(0.2, 0.2, 0.2), background=(0., 0., 0.3), camera_position=(0.5, 1.5, 3.), clamp=(0., 1.))
    rows = [[0.] * 10, [0.] * 10, [1., 0.1, 0.2, 0.3, 0.5, 0.6, 0.7, 0., 0., 1.], [0., 0.1, 0.2, 0.3, 0.5, 0.6, 0.7, 0., 0., 0.]]
    tensors = ('light0.vector', 'light1.vector', 'light2.vector', 'light1.shininess', 'background', 'ambient', 'camera_position', 'light0.color')
    ref, out, dg, dp = _constructed(gpu, rows, lights, kw, tensors=tensors)
    _check_constructed(ref, out, dg, dp, 'background pixels, double_sided=%s' % double_sided)
    # the difference the two conventions make is visible in the restatement itself: the normal of a zero pixel gets a gradient
    # from max(x, 0) only if its mask is non-zero; at least the mask gradient is non-zero here (lit - background = -0.3 in blue)
    assert float(dg[0, 0]) == pytest.approx(-0.3, abs=1e-6)


@pytest.mark.gpu
def test_kink_single_sided_zero_cosine_passes_the_gradient(gpu):
    """A covered pixel whose normal is exactly perpendicular to the light: max(cos, 0) passes the gradient at cos == 0 (the
    normal's gradient is the light's), abs gives 0."""
    rows = [[1., 0., 0., 0., 0.5, 0.5, 0.5, 1., 0., 0.]]
    for ds in (False, True):
        lights = [('diffuse_directional', (0., 0., -1.), (1., 1., 1.), ds)]
        ref, out, dg, dp = _constructed(gpu, rows, lights, dict(ambient=(0.1, 0.1, 0.1), clamp=(0., 1.)), tensors=('light0.vector',))
        _check_constructed(ref, out, dg, dp, 'zero cosine, double_sided=%s' % ds)
        assert (float(dg[0, 9]) != 0.) == (not ds)


@pytest.mark.gpu
def test_kink_where_the_1e_12_sits(gpu):
    """The reference's two 1e-12s are visible only where the rest vanishes.  Pixel 0: the view vector is exactly perpendicular to
    the reflected direction (zero normal, so r = d = x; camera straight above), so cos = 1e-12 * sum(r) and, without ambient, the
    pixel is 1e-12 * colour -- 0 if the 1e-12 were added anywhere else.  Pixel 1 sits exactly at the point light: e = 0 and
    e / (|e| + 1e-12) = 0 where e / |e| would be NaN; the gradient to its position is n * 1e12, finite."""
    lights = [('specular_directional', (1., 0., 0.), (1., 1., 1.), 1., False), ('diffuse_point', (0.25, 0.5, -1.), (1., 1., 1.), False)]
    kw = dict(ambient=(0., 0., 0.), camera_position=(0., 0., 3.), clamp=None)
    rows = [[1., 0., 0., 0., 0.5, 0.25, 1., 0., 0., 0.], [1., 0.25, 0.5, -1., 0.5, 0.5, 0.5, 0., 0.6, 0.8]]
    ref, out, dg, dp = _constructed(gpu, rows, lights, kw, tensors=('light0.vector', 'light1.vector', 'camera_position'))
    _check_constructed(ref, out, dg, dp, 'the 1e-12s')
    assert float(out[0, 2]) == pytest.approx(1e-12, rel=1e-5) and bool(torch.isfinite(dg).all()) and float(dg[1, 1:4].abs().max()) > 1e10


@pytest.mark.gpu
def test_kink_clamp_edges_pass_the_gradient(gpu):
    """Pre-clamp values exactly at lo and at hi (exactly representable: colour x ambient with powers of two): torch's clamp
    passes the gradient at both edges; just outside it does not."""
    kw = dict(ambient=(0.5, 0.5, 0.5), background=(0., 0., 0.), clamp=(0.25, 1.))
    rows = [[1., 0., 0., 0., 0.5, 2., 2.5, 0., 0., 1.],     # pre = 0.25 (lo), 1 (hi), 1.25 (above)
            [1., 0., 0., 0., 0.25, 1., 0.5, 0., 0., 1.]]    # pre = 0.125 (below), 0.5, 0.25 (lo)
    ref, out, dg, dp = _constructed(gpu, rows, [], kw, tensors=('ambient',))
    _check_constructed(ref, out, dg, dp, 'clamp edges')
    assert dg[0, 4:7].tolist() == [0.5, 0.5, 0.] and dg[1, 4:7].tolist() == [0., 0.5, 0.5]


@pytest.mark.gpu
@pytest.mark.parametrize('shininess', [1., 2., 6.])
def test_kink_zero_cosine_under_pow(gpu, shininess):
    """pow(0, s): gradient 0 to s; to its base 0 for s > 1 and 1 at s = 1.  Both lights have a zero direction, so the reflected
    direction and with it the cosine are exactly 0, single sided (light 0) and double sided (light 1), on a covered and on an
    uncovered pixel."""
    lights = [('specular_directional', (0., 0., 0.), (1., 1., 1.), shininess, False),
              ('specular_directional', (0., 0., 0.), (1., 1., 1.), shininess, True)]
    kw = dict(ambient=(0.1, 0.1, 0.1), camera_position=(0., 0., 3.), clamp=None)
    rows = [[1., 0.1, 0.2, 0., 0.5, 0.5, 0.5, 0., 0., 1.], [1., 0., 0., 0., 1., 1., 1., 0., 0., 0.]]
    tensors = ('light0.vector', 'light0.shininess', 'light1.shininess', 'camera_position')
    ref, out, dg, dp = _constructed(gpu, rows, lights, kw, tensors=tensors)
    _check_constructed(ref, out, dg, dp, 'pow(0, %g)' % shininess)
    assert float(dp['light0.shininess']) == 0. and float(dp['light1.shininess']) == 0.


@pytest.mark.gpu
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('attribute', ['normals', 'colors', 'positions', 'mask'])
@pytest.mark.parametrize('clamp', [None, (0., 1.)])
def test_non_finite_values_stay_in_their_pixel(gpu, bad, attribute, clamp):
    """A non-finite attribute makes its own pixel's output and gradient (and the parameter gradients) non-finite exactly where the
    composition does; every other pixel's output and d gbuffer are what they are without it."""
    case = non_finite_case(clamp)
    clean = case.reference()
    victim = 137
    case.g[victim, case.layout[attribute]] = bad
    ref = case.reference()
    out, dg, dp = run_fused(case, gpu)
    out, dg = out.detach().cpu().numpy(), dg.cpu().numpy()
    others = np.arange(case.n) != victim
    close(out[others], clean['out'][others], clean['mass_out'][others], KERNEL * F32_PIXELS, 'other pixels')
    close_gbuffer(dg[others], clean['d_gbuffer'][others], clean['mass_gbuffer'][others], case.layout, KERNEL, 'other pixels')
    assert np.array_equal(np.isfinite(out[victim]), np.isfinite(ref['out'][victim].numpy()))
    assert np.array_equal(np.isfinite(dg[victim]), np.isfinite(ref['d_gbuffer'][victim].numpy()))
    for k, want in ref['d_params'].items():
        assert np.array_equal(np.isfinite(dp[k].cpu().numpy().reshape(want.shape)), np.isfinite(want.numpy())), k


@pytest.mark.gpu
def test_only_the_needed_gradients(gpu):
    case = shape_case('33x17')
    ref = case.reference()
    out, dg, dp = run_fused(case, gpu, params_grad=False)
    assert all(v is None for v in dp.values())
    close_gbuffer(dg.reshape(-1, case.cg), ref['d_gbuffer'], ref['mass_gbuffer'], case.layout, KERNEL, 'no parameter gradient:')
    out, dg, dp = run_fused(case, gpu, g_grad=False)
    assert dg is None
    for k, want in ref['d_params'].items():
        close(dp[k], want, ref['mass_params'][k], KERNEL * F32_D_PARAMS, 'no G-buffer gradient: d_' + k)
    out, _, _ = run_fused(case, gpu, grad=False, params_grad=False, g_grad=False)
    assert not out.requires_grad


@pytest.mark.gpu
def test_parameter_gradients_are_reproducible_and_backward_is_reentrant(gpu):
    case = shape_case('640x480')
    _, dg1, dp1 = run_fused(case, gpu)
    _, dg2, dp2 = run_fused(case, gpu)
    assert torch.equal(dg1, dg2)
    for k in dp1:
        assert torch.equal(dp1[k], dp2[k]), k      # bit for bit: fixed-order sums, no atomics
    # backward twice over one forward (retain_graph=True, as _RasteriseDeferred.backward calls it)
    from dirt_amd import shading
    g = torch.from_numpy(case.g).to(gpu).reshape(case.shape + (case.cg,)).requires_grad_(True)
    d = torch.tensor(case.lights[0][1], device=gpu, requires_grad=True)
    out = shading.shade_gbuffer(g, [('diffuse_directional', d, (0.5, 0.4, 0.3), False)], ambient=(0.1, 0.1, 0.1), **case.layout)
    go = torch.from_numpy(case.go).to(gpu).reshape(out.shape)
    a = torch.autograd.grad(out, [g, d], go, retain_graph=True)
    b = torch.autograd.grad(out, [g, d], go, retain_graph=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].data_ptr() != b[0].data_ptr()


def _sample_fused_shader(gbuffer, view_matrix, light_direction):
    from dirt_amd import shading
    lights, kw = R.sample_lights(light_direction, torch.linalg.inv(view_matrix)[3, :3])
    return shading.shade_gbuffer(gbuffer, lights, **R.SAMPLE_LAYOUT, **kw)


@pytest.mark.gpu
def test_equals_the_sample_shader_on_the_gpu(gpu):
    """shade_gbuffer with the sample's lights against examples/deferred.py::shader_fn on the GPU.  Both are float32
    implementations of one composition: torch's is within F32_* of the float64 restatement, the kernel within 4 x that, so
    they are within 5 x of each other, per element, by the element's mass."""
    ex = _load_example('deferred')
    g_np, lights, kw, go_np, view, light = sample_frame(6, 480 * 640)
    ref = R.compose(g_np, lights, R.SAMPLE_LAYOUT, grad_out=go_np, **kw)
    res = []
    for fn in (ex.shader_fn, _sample_fused_shader):
        g = torch.from_numpy(g_np).to(gpu).reshape(480, 640, 10).requires_grad_(True)
        v, l = view.to(gpu).requires_grad_(True), light.to(gpu).requires_grad_(True)
        px = fn(g, v, l)
        px.backward(torch.from_numpy(go_np).to(gpu).reshape(px.shape))
        res.append((px.detach().reshape(-1, 3), g.grad.reshape(-1, 10), l.grad, v.grad))
    (pa, ga, la, va), (pb, gb, lb, vb) = res
    close(pb, pa.cpu().numpy(), ref['mass_out'], 5 * F32_PIXELS, 'fused vs torch on the GPU: pixels')
    close_gbuffer(gb, ga.cpu().numpy(), ref['mass_gbuffer'], R.SAMPLE_LAYOUT, 5, 'fused vs torch on the GPU:')
    m_light = ref['mass_params']['light0.vector'] + ref['mass_params']['light1.vector']
    close(lb[None], la[None].cpu().numpy(), m_light, 5 * F32_D_PARAMS, 'fused vs torch on the GPU: d_light')
    # the view matrix gets the camera position's gradient through inv(): linear in it, so the camera's mass carries over
    m_view = torch.autograd.functional.jacobian(lambda m: torch.linalg.inv(m)[3, :3], view.double()).abs().permute(1, 2, 0) @ \
        ref['mass_params']['camera_position'][0]
    close(vb, va.cpu().numpy(), m_view, 5 * F32_D_PARAMS, 'fused vs torch on the GPU: d_view')


@pytest.mark.gpu
def test_rasterise_deferred_with_the_fused_shader(gpu):
    """End to end on the cube of examples/deferred.py: rasterise_deferred with the fused shader against the same call with the
    torch shader.  Pixels and the light's gradient by the mass rule (5 x the float32 figure, as above; masses from the
    restatement on the rasterised G-buffer).  The vertex and view-matrix gradients come from filtering the shaded image,
    where a one-ulp pixel difference can flip a discrete dilation choice, and no mass is at hand for them: an element counts as
    agreeing if |a - b| <= 1e-3 * max(|a|, |b|) (or both are below 1e-7); elements that do not are excluded, and their share
    is capped at 1 % per tensor."""
    import dirt_amd
    ex = _load_example('deferred')
    verts_np, faces_np = ex.build_cube()
    results = []
    for fn in (ex.shader_fn, _sample_fused_shader):
        vertices = torch.from_numpy(verts_np).to(gpu).requires_grad_(True)
        faces = torch.from_numpy(faces_np).to(gpu)
        view = ex.matrices.compose(ex.matrices.translation(torch.tensor([0., -1.5, -3.5], device=gpu)),
                                   ex.matrices.rodrigues(torch.tensor([-0.3, 0., 0.], device=gpu))).requires_grad_(True)
        light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=gpu), dim=0).requires_grad_(True)
        clip, f2, attributes = ex.geometry(vertices, faces, view)
        pixels = dirt_amd.rasterise_deferred(vertices=clip, vertex_attributes=attributes, faces=f2,
                                             background_attributes=torch.zeros([ex.frame_height, ex.frame_width, 10], device=gpu),
                                             shader_fn=fn, shader_additional_inputs=[view, light])
        (pixels ** 2).mean().backward()
        gbuf = dirt_amd.rasterise(torch.zeros([ex.frame_height, ex.frame_width, 10], device=gpu), clip.detach(), attributes.detach(), f2)
        results.append((pixels.detach(), vertices.grad, view.grad, light.grad, gbuf, view.detach(), light.detach()))
    (pa, va, wa, la, gbuf, view, light), (pb, vb, wb, lb, _, _, _) = results
    lights, kw = R.sample_lights(light.cpu().numpy(), torch.linalg.inv(view)[3, :3].cpu().numpy())
    go = (2. / pa.numel()) * pa.reshape(-1, 3).cpu().numpy()
    ref = R.compose(gbuf.reshape(-1, 10).cpu().numpy(), lights, R.SAMPLE_LAYOUT, grad_out=go, **kw)
    close(pb.reshape(-1, 3), pa.reshape(-1, 3).cpu().numpy(), ref['mass_out'], 5 * F32_PIXELS, 'deferred: pixels')
    m_light = ref['mass_params']['light0.vector'] + ref['mass_params']['light1.vector']
    close(lb[None], la[None].cpu().numpy(), m_light, 5 * F32_D_PARAMS, 'deferred: d_light')
    for name, a, b in (('vertices', va, vb), ('view matrix', wa, wb)):
        a, b = a.cpu().double(), b.cpu().double()
        agree = ((a - b).abs() <= 1e-3 * torch.maximum(a.abs(), b.abs())) | ((a.abs() < 1e-7) & (b.abs() < 1e-7))
        share = 1. - float(agree.double().mean())
        print('deferred: d_%s: %d of %d elements excluded' % (name, int((~agree).sum()), agree.numel()))
        assert share <= 0.01, (name, share)
        assert bool(a.abs().max() > 0)


@pytest.mark.gpu
def test_graphed_step_captures_the_fused_shader(gpu):
    """A GraphedStep whose loss shades its pixels (a 10-channel rasterise_batch as the G-buffer) with shade_gbuffer captures --
    the call makes no host synchronisation -- and its replay returns the loss and gradients of the eager step."""
    import dirt_amd
    from dirt_amd import shading
    from tests import scenes
    s = scenes.rand_scene(200, 96, 128, 10, 41, 0.05, 0.3)
    bg, v, vc, f = (torch.from_numpy(s[k][None].copy()).to(gpu) for k in ('background', 'vertices', 'vertex_colors', 'faces'))
    direction = torch.tensor([0.6, -0.64, -0.48], device=gpu, requires_grad=True)
    camera = torch.tensor([0.5, 1.5, 3.], device=gpu)
    lights, kw = R.sample_lights(direction, camera)

    def loss_fn(px):
        return (shading.shade_gbuffer(px, lights, **R.SAMPLE_LAYOUT, **kw) ** 2).mean()

    step = dirt_amd.GraphedStep(bg, v, vc, f, loss_fn=loss_fn)
    for _ in range(2):
        loss, (gb, gv, gvc) = step()
    leaves = [t.detach().clone().requires_grad_(True) for t in (bg, v, vc)]
    eager = loss_fn(dirt_amd.rasterise_batch(leaves[0], leaves[1], leaves[2], f))
    eager.backward()
    torch.cuda.synchronize()
    assert float((loss - eager).detach().abs()) <= 1e-6 * float(eager.detach().abs())
    assert torch.equal(gb, leaves[0].grad)      # d gbuffer outside the mesh: the kernel's own output, no atomics on the way
    assert bool(gb.abs().max() > 0)
    for a, b in ((gv, leaves[1].grad), (gvc, leaves[2].grad)):   # float atomics in the rasteriser's gradient: summation order
        agree = (a - b).abs() <= 1e-4 * torch.maximum(a.abs(), b.abs()) + 1e-9
        assert float(agree.float().mean()) >= 0.99


# ---- many scenes, many rows of partial sums: shade_launch_reduce (dirt_shade.hip) and the grid's y dimension, which this file,
# tests/test_shade_sh.py and tests/test_shade_pbr_edges.py share.  The bound is derived from dirt_stage.h::block_column_sum:
# lane t adds rows t, t + 256, ... one after the other (ceil(rows / 256) additions, the first to a zero), then the 256 lanes
# fold in 8 halvings; the longest chain of additions an element passes through is L = ceil(rows / 256) + 8, and
# |sum32 - sum64| <= L 2^-24 sum |row| to first order.

REDUCE_BLOCK, FOLD_LEVELS = 256, 8     # SHADE_BLOCK lanes reduce a column; 256 -> 1 in eight halvings
MAX_SCENES = 65535                     # the grid's y dimension; 65536 is refused (test_c_entry_points_refuse_bad_arguments_without_a_device)
SPAN = 1024                            # pixels of a backward workgroup of the three shaders (BLOCK x ITER of each)


def reduce_chain(rows):
    """L: the additions of the longest chain block_column_sum makes over `rows` rows"""
    return -(-rows // REDUCE_BLOCK) + FOLD_LEVELS


def within_the_reduce_bound(got, rows, what):
    """got [P]: the float32 column sums of rows [R, P] by block_column_sum"""
    rows = rows.double().cpu()
    L = reduce_chain(rows.shape[0])
    err, bound = (got.double().cpu().reshape(-1) - rows.sum(0)).abs(), L * 2. ** -24 * rows.abs().sum(0)
    print('%s: %d rows, L = %d, worst |sum32 - sum64| / bound = %.3f' % (what, rows.shape[0], L, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((bound > 0).any()) and bool((err <= bound).all()), (what, err, bound)


def many_scenes(run, dev, pixels, values, seed, what):
    """[65535, 1, 1, Cg]: the grid's y dimension at its limit.  run(g, values, go) -> (out, d gbuffer, {name: gradient}) is the
    fused call with gradients; pixels: numpy [n, Cg], dealt out to the scenes in turn; values: {name: GPU tensor}, the
    parameters one block has.
    With a block per scene (the values times U(0.9, 1.1) per scene), a scene's output, d gbuffer and parameter gradients have
    the bits of a one-scene call on its pixel with its parameters.  With one block shared, output and d gbuffer have the bits
    of the pixels run as one flat frame, and the parameter sums -- 65535 rows, 256 turns of the reduce loop per lane -- lie
    within the bound of the float64 sum of the rows, which are what the per-scene call on the same values returns row by row
    (one row per scene there: its reduce adds the row to a zero)."""
    B, (n, cg) = MAX_SCENES, pixels.shape
    rng = np.random.default_rng(seed)
    g = torch.from_numpy(pixels)[torch.from_numpy(np.arange(B) % n)].to(dev).reshape(B, 1, 1, cg)
    go = torch.from_numpy(rng.standard_normal((B, 1, 1, 3)).astype(np.float32)).to(dev)
    rows_of = lambda v: v[None].expand((B,) + tuple(v.shape))   # noqa: E731
    per_scene = {k: (rows_of(v) * torch.from_numpy(rng.uniform(0.9, 1.1, (B,) + tuple(v.shape)).astype(np.float32)).to(dev)).contiguous()
                 for k, v in values.items()}
    out, dg, dp = run(g, per_scene, go)
    assert all(dp[k].shape == per_scene[k].shape for k in values)
    for s in (0, 1, 255, 256, 257, 32768, B - 256, B - 1):
        o1, g1, p1 = run(g[s:s + 1], {k: v[s] for k, v in per_scene.items()}, go[s:s + 1])
        assert torch.equal(out[s], o1[0]) and torch.equal(dg[s], g1[0]), (what, s)
        for k in values:
            assert torch.equal(dp[k][s], p1[k]), (what, s, k)
    _, _, rows = run(g, {k: rows_of(v).contiguous() for k, v in values.items()}, go)
    out, dg, dp = run(g, values, go)
    flat_out, flat_dg, _ = run(g.reshape(B, cg), values, go.reshape(B, 3))
    assert torch.equal(out.reshape(B, 3), flat_out) and torch.equal(dg.reshape(B, cg), flat_dg), what
    assert reduce_chain(B) == 264
    for k in values:
        within_the_reduce_bound(dp[k], rows[k].reshape(B, -1), '%s, 65535 scenes, d %s' % (what, k))


def frame_of_512_rows(run, dev, pixels, grad_out, values, seed, what):
    """[2, 512, 512, Cg] with one parameter block: 256 workgroups per scene, 512 rows, the reduce loop's second turn in every
    lane.  The frame is one workgroup's span of pixels (numpy [1024, Cg]) 512 times over, its grad_out that span's times a
    signed power of two per workgroup: output and d gbuffer have the bits of the span run alone (scaled: exact), and every
    row of partial sums is the span's parameter gradients scaled likewise, so the sums are known in float64."""
    copies, (n, cg) = 512, pixels.shape
    assert n == SPAN and grad_out.shape == (SPAN, 3)
    span_g, span_go = torch.from_numpy(pixels).to(dev), torch.from_numpy(grad_out).to(dev)
    o1, g1, p1 = run(span_g, values, span_go)
    # 1 or 2 in a lane's first turn, 0.5 or 4 in its second: the two rows a lane adds never cancel, so neither can go missing unseen
    rng = np.random.default_rng(seed)
    scale = rng.choice([-1., 1.], copies) * np.where(np.arange(copies) < REDUCE_BLOCK, rng.choice([1., 2.], copies), rng.choice([0.5, 4.], copies))
    scale = torch.from_numpy(scale.astype(np.float32)).to(dev)
    g = span_g.repeat(copies, 1).reshape(2, 512, 512, cg)
    go = (span_go[None] * scale[:, None, None]).reshape(2, 512, 512, 3)
    out, dg, dp = run(g, values, go)
    assert torch.equal(out.reshape(copies, SPAN, 3), o1[None].expand(copies, -1, -1)), what
    assert torch.equal(dg.reshape(copies, SPAN, cg), g1[None] * scale[:, None, None]) and bool(g1.any()), what
    assert reduce_chain(copies) == 10
    for k in values:
        within_the_reduce_bound(dp[k], p1[k].reshape(1, -1) * scale[:, None], '%s, 2 x 512 x 512, d %s' % (what, k))


def _many(dev):
    """-> (run, pixels, grad_out, values) of the two-light extra case for `many_scenes` and `frame_of_512_rows`"""
    from dirt_amd import shading
    case, _ = extra_case('lights2')
    values = {k: case.kw[k] for k in ('ambient', 'background', 'camera_position')}
    for i, rec in enumerate(case.lights):
        values['light%d.vector' % i], values['light%d.color' % i] = rec[1], rec[2]
        if rec[0] == 'specular_directional':
            values['light%d.shininess' % i] = rec[3]
    values = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev) for k, v in values.items()}

    def run(g, values, go):
        g = g.detach().requires_grad_(True)
        named = {k: v.detach().requires_grad_(True) for k, v in values.items()}
        lights = [(rec[0], named['light%d.vector' % i], named['light%d.color' % i]) +
                  ((named['light%d.shininess' % i],) if rec[0] == 'specular_directional' else ()) + (rec[-1],) for i, rec in enumerate(case.lights)]
        out = shading.shade_gbuffer(g, lights, clamp=case.kw['clamp'], **case.layout, **{k: named[k] for k in ('ambient', 'background', 'camera_position')})
        out.backward(go)
        return out.detach(), g.grad, {k: t.grad for k, t in named.items()}

    return run, case.g, case.go, values


@pytest.mark.gpu
def test_65535_scenes_of_one_pixel(gpu):
    run, pixels, _, values = _many(gpu)
    many_scenes(run, gpu, pixels, values, 5400, 'shade_gbuffer')


@pytest.mark.gpu
def test_a_2x512x512_frame_adds_512_rows(gpu):
    run, pixels, grad_out, values = _many(gpu)
    frame_of_512_rows(run, gpu, pixels[:SPAN], grad_out[:SPAN], values, 5401, 'shade_gbuffer')
