"""`dirt_amd.shading.shade_gbuffer_pbr(..., visibility=)` (dirt_shade_pbr.hip's VIS kernels, built as dirt_shade_pbr_visibility.hip)
and `dirt_amd.lighting.cook_torrance(..., visibility=)` against the restatement of tests/shade_pbr_visibility_reference.py.
Every comparison is per element, |gpu - ref64| <= KERNEL * F32 * (L1 mass of the element's terms); an element of zero mass
must equal the reference exactly; the channels of d gbuffer no attribute uses must be exact zeros.

The tolerances are tests/test_shade_pbr.py's convention: the float32 torch form is run on the cases of this file, its worst
|f32 - ref64| / mass per kind of result is F32, and the kernel gets KERNEL = 4 times that.  Produced by

    python -m tests.shade_pbr_visibility_reference
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import shade_pbr_reference as R
from tests import shade_pbr_visibility_reference as RV
from tests import test_shade_pbr as B

ROOT = B.ROOT
# worst |f32 - ref64| / mass of the float32 torch form on CASES, per kind of result (python -m tests.shade_pbr_visibility_reference)
F32 = {'pixels': 7.78e-7, 'd_colors': 9.38e-7, 'd_material': 1.02e-6, 'd_normals': 2.40e-6, 'd_positions': 1.48e-6, 'd_mask': 3.38e-7,
       'd_params': 5.94e-7, 'd_visibility': 1.12e-6}
KERNEL = B.KERNEL
D, P = B.D, B.P
FLAT, SPAN = B.FLAT, B.SPAN
IMAGE = (17, 19)


class Case:
    """Inputs of one comparison, as tests/test_shade_pbr.py::Case draws them, with a visibility [n, lights]: multiples of 2^-8 in
    [0, 1] (a tenth of them exactly 0, a tenth exactly 1), the lights' colours multiples of 2^-6, so that the restatement's
    per-pixel colour k s is exact in float32.  The pixels stay off the kinks of the shaded result, visibility included."""

    def __init__(self, seed, layout='c12', n=FLAT, kinds=(D, P), clamp=(0., 1.), mask=True, batch=None, per_scene='shared', zero_column=None,
                 shape=None):
        self.cg, lay = B.LAYOUTS[layout]
        self.layout = dict(lay)
        if not mask:
            self.layout['mask'] = None
        self.batch, self.kinds, self.shape = batch, tuple(kinds), shape
        self.n = n * (batch or 1)
        self.idx = np.repeat(np.arange(batch), n) if batch and per_scene != 'shared' else None
        rng = np.random.default_rng(seed)
        rows = batch if self.idx is not None else None
        lights = R.random_lights(rng, kinds, rows)
        shp = (rows, 3) if rows else (3,)
        self.params = {'ambient': rng.uniform(0.05, 0.3, shp), 'background': rng.uniform(0.1, 0.9, shp),
                       'camera_position': np.asarray([0.3, -0.2, 4.]) + 0.1 * rng.standard_normal(shp)}
        for i, (_, vector, _) in enumerate(lights):
            self.params['light%d.vector' % i], self.params['light%d.color' % i] = vector, RV.dyadic(rng, 0.2, 0.6, shp, RV.COLOR_BITS)
        self.params = {k: np.asarray(v, np.float32) for k, v in self.params.items()}
        self.lights = [(kind, self.params['light%d.vector' % i], self.params['light%d.color' % i]) for i, kind in enumerate(kinds)]
        u = rng.uniform(0., 1., (self.n, len(kinds)))
        self.vis = np.where(u < 0.1, 0., np.where(u < 0.2, 1., RV.dyadic(rng, 0., 1., (self.n, len(kinds)), RV.VISIBILITY_BITS))).astype(np.float32)
        if zero_column is not None:
            self.vis[:, zero_column] = 0.
        self.kw = dict(ambient=self.params['ambient'], camera_position=self.params['camera_position'], background=self.params['background'],
                       clamp=clamp, min_roughness=B.MIN_ROUGHNESS, dielectric_f0=B.DIELECTRIC_F0)
        # the draw of tests/shade_pbr_reference.py, its cap unchanged, on the lights as the pixels see them: colour k s per pixel
        idx = self.idx if self.idx is not None else np.zeros(self.n, np.int64)
        expand = lambda x: RV._rows(x, idx) if x.ndim == 2 else x   # noqa: E731
        px_lights = [(kind, expand(v), RV._rows(c, idx) * self.vis[:, i:i + 1]) for i, (kind, v, c) in enumerate(self.lights)]
        px_kw = {k: expand(v) if isinstance(v, np.ndarray) else v for k, v in self.kw.items()}
        self.g, self.colors, self.material, self.share = R.draw_off_kinks(rng, self.n, self.cg, self.layout, px_lights, px_kw,
                                                                          scene_index=np.arange(self.n))
        self.go = rng.standard_normal((self.n, 3)).astype(np.float32)

    def measure(self):
        return (self.g, self.lights, self.layout, self.vis), dict(self.kw, colors=self.colors, material=self.material, grad_out=self.go,
                                                                  scene_index=self.idx)

    def reference(self):
        args, kw = self.measure()
        return RV.compose(*args, **kw)


CASES = {
    'flat_1': dict(seed=7000, kinds=(D,)),
    'flat_2': dict(seed=7001, kinds=(P, D)),
    'flat_3': dict(seed=7002, kinds=(D, P, D), layout='t7'),
    'flat_4': dict(seed=7003, kinds=(D, P, P, D)),
    'tensors_1': dict(seed=7004, kinds=(P,), layout='t7', clamp=B.NARROW),
    'tensors_4': dict(seed=7005, kinds=(P, D, D, P), layout='t7'),
    'image_2': dict(seed=7006, kinds=(P, D), layout='tc', n=IMAGE[0] * IMAGE[1], shape=IMAGE, clamp=None),
    'image_3': dict(seed=7007, kinds=(D, D, P), layout='ct', n=IMAGE[0] * IMAGE[1], shape=IMAGE, mask=False),
    'c257': dict(seed=7008, kinds=(D, P), layout='c257', n=B.PBR_BLOCK + 3),
    'nomask_noclamp': dict(seed=7009, kinds=(P, P, D), mask=False, clamp=None),
    'scenes_shared': dict(seed=7010, kinds=(P, D), batch=3),
    'scenes_per_scene': dict(seed=7011, kinds=(D, P), layout='t7', batch=3, per_scene='per_scene'),
    'zero_column': dict(seed=7012, kinds=(D, P, D), zero_column=1),
}


def _options():
    """the four source combinations x with and without a mask x clamp set, None and narrow, as tests/test_shade_pbr.py has them; the
    light count goes round 1..4"""
    cases, i = {}, 0
    for source, layout in B.SOURCES.items():
        for mask in (True, False):
            for cname, clamp in (('clamp', (0., 1.)), ('noclamp', None), ('narrow', B.NARROW)):
                cases['%s-%s-%s' % (source, 'mask' if mask else 'nomask', cname)] = dict(seed=7050 + i, layout=layout, mask=mask, clamp=clamp,
                                                                                        kinds=(P, D, P, D)[:1 + i % 4])
                i += 1
    return cases


CASES.update(_options())
_CASES = {}


def case_of(name):
    if name not in _CASES:
        case = Case(**CASES[name])
        _CASES[name] = (case, case.reference())
    return _CASES[name]


def shade(case, dev, want=(True, True, True, True, True), visibility='case', drop=None):
    """-> dict of the fused call's results on `case`: out and the gradients wanted of (G-buffer, parameters, colour tensor, material
    tensor, visibility).  visibility: 'case', None (the call without one) or a tensor to pass as it is; drop: a light to leave
    out, with its column of the visibility."""
    from dirt_amd import shading
    want_g, want_p, want_c, want_m, want_v = want
    shape = (case.batch, case.n // case.batch, 1) if case.batch else (case.shape or (case.n,))
    t = lambda x: torch.from_numpy(x).to(dev)   # noqa: E731
    g = t(case.g).reshape(shape + (case.cg,)).requires_grad_(want_g)
    prm = {k: t(v).requires_grad_(want_p) for k, v in case.params.items()}
    col, mat = case.layout.get('colors'), case.layout.get('material')
    if col is None:
        col = t(case.colors).reshape(shape + (3,)).requires_grad_(want_c)
    if mat is None:
        mat = t(case.material).reshape(shape + (2,)).requires_grad_(want_m)
    keep = [i for i in range(len(case.kinds)) if i != drop]
    lights = [(case.kinds[i], prm['light%d.vector' % i], prm['light%d.color' % i]) for i in keep]
    leaf = None
    if isinstance(visibility, str):
        leaf = t(np.ascontiguousarray(case.vis[:, keep])).reshape(shape + (len(keep),)).requires_grad_(want_v)
        visibility = leaf
    out = shading.shade_gbuffer_pbr(g, lights, colors=col, material=mat, normals=case.layout['normals'], positions=case.layout['positions'],
                                    mask=case.layout.get('mask'), ambient=prm['ambient'], camera_position=prm['camera_position'],
                                    background=prm['background'], clamp=case.kw['clamp'], visibility=visibility)
    res = {'out': out.detach().reshape(-1, 3)}
    if out.requires_grad:
        out.backward(t(case.go).reshape(out.shape))
    if want_g:
        res['d_gbuffer'] = g.grad.reshape(-1, case.cg)
        for k, w in R.ATTRIBUTES:
            if case.layout.get(k) is not None:
                res['d_' + k] = res['d_gbuffer'][:, case.layout[k]:case.layout[k] + w]
    if isinstance(col, torch.Tensor) and want_c:
        res['d_colors'] = col.grad.reshape(-1, 3)
    if isinstance(mat, torch.Tensor) and want_m:
        res['d_material'] = mat.grad.reshape(-1, 2)
    if want_p:
        res['d_params'] = {k: v.grad for k, v in prm.items()}
    if leaf is not None and want_v:
        res['d_visibility'] = leaf.grad.reshape(-1, len(keep))
    return res


def check(case, got, ref, what, tol=None, factor=KERNEL):
    """The mass rule per kind of result, exact equality where the mass is zero, exact zeros in the unused channels."""
    tol = tol or F32
    worst = RV.ratios(got, ref)
    print(what, ' '.join('%s %.3e' % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= factor * tol[k], '%s %s: |got - ref64| / mass = %.3e, allowed %.3e' % (what, k, v, factor * tol[k])
    triples = [(got.get(key), ref.get(key), ref.get(mass)) for _, key, mass in R.PAIRS + (('d_visibility', 'd_visibility', 'mass_visibility'),)]
    triples += [(v, ref['d_params'][k], ref['mass_params'][k]) for k, v in (got.get('d_params') or {}).items()]
    for a, r, m in triples:
        if a is None:
            continue
        a = a.detach().cpu().double().reshape(r.shape)
        assert bool(torch.isfinite(a).all()), what
        assert torch.equal(a[m == 0], r[m == 0]), '%s: an element of zero mass differs' % what
    if got.get('d_gbuffer') is not None:
        unused = np.ones(case.cg, bool)
        for k, w in R.ATTRIBUTES:
            if case.layout.get(k) is not None:
                unused[case.layout[k]:case.layout[k] + w] = False
        assert not bool(got['d_gbuffer'][:, torch.from_numpy(unused).to(got['d_gbuffer'].device)].any()), '%s: d gbuffer of an unused channel' % what
    return worst


def compare(name, dev, want=(True,) * 5):
    case, ref = case_of(name)
    got = shade(case, dev, want)
    check(case, got, ref, name)
    return case, ref, got


def same_bits(a, b, keys=None):
    for k in keys or a:
        if k == 'd_params':
            for p in a[k]:
                assert torch.equal(a[k][p], b[k][p]), (k, p)
        else:
            assert torch.equal(a[k], b[k]), k


# ---- CPU tests

def test_cook_torrance_with_all_ones_has_the_bits_of_the_call_without():
    from dirt_amd import lighting
    rng = np.random.default_rng(7100)
    for dtype in (torch.float32, torch.float64):
        t = lambda x: torch.from_numpy(x).to(dtype).requires_grad_(True)   # noqa: E731
        results = []
        for ones in (False, True):
            rng = np.random.default_rng(7100)
            p, n, c = t(rng.uniform(-1., 1., (2, 9, 3))), t(rng.standard_normal((2, 9, 3))), t(rng.uniform(0., 1., (2, 9, 3)))
            r, mu, cam = t(rng.uniform(0., 1.2, (2, 9))), t(rng.uniform(0., 1., (2, 9))), t(np.asarray([[0.3, -0.2, 4.], [0., 0.1, 3.]]))
            lights = [(D, t(rng.standard_normal((2, 3))), t(rng.uniform(0., 1., (2, 3)))), (P, t(3. * rng.standard_normal((2, 3))), t(rng.uniform(0., 1., (2, 3))))]
            out = lighting.cook_torrance(p, n, c, r, mu, cam, lights, visibility=torch.ones(2, 9, 2, dtype=dtype) if ones else None)
            leaves = [p, n, c, r, mu, cam] + [x for rec in lights for x in rec[1:]]
            results.append([out.detach()] + list(torch.autograd.grad(out, leaves, torch.from_numpy(rng.standard_normal((2, 9, 3))).to(dtype))))
        for a, b in zip(*results):
            assert torch.equal(a, b)
    with pytest.raises(ValueError) as e:
        lighting.cook_torrance(p, n, c, r, mu, cam, lights, visibility=torch.ones(2, 9, 3))
    assert str(e.value) == 'visibility has 3 channels for 2 lights'
    # a plain multiplication: twice the visibility of one light adds that light's term once more; a NaN stays with its pixel
    one = lighting.cook_torrance(p, n, c, r, mu, cam, lights[:1]).detach()
    both = lighting.cook_torrance(p, n, c, r, mu, cam, lights).detach()
    vis = torch.ones(2, 9, 2, dtype=torch.float64)
    vis[..., 0] = 2.
    vis[1, 4, 1] = float('nan')
    got = lighting.cook_torrance(p, n, c, r, mu, cam, lights, visibility=vis).detach()
    ok = torch.ones(2, 9, dtype=torch.bool)
    ok[1, 4] = False
    assert bool(((got - (both + one)).abs()[ok] <= 1e-14 * (1. + both.abs()[ok])).all()) and bool(torch.isnan(got[1, 4]).all())


def test_the_torch_form_agrees_with_the_restatement():
    """`lighting.cook_torrance(visibility=)` composed in float64 against the restatement (the same function without a visibility,
    on per-pixel colours k s): two routes to the same numbers, within 1e-12 of each element's mass."""
    for name in ('flat_2', 'tensors_4', 'scenes_per_scene', 'zero_column', 'image_2'):
        case, ref = case_of(name)
        args, kw = case.measure()
        got = RV.torch_form(*args, dtype=torch.float64, **kw)
        worst = check(case, got, ref, name + ' float64', tol=dict.fromkeys(RV.KINDS, 1.), factor=1e-12)
        assert set(worst) >= {'pixels', 'd_normals', 'd_positions', 'd_params', 'd_visibility', 'd_colors', 'd_material'}, sorted(worst)


def test_the_float32_form_stays_within_the_committed_figures():
    """F32 is what `python -m tests.shade_pbr_visibility_reference` prints: measured again here on every case of this file;
    `draw_off_kinks` asserts its cap (under 5 % of a first draw rejected), which the cases stay under with the visibility in."""
    worst = dict.fromkeys(RV.KINDS, 0.)
    for name in CASES:
        case, _ = case_of(name)
        assert case.share < 0.05, name
        for k, v in RV.measure_f32([case.measure()]).items():
            assert v <= F32[k], '%s %s: committed %.3e, measured on this case %.3e' % (name, k, F32[k], v)
            worst[k] = max(worst[k], v)
    print({k: '%.3e' % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v >= 0.5 * F32[k], '%s: committed %.3e is not what these inputs give (%.3e)' % (k, F32[k], v)
        assert F32[k] <= 1e-5, k


def test_the_cases_hold_what_their_names_say():
    assert FLAT == 1027 and B.PBR_BLOCK == 256
    for name, kw in CASES.items():
        case, ref = case_of(name)
        assert case.vis.shape == (case.n, len(case.kinds)) and ref['d_visibility'].shape == case.vis.shape, name
        assert bool((case.vis == 0).any()) and bool((case.vis == 1).any()) and 0. <= case.vis.min() and case.vis.max() <= 1., name
    assert sorted({len(c['kinds']) for c in CASES.values()}) == [1, 2, 3, 4]
    assert case_of('image_2')[0].n == 17 * 19 and case_of('c257')[0].cg == 257 and case_of('c257')[0].n == 259
    assert case_of('scenes_per_scene')[0].params['light1.color'].shape == (3, 3) and case_of('scenes_shared')[0].idx is None
    assert not bool(case_of('zero_column')[0].vis[:, 1].any())
    assert case_of('tensors_4')[0].colors is not None and case_of('flat_4')[0].colors is None
    # a zero visibility is a zero mass for the light's colour at that pixel, and the restatement's gradient there is exactly 0
    case, ref = case_of('zero_column')
    assert not bool(ref['mass_params']['light1.color'].any()) and not bool(ref['d_params']['light1.color'].any())
    assert bool((ref['mass_visibility'][:, 1] > 0).any())


G = torch.zeros(4, 5, 12)


def test_shade_gbuffer_pbr_refuses_a_bad_visibility():
    from dirt_amd import shading
    light = shading.pbr_directional_light((0., 0., -1.), (1., 1., 1.))
    kw = dict(colors=4, material=10, normals=7, positions=1, mask=0, camera_position=(0., 0., 4.))
    for g, lights, vis, text in (
            (G, [light], torch.zeros(4, 5, 2), "visibility must have shape [4, 5, 1] (the G-buffer's [4, 5, 12] with one channel per light), got [4, 5, 2]"),
            (G, [light, light], torch.zeros(4, 5, 1), "visibility must have shape [4, 5, 2] (the G-buffer's [4, 5, 12] with one channel per light), got [4, 5, 1]"),
            (G, [light], torch.zeros(5, 4, 1), "visibility must have shape [4, 5, 1] (the G-buffer's [4, 5, 12] with one channel per light), got [5, 4, 1]"),
            (G, [light], torch.zeros(20, 1), "visibility must have shape [4, 5, 1] (the G-buffer's [4, 5, 12] with one channel per light), got [20, 1]"),
            (G[None], [light], torch.zeros(4, 5, 1), "visibility must have shape [1, 4, 5, 1] (the G-buffer's [1, 4, 5, 12] with one channel per light), got [4, 5, 1]"),
            (G, [light], torch.zeros(4, 5, 1, dtype=torch.int32), 'visibility must be floating-point, got torch.int32'),
            (G, [light], torch.zeros(4, 5, 1, dtype=torch.bool), 'visibility must be floating-point, got torch.bool'),
            (G, [light], torch.zeros(4, 5, 1, device='meta'), 'visibility is on meta, the G-buffer on cpu'),
            (G, [], torch.zeros(4, 5, 0), 'visibility needs at least one light, got none'),
            (G, [light], 3, 'visibility must be a tensor (there is no channel-index form), got 3')):
        with pytest.raises(ValueError) as e:      # (as tests/test_shade_pbr.py checks `_check_pbr_arguments`: the checks alone, on the CPU)
            shading._check_pbr_visibility(g, len(lights), vis)
        assert str(e.value) == text, str(e.value)
    assert shading._check_pbr_visibility(G, 1, None) is None and shading._check_pbr_visibility(G, 0, None) is None
    assert shading._check_pbr_visibility(G, 2, torch.zeros(4, 5, 2, dtype=torch.float64)) is None
    # a good visibility reaches the device check of the call
    with pytest.raises(RuntimeError) as e:
        shading.shade_gbuffer_pbr(G, [light], visibility=torch.zeros(4, 5, 1), **kw)
    assert str(e.value) == 'dirt_amd.shading.shade_gbuffer_pbr' + B.CPU


def test_the_symbols_are_exported_and_declared():
    import inspect
    from dirt_amd import _lib, build, lighting, shading
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for symbol in ('dirt_shade_pbr_visibility_forward', 'dirt_shade_pbr_visibility_backward'):
        assert symbol in _lib.SYMBOLS and re.search(r'\b%s\(' % symbol, header)
    assert _lib.ABI_VERSION == 4 and '#define DIRT_ABI_VERSION 4' in header
    assert 'dirt_shade_pbr_visibility.hip' in build.SOURCES and 'dirt_shade_pbr_visibility.hip' not in build.PER_SOURCE_FLAGS
    assert inspect.signature(shading.shade_gbuffer_pbr).parameters['visibility'].default is None
    assert inspect.signature(lighting.cook_torrance).parameters['visibility'].default is None
    lib = _lib.load()
    assert len(lib.dirt_shade_pbr_visibility_forward.argtypes) == len(lib.dirt_shade_pbr_forward.argtypes) + 2
    assert len(lib.dirt_shade_pbr_visibility_backward.argtypes) == len(lib.dirt_shade_pbr_backward.argtypes) + 3
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_shade_pbr.hip')).read()
    assert 'atomicAdd' not in source and 'atomic_' not in source


def test_the_new_kernels_use_no_scratch_memory():
    from dirt_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if 'shade_visible_pbr_' in k}
    assert len(res) == 17, sorted(res)       # the forward and <lights 1..4, PARAMS, GBUF>
    for name, v in res.items():
        assert v['scratch'] == 0 and v['lds'] <= 16384, (name, v)


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib, build
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)
    E = _lib.E_INVALID_ARGUMENT

    def tail(kw):
        d = dict(scenes=1, pixels=64, cg=12, cs=0, ms=0, vs=2, oc=4, omat=10, on=7, op=1, om=0, ps=1, lights=2, kinds=2, mr=0.04, f0=0.04, lo=0., hi=1.,
                 flags=1)
        d.update(kw)
        return tuple(d[k] for k in ('scenes', 'pixels', 'cg', 'cs', 'ms', 'vs', 'oc', 'omat', 'on', 'op', 'om', 'ps', 'lights', 'kinds', 'mr', 'f0', 'lo',
                                    'hi', 'flags')) + (None,)

    def fwd(g=one, c=None, m=None, v=one, p=one, out=one, **kw):
        return lib.dirt_shade_pbr_visibility_forward(g, c, m, v, p, out, *tail(kw))

    def bwd(g=one, c=None, m=None, v=one, p=one, go=one, gg=one, gc=None, gm=None, gv=one, gp=one, scratch=one, nbytes=1 << 20, **kw):
        return lib.dirt_shade_pbr_visibility_backward(g, c, m, v, p, go, gg, gc, gm, gv, gp, scratch, nbytes, *tail(kw))

    for who, call in (('dirt_shade_pbr_visibility_forward', fwd), ('dirt_shade_pbr_visibility_backward', bwd)):
        for kw, text in ((dict(lights=0, kinds=0, vs=0), '%s: a visibility needs at least one light (dirt_shade_pbr_forward / _backward shade without one)'),
                         (dict(vs=1), "%s: visibility_stride=1, a pixel's visibility is 2 floats (one per light)"),
                         (dict(lights=4, kinds=0, vs=3), "%s: visibility_stride=3, a pixel's visibility is 4 floats (one per light)"),
                         (dict(vs=-6), "%s: visibility_stride=-6, a pixel's visibility is 2 floats (one per light)"),
                         (dict(v=None), '%s: visibility is NULL with pixels to shade'),
                         # the existing refusals, through the shared checks
                         (dict(cg=1025), '%s: 1025 G-buffer channels, 1..1024'), (dict(pixels=-5), '%s: negative sizes (scenes=1 pixels=-5)'),
                         (dict(scenes=65536), '%s: 65536 scenes, at most 65535'),
                         (dict(c=one, cs=2), "%s: color_stride=2, a pixel's colour is 3 floats"),
                         (dict(m=one, ms=1), "%s: material_stride=1, a pixel's material is 2 floats"),
                         (dict(lights=5, kinds=0, vs=5), '%s: 5 lights, at most 4'), (dict(lights=-1, kinds=0), '%s: -1 lights, at most 4'),
                         (dict(lights=2, kinds=4), '%s: light_kinds 0x4 has bits beyond 2 lights'),
                         (dict(ps=2), '%s: param_scenes=2 is neither 1 nor scenes=1'), (dict(flags=3), '%s: unknown flags 0x3'),
                         (dict(oc=9), '%s: material (channel 10) overlaps colors (channel 9)'),
                         (dict(om=12), '%s: mask at channel 12 does not fit in 12 channels'),
                         (dict(mr=0.), '%s: min_roughness=0 is not in (0, 1]'), (dict(f0=2.), '%s: dielectric_f0=2 is not in [0, 1]'),
                         (dict(lo=1., hi=0.), '%s: clamp bounds lo=1 > hi=0')):
            assert call(**kw) == E, (who, kw)
            assert lib.dirt_last_error().decode() == text % who, (who, kw, lib.dirt_last_error())
        assert call(pixels=0) == 0 and call(scenes=0) == 0 and lib.dirt_last_error() == b''
        assert call(pixels=0, v=None) == 0      # nothing to shade: the visibility is not looked at
        assert call(pixels=0, lights=0, kinds=0) == E      # but a call without a light is refused whatever its size
    assert fwd(out=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_pbr_visibility_forward: gbuffer / params / out is NULL'
    assert bwd(go=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_pbr_visibility_backward: gbuffer / params / grad_out is NULL'
    assert bwd(gc=one) == E
    assert lib.dirt_last_error().decode() == "dirt_shade_pbr_visibility_backward: grad_colors without colors (the channel path's is part of grad_gbuffer)"
    assert bwd(gg=None, gp=None, gv=None) == 0 and bwd(gg=None, gp=None, gv=None, v=None) == 0      # nothing wanted: nothing is launched
    # the visibility's gradient alone counts as wanted: the call goes on to its next check
    assert bwd(gg=None, gp=None, v=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_pbr_visibility_backward: visibility is NULL with pixels to shade'
    need = lib.dirt_shade_pbr_scratch_bytes(1, 64, 2)
    assert bwd(nbytes=need - 1) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_pbr_visibility_backward: scratch is NULL or smaller than dirt_shade_pbr_scratch_bytes (99 < 100)'
    assert bwd(gp=None, scratch=None, nbytes=0, pixels=0) == 0


# ---- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('name', [k for k in CASES if k != 'zero_column'])
def test_cases_against_the_restatement(gpu, name):
    compare(name, gpu)


PATTERNS = [('flat_2', w[:2] + (False, False) + w[2:]) for w in itertools.product((True, False), repeat=3)] + \
           [('flat_3', w) for w in itertools.product((True, False), repeat=5)] + \
           [(name, w + (False, False, True)) for name in ('flat_1', 'tensors_4') for w in itertools.product((True, False), repeat=2)]


@pytest.mark.gpu
@pytest.mark.parametrize('name, want', PATTERNS, ids=['%s-%s' % (n, ''.join(c for c, on in zip('gpcmv', w) if on) or 'none') for n, w in PATTERNS])
def test_every_pattern_of_wanted_gradients(gpu, name, want):
    """Channels (two lights) and tensors (three) through every pattern of wanted gradients over (G-buffer, parameters, colour
    tensor, material tensor, visibility), the visibility alone and none included; one and four lights through the four (G-buffer,
    parameters) patterns with the visibility's: together the sixteen backward kernels.  What is not wanted stays absent."""
    case, ref, got = compare(name, gpu, want)
    tensors = case.colors is not None
    assert ('d_gbuffer' in got) == want[0] and ('d_params' in got) == want[1] and ('d_visibility' in got) == want[4]
    assert ('d_colors' in got) == (want[2] if tensors else want[0]) and ('d_material' in got) == (want[3] if tensors else want[0])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['flat_1', 'flat_4', 'tensors_1', 'tensors_4'])
def test_all_ones_give_the_bits_of_the_call_without_a_visibility(gpu, name):
    case, _ = case_of(name)
    shape = case.shape or (case.n,)
    ones = torch.ones(shape + (len(case.kinds),), device=gpu, requires_grad=True)
    without, with_ones = shade(case, gpu, visibility=None), shade(case, gpu, visibility=ones)
    assert set(without) == set(with_ones)
    same_bits(without, with_ones)
    assert ones.grad is not None and bool(torch.isfinite(ones.grad).all()) and bool(ones.grad.any())


@pytest.mark.gpu
def test_a_column_of_zeros_is_the_call_without_that_light(gpu):
    case, ref = case_of('zero_column')
    got = shade(case, gpu)
    check(case, got, ref, 'zero_column')      # d visibility[..., 1] included
    assert bool(got['d_visibility'][:, 1].any())
    removed = shade(case, gpu, drop=1)
    assert torch.equal(got['out'], removed['out'])
    assert not bool(got['d_params']['light1.color'].any()) and not bool(got['d_params']['light1.vector'].any())


@pytest.mark.gpu
def test_a_slice_is_read_in_place(gpu, monkeypatch):
    """`wide[..., 1:5]` of a six-channel tensor: the pointer the C ABI receives is the tensor's own at stride 6, every result has
    the bits of the run on a contiguous copy, and `wide.grad` is zero outside the slice."""
    from dirt_amd import _stage, _lib
    case, ref = case_of('flat_4')
    seen = []
    call = _stage.call
    monkeypatch.setattr(_stage, 'call', lambda f, dev, *args, **kw: (seen.append((f, args)), call(f, dev, *args, **kw))[1])
    lib = _lib.load()
    plain = shade(case, gpu)
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_pbr_visibility_forward]
    assert forward[9:12] == (0, 0, 4)
    wide = torch.full((case.n, 6), 1.e30, device=gpu)
    wide[:, 1:5] = torch.from_numpy(case.vis).to(gpu)
    wide.requires_grad_(True)
    del seen[:]
    got = shade(case, gpu, visibility=wide[:, 1:5])
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_pbr_visibility_forward]
    (backward,) = [a for f, a in seen if f is lib.dirt_shade_pbr_visibility_backward]
    assert forward[3] == wide.data_ptr() + 4 and forward[9:12] == (0, 0, 6)
    assert backward[3] == forward[3] and backward[16:19] == (0, 0, 6)
    same_bits(plain, got, keys=list(got))
    assert torch.equal(wide.grad[:, 1:5], plain['d_visibility']) and not bool(wide.grad[:, 0].any()) and not bool(wide.grad[:, 5].any())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['c257', 'scenes_per_scene', 'flat_4'])
def test_two_runs_give_the_same_bits(gpu, name):
    case, _ = case_of(name)
    a, b = shade(case, gpu), shade(case, gpu)
    assert set(a) == set(b)
    same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 255, 256, 257, FLAT])
def test_the_c_abi_writes_inside_its_outputs(gpu, lib, n):
    """Guard values around out and grad_visibility (and grad_gbuffer, grad_params, the scratch) stay; every element inside is
    written, with the wrapper's bits for the first n pixels."""
    from dirt_amd import _lib
    case, _ = case_of('flat_2')
    guard, nl = 7, len(case.kinds)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)   # noqa: E731
    g, vis, go = t(case.g[:n]), t(case.vis[:n]), t(case.go[:n])
    block = np.zeros((1, 9 + 8 * nl), np.float32)
    block[0, 0:3], block[0, 3:6], block[0, 6:9] = case.params['ambient'], case.params['background'], case.params['camera_position']
    for i in range(nl):
        block[0, 9 + 8 * i:12 + 8 * i], block[0, 12 + 8 * i:15 + 8 * i] = case.params['light%d.vector' % i], case.params['light%d.color' % i]
    block = t(block)
    nbytes = lib.dirt_shade_pbr_scratch_bytes(1, n, nl)
    bufs = {}
    for k, count in (('out', 3 * n), ('gg', case.cg * n), ('gv', nl * n), ('gp', 9 + 8 * nl), ('scratch', nbytes // 4)):
        full = torch.full((count + 2 * guard,), 12345., device=gpu)
        bufs[k] = (full, full[guard:guard + count])
    lay = case.layout
    kinds = sum(1 << i for i, kind in enumerate(case.kinds) if kind == P)
    tail = (1, n, case.cg, 0, 0, nl, lay['colors'], lay['material'], lay['normals'], lay['positions'], lay['mask'], 1, nl, kinds, B.MIN_ROUGHNESS,
            B.DIELECTRIC_F0, 0., 1., _lib.SHADE_CLAMP, None)
    torch.cuda.synchronize()
    _lib.check(lib.dirt_shade_pbr_visibility_forward(g.data_ptr(), None, None, vis.data_ptr(), block.data_ptr(), bufs['out'][1].data_ptr(), *tail))
    _lib.check(lib.dirt_shade_pbr_visibility_backward(g.data_ptr(), None, None, vis.data_ptr(), block.data_ptr(), go.data_ptr(), bufs['gg'][1].data_ptr(),
                                                      None, None, bufs['gv'][1].data_ptr(), bufs['gp'][1].data_ptr(), bufs['scratch'][1].data_ptr(),
                                                      nbytes, *tail))
    torch.cuda.synchronize()
    for k, (full, inner) in bufs.items():
        assert bool((full[:guard] == 12345.).all()) and bool((full[-guard:] == 12345.).all()), k
        assert not bool((inner == 12345.).any()), k
    got = shade(case, gpu)
    assert torch.equal(bufs['out'][1].reshape(n, 3), got['out'][:n]) and torch.equal(bufs['gv'][1].reshape(n, nl), got['d_visibility'][:n])
    assert torch.equal(bufs['gg'][1].reshape(n, case.cg), got['d_gbuffer'][:n])
    if n == case.n:
        assert torch.equal(bufs['gp'][1][12:15], got['d_params']['light0.color']) and torch.equal(bufs['gp'][1][17:20], got['d_params']['light1.vector'])


@pytest.mark.gpu
def test_graph_capture_replays_on_new_visibility_values(gpu):
    """Forward and backward captured with torch.cuda.graph, replayed once after the visibility was overwritten in place: the
    replay has the eager bits of the new values."""
    from dirt_amd import shading
    case, _ = case_of('flat_3')
    t = lambda x: torch.from_numpy(x).to(gpu)   # noqa: E731
    new = RV.dyadic(np.random.default_rng(7200), 0., 1., case.vis.shape, RV.VISIBILITY_BITS)
    new_leaf = t(new).requires_grad_(True)
    eager = shade(case, gpu, visibility=new_leaf)
    eager['d_visibility'] = new_leaf.grad
    g, col, mat, vis = (t(x).requires_grad_(True) for x in (case.g, case.colors, case.material, case.vis))
    prm = {k: t(v).requires_grad_(True) for k, v in case.params.items()}
    go = t(case.go)
    names = list(prm)

    def step():
        lights = [(kind, prm['light%d.vector' % i], prm['light%d.color' % i]) for i, kind in enumerate(case.kinds)]
        out = shading.shade_gbuffer_pbr(g, lights, colors=col, material=mat, normals=case.layout['normals'], positions=case.layout['positions'],
                                        mask=case.layout['mask'], ambient=prm['ambient'], camera_position=prm['camera_position'],
                                        background=prm['background'], clamp=case.kw['clamp'], visibility=vis)
        return (out,) + torch.autograd.grad(out, [g, col, mat, vis] + [prm[k] for k in names], go)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        vis.copy_(t(new))
    for x in captured:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(t(new), t(case.vis))
    for x, k in zip(captured[:4], ('out', 'd_gbuffer', 'd_colors', 'd_material')):
        assert torch.equal(x.reshape(eager[k].shape), eager[k]), k
    assert torch.equal(captured[4], eager['d_visibility'])
    for x, k in zip(captured[5:], names):
        assert torch.equal(x, eager['d_params'][k]), k


def _shadow_scene(dev):
    """A 17 x 19 G-buffer (mask, position, colour, normal, roughness, metalness) of random pixels inside two lights' 5 x 3 shadow
    maps: orthographic lights along -z and -x, the maps' depths around the pixels' own, so that the comparison is mixed."""
    rng = np.random.default_rng(7300)
    h, w = IMAGE
    layout = dict(mask=0, positions=1, colors=4, normals=7, material=10)
    g, _, _ = R.random_pixels(rng, h * w, 12, layout)
    g[:, 1:4] *= 0.8
    eye = np.eye(4, dtype=np.float32)
    along_x = np.asarray([[0., 0., 1., 0.], [0., 1., 0., 0.], [-1., 0., 0., 0.], [0., 0., 0., 1.]], np.float32)      # clip (z, y, -x)
    matrices = np.stack([eye, along_x])
    maps = rng.uniform(-0.6, 0.6, (2, 5, 3)).astype(np.float32)
    lights = [(D, np.asarray([0., 0., -1.], np.float32), np.asarray([0.5, 0.375, 0.25], np.float32)),
              (P, np.asarray([2., 1., 3.], np.float32), np.asarray([0.25, 0.5, 0.375], np.float32))]
    return layout, g.reshape(h, w, 12), matrices, maps, lights


@pytest.mark.gpu
def test_shadow_visibility_into_the_shader_against_the_composed_route(gpu, monkeypatch):
    """`shadow_visibility` -> `shade_gbuffer_pbr(visibility=)` against the route composed of calls without the operand: a call per
    light times its column, the ambient call, one clamp.  Pixels and d visibility per element within the sum of both routes'
    allowances, 2 x KERNEL x F32 x mass (masses from the restatement on the looked-up visibility; the composed route's own
    products and sums round within a few 6e-8 of the same mass).  The look-up's output is passed as it is (no copy).  The
    gradients at the shadow maps and the light matrices come through the look-up's backward, where no mass is at hand (and the
    maps' is summed with atomics): as tests/test_shade_pbr.py does there, an element agrees if |a - b| <= 1e-3 max(|a|, |b|) or
    both are below 1e-7; at most 1 % may not."""
    from dirt_amd import _stage, _lib, shading
    layout, g_np, matrices_np, maps_np, lights_np = _shadow_scene(gpu)
    ambient, background, camera = (0.125, 0.25, 0.125), (0.25, 0.125, 0.5), (0.25, -0.25, 4.)
    seen = []
    call = _stage.call
    monkeypatch.setattr(_stage, 'call', lambda f, dev, *args, **kw: (seen.append((f, args)), call(f, dev, *args, **kw))[1])
    go = torch.from_numpy(np.random.default_rng(7301).standard_normal(IMAGE + (3,)).astype(np.float32)).to(gpu)
    results = []
    for fused in (True, False):
        g = torch.from_numpy(g_np).to(gpu)
        maps, mats = (torch.from_numpy(x).to(gpu).requires_grad_(True) for x in (maps_np, matrices_np))
        lights = [(kind, torch.from_numpy(v).to(gpu), torch.from_numpy(c).to(gpu)) for kind, v, c in lights_np]
        vis = shading.shadow_visibility(g, maps, mats, positions=layout['positions'], mask=layout['mask'], kernel=3, bias=0.01, softness=0.25)
        vis.retain_grad()
        kw = dict(camera_position=camera, **layout)
        if fused:
            out = shading.shade_gbuffer_pbr(g, lights, ambient=ambient, background=background, visibility=vis, **kw)
            (forward,) = [a for f, a in seen if f is _lib.load().dirt_shade_pbr_visibility_forward]
            assert forward[3] == vis.data_ptr() and forward[11] == 2
        else:
            lit = sum(shading.shade_gbuffer_pbr(g, [light], clamp=None, **kw) * vis[..., i:i + 1] for i, light in enumerate(lights))
            out = torch.clamp(lit + shading.shade_gbuffer_pbr(g, [], ambient=ambient, background=background, clamp=None, **kw), 0., 1.)
        out.backward(go)
        results.append((out.detach(), vis.detach(), vis.grad, maps.grad, mats.grad))
    (oa, va, dva, sa, ma), (ob, vb, dvb, sb, mb) = results
    assert torch.equal(va, vb) and 0.1 < float(((va > 0) & (va < 1)).float().mean()) and bool((va == 1).any())
    ref = RV.compose(g_np.reshape(-1, 12), lights_np, layout, va.reshape(-1, 2).cpu().numpy(), ambient=ambient, background=background,
                     camera_position=camera, grad_out=go.reshape(-1, 3).cpu().numpy(), exact=False)
    for what, a, b, r, mass, f in (('pixels', oa, ob, ref['out'], ref['mass_out'], F32['pixels']),
                                   ('d visibility', dva, dvb, ref['d_visibility'], ref['mass_visibility'], F32['d_visibility'])):
        a, b = a.cpu().double().reshape(mass.shape), b.cpu().double().reshape(mass.shape)
        print(what, float(((a - b).abs() / mass.clamp_min(1e-300)).max()) / f, float(((a - r).abs() / mass.clamp_min(1e-300)).max()) / f)
        assert bool(((a - b).abs() <= 2 * KERNEL * f * mass).all()), what
        assert bool(((a - r).abs() <= (KERNEL + 1) * f * mass).all()), what      # the visibility is not dyadic here: one more rounding of k s
    for what, a, b in (('d shadow maps', sa, sb), ('d light matrices', ma, mb)):
        a, b = a.cpu().double(), b.cpu().double()
        agree = ((a - b).abs() <= 1e-3 * torch.maximum(a.abs(), b.abs())) | ((a.abs() < 1e-7) & (b.abs() < 1e-7))
        print('%s: %d of %d elements excluded' % (what, int((~agree).sum()), agree.numel()))
        assert 1. - float(agree.double().mean()) <= 0.01 and bool(a.abs().max() > 0), what


@pytest.mark.gpu
def test_the_example_lowers_its_loss(gpu):
    ex = B._load_example('fit_light_shadow_pbr_fused')
    losses, before, after = ex.fit(width=64, height=64, steps=25, device=gpu)
    assert losses[-1] < losses[0] and after < before
